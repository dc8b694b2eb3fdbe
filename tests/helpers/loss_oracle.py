"""Torch restatement of the training loss and its statistics (compute_loss_acc, train.py:51-208, and train.py:460-469) in the form the
kernels compute it (csrc/loss.hip): per-edge terms in fp32 with the stable BCE-with-logits form, sums and means in fp64.  Runs on any
device; autograd through it gives the reference gradients.  The checker of gnn_cca_amd.loss, not a product path."""
import numpy as np
import torch
import torch.nn.functional as F

CONFIGS = (("BCE", 0.0), ("BCE_weighted", 4.5), ("BCE_weighted", 9.0), ("Focal", 0.0))


def edge_loss(logits, labels, criterion="BCE", pos_weight=None, focusing_param=5.0, balance_param=0.9, mode="train"):
    """logits [S, E] fp32 (may require grad), labels [E] fp32 -> dict: loss (fp64 0-d, differentiable), loss_class1, loss_class0,
    precision1 / precision0 / precision (Python floats), mean_prob float64 [S, 2], n_pos, n_neg, coef [S]."""
    s_steps, e = logits.shape
    y = labels.reshape(-1).to(torch.float32)
    pos, neg = y == 1, y == 0
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    weighted = mode == "train" and criterion == "BCE_weighted"
    focal = mode == "train" and criterion == "Focal"
    w = 1.0 + (float(pos_weight) - 1.0) * y if weighted else torch.ones_like(y)
    a, g = float(balance_param), float(focusing_param)
    loss = torch.zeros((), dtype=torch.float64, device=logits.device)
    l1 = l0 = 0.0
    mean_prob = np.zeros((s_steps, 2))
    coef = np.ones(s_steps)
    nan = float("nan")
    for s in range(s_steps):
        x = logits[s]
        l = (1.0 - y) * x - w * F.logsigmoid(x)
        m = l.double().sum() / e   # 0 / 0 = NaN for E = 0, as torch.mean of an empty tensor
        if focal:
            md = float(m.detach())
            pt = np.exp(-md)
            coef[s] = a * ((1 - pt) ** g + (g * (1 - pt) ** (g - 1) * pt * md if g != 0 and 1 - pt > 0 else 0.0))
            term = a * ((1.0 - torch.exp(-m)) ** g * m)
            ln = a * ((1.0 - torch.exp(-l)) ** g * l)
        else:
            term, ln = m, l
        loss = loss + term
        ln = ln.detach().double()
        l1 += float(ln[pos].sum()) / n_pos if n_pos else nan
        l0 += float(ln[neg].sum()) / n_neg if n_neg else nan
        p = (1.0 / (1.0 + torch.exp(-x.detach()))).double()
        mean_prob[s, 0] = float(p[neg].sum()) / n_neg if n_neg else 0.5
        mean_prob[s, 1] = float(p[pos].sum()) / n_pos if n_pos else 0.5
    x = logits[-1].detach()
    pred1 = (1.0 / (1.0 + torch.exp(-x))) >= 0.5
    hit1, hit0 = int((pred1 & pos).sum()), int((~pred1 & neg).sum())
    hits = hit1 + hit0
    return dict(loss=loss, loss_class1=l1, loss_class0=l0,
                precision1=0.0 if hit1 == 0 else (hit1 / n_pos) * 100.0,
                precision0=0.0 if hit0 == 0 else (hit0 / n_neg) * 100.0,
                precision=0.0 if hits == 0 else (hits / e) * 100.0,
                mean_prob=mean_prob, n_pos=n_pos, n_neg=n_neg, coef=coef)


def golden_cases(z):
    """Yields (key, dict) for every case of tests/golden/post2_train_loss.npz."""
    for key in z["case_names"]:
        key = str(key)
        name = key.split("__")[0]
        ci, validate, pw = z[f"meta__{key}"]
        crit, _ = CONFIGS[int(ci)]
        yield key, dict(x=z[f"x__{name}"], y=z[f"y__{name}"].astype(np.float32), criterion=crit, pos_weight=float(pw) if pw else None,
                        mode="validate" if validate else "train", stats=z[f"stats__{key}"], mean_prob=z[f"mp__{key}"],
                        grad=z[f"grad__{key}"] if f"grad__{key}" in z.files else None)


def close(got, want, rtol=1e-6):
    """NaN exactly where `want` has NaN, else |got - want| <= rtol |want| (absolute rtol when want == 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.all(np.abs(got[ok] - want[ok]) <= rtol * np.abs(want[ok]) + rtol * (want[ok] == 0)))
