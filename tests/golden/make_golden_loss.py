#!/usr/bin/env python3
"""Golden vectors for the training loss and its statistics (gnn_cca_amd.loss, csrc/loss.hip).

The reference's lines are READ from /root/reference at run time and executed unmodified, as tests/golden/make_golden_post2.py does:
  * train.py:51-208, `compute_loss_acc` (the loss, the per-class losses, the three precisions, the per-step probabilities);
  * train.py:460-469, the per-step, per-class mean probabilities;
  * train.py:472-479, the six AverageMeter updates, and train.py:508-514, the epoch entries of list_mean_probs_history;
  * main_training.py:258-268, the criterion and criterion_no_reduction of each configuration, against the reference's own libs.utils
    (FocalLoss_binary, AverageMeter; imported unmodified with the torch_scatter / cv2 stand-ins of make_golden.py / make_golden_post.py).
The gradients are torch autograd of the returned loss with respect to every step's logits.  `.cuda()` is the identity here (the build
container has no GPU).  Only numbers are stored (tests/golden/post2_train_loss.npz).  Build container only:

    python tests/golden/make_golden_loss.py
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_torch_scatter_standin  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "post2_train_loss.npz")
CONFIGS = (("BCE", 0.0), ("BCE_weighted", 4.5), ("BCE_weighted", 9.0), ("Focal", 0.0))
BATCH_SIZE = 64   # config_training.yaml:54


def lines(path, first, last, dedent=True):
    with open(os.path.join(REF, path)) as f:
        text = "".join(f.readlines()[first - 1:last])
    return textwrap.dedent(text) if dedent else text


class Batch:
    pass


class _Plt:
    def __getattr__(self, name):
        return lambda *a, **k: None


def criteria(utils, name, pw):
    cfg = {"TRAINING": {"LOSS": {"NAME": name}}, "POSITIVE_WEIGHT": {"DS": pw}, "DATASET_TRAIN": {"NAME": ["DS"]}}
    ns = {"CONFIG": cfg, "utils": utils, "nn": nn, "torch": torch}
    exec(compile(lines("main_training.py", 258, 268), "<reference main_training.py:258-268>", "exec"), ns)
    return ns["criterion"], ns["criterion_no_reduction"]


def inputs(rng):
    """name -> (logits fp32 [S, E], labels fp32 [E])"""
    sets = {}
    t = np.load(os.path.join(HERE, "bwd_terrace32.npz"))
    lab768 = np.asarray(t["labels"], dtype=np.float32).reshape(-1)
    assert lab768.shape == (768,)

    def logits(s, e, scale=3.0):
        x = (scale * rng.standard_normal((s, e))).astype(np.float32)
        if e >= 16:   # exact 0, a small negative that sigmoid rounds to 0.5, saturated values
            x[:, :6] = np.array([0.0, -1e-9, 100.0, -100.0, 1e-9, -0.0], dtype=np.float32)
        return x

    sets["e0_s3"] = (np.zeros((3, 0), np.float32), np.zeros(0, np.float32))
    sets["e1_s1_pos"] = (np.array([[0.3]], np.float32), np.ones(1, np.float32))
    sets["e1_s3_neg"] = (np.array([[-0.7], [-1e-9], [2.0]], np.float32), np.zeros(1, np.float32))
    sets["terrace_s1"] = (logits(1, 768), lab768)
    sets["terrace_s3"] = (logits(3, 768), lab768)
    sets["terrace_s8"] = (logits(8, 768, 2.0), lab768)
    sets["allpos_s3"] = (logits(3, 768), np.ones(768, np.float32))
    sets["allneg_s3"] = (logits(3, 768), np.zeros(768, np.float32))
    lab20k = (rng.random(20000) < 0.18).astype(np.float32)
    sets["big_s1"] = (logits(1, 20000, 4.0), lab20k)
    sets["big_s3"] = (logits(3, 4096, 4.0), lab20k[:4096])
    return sets


def run_case(compute_loss_acc, crit, crit_nr, x, y, mode, mean_probs=None):
    s, e = x.shape
    steps = [torch.from_numpy(x[k].copy()).view(e, 1).requires_grad_(True) for k in range(s)]
    b = Batch()
    b.edge_labels = torch.from_numpy(y.copy())
    outputs = {"classified_edges": steps}
    loss, p1, p0, p, l1, l0, list_pred_probs = compute_loss_acc(outputs, b, crit, crit_nr, mode)
    list_mean_probs = mean_probs if mean_probs is not None else {c: {f"step{k}": [] for k in range(s)} for c in ("0", "1")}
    ns = {"torch": torch, "data_batch": b, "list_pred_probs": list_pred_probs, "list_mean_probs": list_mean_probs}
    exec(compile(lines("train.py", 460, 469), "<reference train.py:460-469>", "exec"), ns)
    mp = np.array([[float(list_mean_probs[c][f"step{k}"][-1]) for c in ("0", "1")] for k in range(s)], dtype=np.float32)
    loss.backward()
    grads = np.stack([t.grad.numpy().reshape(-1) for t in steps]).astype(np.float32)
    return dict(loss=loss, p1=p1, p0=p0, p=p, l1=l1, l0=l0, mean_prob=mp, grads=grads, b=b)


def main():
    _install_torch_scatter_standin()
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, REF)
    from libs import utils  # the reference, unmodified
    torch.Tensor.cuda = lambda self, *a, **k: self   # no device here: the reference's .cuda() calls become the identity

    ns = {"np": np, "torch": torch, "F": F}
    exec(compile(lines("train.py", 51, 208, dedent=False), "<reference train.py:51-208>", "exec"), ns)
    compute_loss_acc = ns["compute_loss_acc"]

    rng = np.random.default_rng(2024)
    sets = inputs(rng)
    out = {"set_names": np.array(sorted(sets))}
    for name, (x, y) in sets.items():
        out[f"x__{name}"] = x
        out[f"y__{name}"] = y.astype(np.uint8)
    cases = []
    for name in sorted(sets):
        x, y = sets[name]
        for crit_name, pw in CONFIGS:
            crit, crit_nr = criteria(utils, crit_name, pw)
            for mode in ("train", "validate"):
                r = run_case(compute_loss_acc, crit, crit_nr, x, y, mode)
                key = f"{name}__{crit_name}{'' if pw == 0 else pw}__{mode}"
                cases.append(key)
                tup = [float(r["loss"]), float(np.sum(np.asarray(r["p1"])) / len(r["p1"])), float(np.sum(np.asarray(r["p0"])) / len(r["p0"])),
                       float(np.sum(np.asarray(r["p"])) / len(r["p"])), float(r["l1"]), float(r["l0"])]
                out[f"stats__{key}"] = np.array(tup, dtype=np.float64)   # loss, precision1, precision0, precision, loss_class1, loss_class0
                out[f"meta__{key}"] = np.array([CONFIGS.index((crit_name, pw)), mode == "validate", pw], dtype=np.float64)
                out[f"mp__{key}"] = r["mean_prob"]
                # gradients (file size): validate once per input set (plain BCE whatever the criterion), one pos_weight, the big sets
                # for Focal only
                keep = (mode == "train" and pw != 4.5) or crit_name == "BCE"
                if name.startswith("big"):
                    keep = mode == "train" and crit_name == "Focal"
                if keep:
                    out[f"grad__{key}"] = r["grads"]
    out["case_names"] = np.array(cases)

    # an epoch of train iterations through the reference's meters: train.py:472-479 and the list_mean_probs_history lines 508-514
    crit, crit_nr = criteria(utils, "BCE", 0.0)
    epoch = ["terrace_s3", "allpos_s3", "big_s3", "allneg_s3", "terrace_s3", "big_s3"]
    s = 3
    list_mean_probs = {c: {f"step{k}": [] for k in range(s)} for c in ("0", "1")}
    meters = {n: utils.AverageMeter(n) for n in ("train_losses", "train_losses1", "train_losses0", "train_precision_class1",
                                                  "train_precision_class0", "train_precision")}
    vals = []
    for name in epoch:
        x, y = sets[name]
        r = run_case(compute_loss_acc, crit, crit_nr, x, y, "train", list_mean_probs)
        ns = dict(meters)
        ns.update(np=np, CONFIG={"TRAINING": {"BATCH_SIZE": {"TRAIN": BATCH_SIZE}}}, loss=r["loss"], loss_class1=r["l1"], loss_class0=r["l0"],
                  precision1=r["p1"], precision0=r["p0"], precision=r["p"])
        exec(compile(lines("train.py", 472, 479), "<reference train.py:472-479>", "exec"), ns)
        vals.append([meters["train_losses"].val, meters["train_losses1"].val, meters["train_losses0"].val, meters["train_precision_class1"].val,
                     meters["train_precision_class0"].val, meters["train_precision"].val])
    hist = {c: {f"step{k}": [] for k in range(s)} for c in ("0", "1")}
    ns = {"np": np, "torch": torch, "plt": _Plt(), "nsteps": s, "list_mean_probs": list_mean_probs, "list_mean_probs_history": hist}
    exec(compile(lines("train.py", 508, 514), "<reference train.py:508-514>", "exec"), ns)
    order = ("train_losses", "train_losses1", "train_losses0", "train_precision_class1", "train_precision_class0", "train_precision")
    out["epoch_sets"] = np.array(epoch)
    out["epoch_batch_size"] = np.array(BATCH_SIZE)
    out["epoch_values"] = np.array(vals, dtype=np.float64)                                   # [K, 6] what each meter received
    out["epoch_mean_probs"] = np.array([[[float(t) for t in list_mean_probs[c][f"step{k}"]] for c in ("0", "1")] for k in range(s)],
                                       dtype=np.float32)                                   # [S, 2, K]
    out["epoch_meters"] = np.array([[meters[n].val, meters[n].sum, meters[n].count, meters[n].avg] for n in order], dtype=np.float64)
    out["epoch_mean_probs_history"] = np.array([[hist[c][f"step{k}"][0] for c in ("0", "1")] for k in range(s)], dtype=np.float32)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
