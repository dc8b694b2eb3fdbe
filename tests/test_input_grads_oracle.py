"""Row N3, input gradients: the autograd oracle (oracle.TorchTrainOracle lets gradients through when it is handed torch tensors that
require grad) against d loss / d x and d loss / d edge_attr of the reference's own module (tests/golden/input_grads/igrad_*.npz,
make_golden_input_grads.py).  Pins the oracle the larger GPU cases of test_gpu_input_grads.py are checked against.  CPU only.

Also home of what both files share: the fixture loader and the RELATIVE accuracy criterion of these gradients,
    e(t) = max|t - t64| / max|t64|          (t64: the reference after .double(); the gradients are small, so an absolute
                                             bound scaled by max(1, |ref|) would be vacuous)
with the reference's own fp32 run as the yardstick, e_ref = e(t32).
"""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle.mpn_oracle import TorchTrainOracle
from test_backward_oracle import _golden_thread_count, load_bwd  # noqa: F401  (autouse: the recording's thread count)

EPS = 2.0 ** -23
IGRAD_DIR = os.path.join(GOLDEN_DIR, "input_grads")


def _cases():
    out = []
    for p in sorted(glob.glob(os.path.join(IGRAD_DIR, "igrad_*.npz"))):
        name = os.path.basename(p)[6:-4]
        prefix = "bwd_" if os.path.exists(os.path.join(GOLDEN_DIR, f"bwd_{name}.npz")) else "lw_"
        out.append((prefix, name))
    return out


IGRAD_CASES = _cases()   # (prefix of the case the inputs / weights come from, name)


def load_igrad(name):
    z = np.load(os.path.join(IGRAD_DIR, f"igrad_{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def rel_err(t, t64):
    """e(t) of the module docstring.  A tensor the reference holds at exactly zero (L = 0: the node features reach no logit; a dead
    network) has no scale: e is then max|t| itself, so the bound asks for zero within 2^-23."""
    t, t64 = np.asarray(t, dtype=np.float64), np.asarray(t64, dtype=np.float64)
    m = float(np.abs(t64).max()) if t64.size else 0.0
    d = float(np.abs(t - t64).max()) if t64.size else 0.0
    return d / m if m > 0 else d


def e_ref_max(agg):
    """Largest e_ref over the fixtures of one aggregator, per tensor: the yardstick for shapes that have no fp64 fixture."""
    best = {"dx": 0.0, "dea": 0.0}
    for prefix, name in IGRAD_CASES:
        params = load_bwd(name, prefix)[0]
        if params["node_agg_fn"] != agg:
            continue
        g = load_igrad(name)
        for k in best:
            best[k] = max(best[k], rel_err(g[k + "32"], g[k + "64"]))
    return best


def oracle_for(params, arch, sd, a):
    dropout = None
    if "dropout_p" in a:
        ps = [float(v) for v in a["dropout_p"]]
        dropout = dict(p_enc=ps[0], p_edge=ps[1], p_node=ps[2], p_cls=ps[3], seed=int(a["dropout_seed"]))
    return TorchTrainOracle(params, arch, sd, dropout=dropout)


def oracle_input_grads(orc, x, edge_index, edge_attr, labels, extra=()):
    """(loss, dx, d_edge_attr, [d extra...]) of the oracle: train.py:80-97's loss, torch.autograd.grad to the inputs.  An input no
    logit depends on (L = 0) gets zeros, as .grad would stay None on the reference."""
    x = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x)).requires_grad_()
    ea = torch.from_numpy(np.asarray(edge_attr)).requires_grad_()
    logits = orc.forward(x, edge_index, ea)
    crit = torch.nn.BCEWithLogitsLoss(reduction="mean")
    loss = sum(crit(t.view(-1), torch.as_tensor(labels).float()) for t in logits)
    wanted = [x, ea, *extra]
    got = torch.autograd.grad(loss, wanted, allow_unused=True)
    got = [g if g is not None else torch.zeros_like(w) for g, w in zip(got, wanted)]
    return (float(loss.detach()), *[g.numpy() for g in got])


def test_every_backward_fixture_has_input_gradients():
    have = {name for _, name in IGRAD_CASES}
    want = {os.path.basename(p)[:-4].split("_", 1)[1] for pat in ("bwd_*.npz", "lw_*.npz")
            for p in glob.glob(os.path.join(GOLDEN_DIR, pat))}
    assert have == want and len(have) >= 16


@pytest.mark.parametrize("prefix,name", IGRAD_CASES)
def test_oracle_input_gradients_match_reference(prefix, name):
    params, arch, sd, _, _, a = load_bwd(name, prefix)
    g = load_igrad(name)
    loss, dx, dea = oracle_input_grads(oracle_for(params, arch, sd, a), a["x"], a["edge_index"], a["edge_attr"], a["labels"])
    assert abs(loss - float(a["loss"])) <= 2e-6
    assert dx.shape == a["x"].shape and dea.shape == a["edge_attr"].shape
    for got, key in ((dx, "dx32"), (dea, "dea32")):   # the bound test_backward_oracle.py uses for the parameter gradients
        ref = g[key]
        assert np.abs(got - ref).max() <= 2e-6 * max(1.0, float(np.abs(ref).max())), key
    # ... and, these gradients being small, the relative distance as well (printed: the oracle is the GPU tests' 32-bit reference)
    print(f"{name}: e_oracle dx {rel_err(dx, g['dx64']):.3e} (e_ref {rel_err(g['dx32'], g['dx64']):.3e})  "
          f"dea {rel_err(dea, g['dea64']):.3e} (e_ref {rel_err(g['dea32'], g['dea64']):.3e})")
