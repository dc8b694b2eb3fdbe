#!/usr/bin/env python3
"""Golden INPUT gradients for SURVEY.md 8f row N3 (d loss / d x, d loss / d edge_attr of a train-mode forward), produced by the
REFERENCE's own MOTMPNet under torch autograd.  Build container only:    python tests/golden/make_golden_input_grads.py

For every existing bwd_<case>.npz (make_golden_backward.py) and lw_<case>.npz (make_golden_layerwise.py, injected Dropout masks) the
case's inputs, labels and weights are reloaded into the reference's module in train mode, the same loss is formed (sum over the
classified steps of BCEWithLogitsLoss(reduction='mean')), and input_grads/igrad_<case>.npz receives (a directory of their own: every
*.npz directly under tests/golden/ without a known prefix is taken for a forward case by conftest.golden_cases)
    dx32, dea32 : the reference in fp32 (the run the parameter gradients of the case came from; they are re-checked here)
    dx64, dea64 : the same module after .double() on double inputs -- the yardstick of the relative accuracy criterion
                  e(t) = max|t - t64| / max|t64|.
Only gradients are stored; neither the existing fixtures nor the oracle change.
"""
import copy
import glob
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_backward import _Data, _install_torch_scatter_standin  # noqa: E402
from make_golden_layerwise import inject  # noqa: E402


def input_grads(MOTMPNet, z, double):
    meta = json.loads(str(z["params_json"]))
    model = MOTMPNet(copy.deepcopy(meta["model_params"]), None, meta["arch"])
    model.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")})
    if "dropout_seed" in z.files:
        inject(model, int(z["dropout_seed"]))
    model.train()
    x, ea = torch.from_numpy(z["x"]), torch.from_numpy(z["edge_attr"])
    labels = torch.from_numpy(z["labels"])
    if double:
        model.double()
        x, ea, labels = x.double(), ea.double(), labels.double()
    x.requires_grad_(), ea.requires_grad_()
    data = _Data()
    data.x, data.edge_index, data.edge_attr = x, torch.from_numpy(z["edge_index"]), ea
    out = model(data)["classified_edges"]
    crit = torch.nn.BCEWithLogitsLoss(reduction="mean")
    loss = 0
    for t in out:
        loss = loss + crit(t.view(-1), labels)
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    dx = x.grad if x.grad is not None else torch.zeros_like(x)          # L = 0: the node features reach no logit
    dea = ea.grad if ea.grad is not None else torch.zeros_like(ea)
    return loss.item(), dx.numpy(), dea.numpy(), grads


def rel(t, t64):
    m = float(np.abs(t64).max())
    return float(np.abs(t.astype(np.float64) - t64).max()) / m if m > 0 else float(np.abs(t).max())


def main():
    torch.set_num_threads(8)   # the thread count the bwd_* / lw_* vectors were recorded with
    _install_torch_scatter_standin()
    sys.path.insert(0, "/root/reference")
    from models.mpn import MOTMPNet

    for path in sorted(glob.glob(os.path.join(HERE, "bwd_*.npz")) + glob.glob(os.path.join(HERE, "lw_*.npz"))):
        z = np.load(path, allow_pickle=False)
        case = os.path.basename(path)[:-4].split("_", 1)[1]
        loss32, dx32, dea32, g32 = input_grads(MOTMPNet, z, False)
        loss64, dx64, dea64, _ = input_grads(MOTMPNet, z, True)
        # the fp32 run must be the run the case recorded: same loss, same parameter gradients
        assert abs(loss32 - float(z["loss"])) <= 2e-6, (case, loss32, float(z["loss"]))
        for k, g in g32.items():
            ref = z["grad::" + k]
            assert np.abs(g.numpy() - ref).max() <= 2e-6 * max(1.0, float(np.abs(ref).max())), (case, k)
        os.makedirs(os.path.join(HERE, "input_grads"), exist_ok=True)
        np.savez(os.path.join(HERE, "input_grads", f"igrad_{case}.npz"), dx32=dx32, dea32=dea32, dx64=dx64, dea64=dea64)
        print(f"igrad_{case:26s} max|dx|={np.abs(dx64).max():.3e} e_ref(dx)={rel(dx32, dx64):.3e}  "
              f"max|dea|={np.abs(dea64).max():.3e} e_ref(dea)={rel(dea32, dea64):.3e}  loss32-loss64={loss32 - loss64:+.2e}")


if __name__ == "__main__":
    main()
