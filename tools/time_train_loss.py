#!/usr/bin/env python3
"""Times gnn_cca_amd.loss on the GPU against what it replaces:

  1. the kernel pair (forward: partials + finish, backward: one elementwise launch) on E edges x S steps, with the bytes each moves;
  2. a torch restatement of the reference's per-iteration loss code (compute_loss_acc, train.py:51-208, the mean probabilities of
     train.py:460-469 and the six meter updates of train.py:472-479, with their .cpu() / .item() synchronisations) on the same tensors;
  3. one GraphedTrainStep iteration (the bwd_terrace32 setup) with EdgeLoss + TrainMeters against the plain BCE lambda.

    python tools/time_train_loss.py [--edges 2097152] [--steps 3] [--iters 200]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_time(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us per call


def reference_style(outputs, labels, crit, crit_nr, meters):
    """The torch operations of compute_loss_acc + train.py:460-479 for the 'train' mode, restated (host synchronisations included)."""
    loss = loss1 = loss0 = 0
    probs = []
    for t in outputs:
        preds = t.view(-1)
        lps = crit_nr(preds, labels)
        loss = loss + crit(preds, labels)
        loss1 = loss1 + torch.mean(lps[labels == 1])
        loss0 = loss0 + torch.mean(lps[labels == 0])
        with torch.no_grad():
            probs.append(torch.sigmoid(preds))
    with torch.no_grad():
        pred = (torch.sigmoid(outputs[-1].view(-1)) >= 0.5) * 1
        lab = labels.cpu().numpy()
        pr = pred.cpu().numpy()
        i1, i0 = np.where(lab == 1), np.where(lab == 0)
        h1, h0, h = np.sum(pr[i1] == lab[i1]), np.sum(pr[i0] == lab[i0]), np.sum(pr == lab)
        p1 = 0 if h1 == 0 else h1 / len(i1[0]) * 100.0
        p0 = 0 if h0 == 0 else h0 / len(i0[0]) * 100.0
        p = 0 if h == 0 else h / len(lab) * 100.0
    mp = []
    for s in range(len(probs)):
        mp.append(torch.mean(probs[s][labels == 0]) if bool((labels == 0).any()) else torch.tensor(0.5, device=labels.device))
        mp.append(torch.mean(probs[s][labels == 1]) if bool((labels == 1).any()) else torch.tensor(0.5, device=labels.device))
    for v, m in zip((loss.item(), loss1.item(), loss0.item(), p1, p0, p), meters):
        m.append(v)
    return loss, mp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=1 << 21)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.frames import _raw_stream
    from gnn_cca_amd.loss import CRITERIA, EdgeLoss, TrainMeters, record_len

    dev = torch.device("cuda:0")
    s, e = args.steps, args.edges
    g = torch.Generator(device=dev).manual_seed(0)
    x = 3.0 * torch.randn(s, e, 1, device=dev, generator=g)
    y = (torch.rand(e, device=dev, generator=g) < 0.15).float()
    lib = nat.lib()
    res = {"edges": e, "steps": s}
    loss = torch.empty((), device=dev)
    rec = torch.empty(record_len(s), dtype=torch.float64, device=dev)
    ws_b = lib.gnncca_edge_loss_workspace_bytes(s, e)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
    grad = torch.empty_like(x)
    one = torch.ones((), device=dev)
    st = _raw_stream(dev)
    for name, crit in CRITERIA.items():
        pw = 4.5 if name == "BCE_weighted" else 1.0

        def fwd():
            lib.gnncca_edge_loss_forward(x.data_ptr(), y.data_ptr(), s, e, crit, 0, pw, 5.0, 0.9, loss.data_ptr(), rec.data_ptr(), None, 0,
                                         None, ws.data_ptr(), ws_b, st)

        def bwd():
            lib.gnncca_edge_loss_backward(x.data_ptr(), y.data_ptr(), s, e, crit, 0, pw, one.data_ptr(), rec.data_ptr(), grad.data_ptr(), st)

        tf, tb = event_time(fwd, args.iters), event_time(bwd, args.iters)
        res[f"kernel_fwd_us_{name}"], res[f"kernel_bwd_us_{name}"] = round(tf, 2), round(tb, 2)
    fwd_bytes, bwd_bytes = 4 * e * (s + 1), 4 * e * (2 * s + 1)
    res["fwd_MB"], res["bwd_MB"] = round(fwd_bytes / 1e6, 1), round(bwd_bytes / 1e6, 1)
    res["fwd_GBps_BCE"] = round(fwd_bytes / res["kernel_fwd_us_BCE"] / 1e3, 1)
    res["bwd_GBps_BCE"] = round(bwd_bytes / res["kernel_bwd_us_BCE"] / 1e3, 1)

    # EdgeLoss forward + backward through autograd (Python included) vs the restated reference code, wall clock per iteration
    xs = x.clone().requires_grad_(True)
    fn = EdgeLoss("BCE")
    outs = list(xs.unbind(0))

    def edge_loss_iter():
        xs.grad = None
        fn({"classified_edges": outs}, y).backward()

    crit, crit_nr = torch.nn.BCEWithLogitsLoss(), torch.nn.BCEWithLogitsLoss(reduction="none")
    meters = [[] for _ in range(6)]

    def reference_iter():
        xs.grad = None
        l, _ = reference_style(outs, y, crit, crit_nr, meters)
        l.backward()

    for name, f in (("edge_loss_iter_ms", edge_loss_iter), ("reference_iter_ms", reference_iter)):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = max(5, args.iters // 20)
        for _ in range(n):
            f()
        torch.cuda.synchronize()
        res[name] = round((time.perf_counter() - t0) * 1e3 / n, 3)

    # whole training iteration from one HIP graph: EdgeLoss + meters vs the BCE lambda
    from gnn_cca_amd import MOTMPNet
    from gnn_cca_amd.training import GraphedTrainStep
    from test_backward_oracle import load_bwd
    params, arch, sd, _, _, a = load_bwd("terrace32")

    class D:
        pass

    for name in ("bce_lambda", "edge_loss_meters"):
        m = MOTMPNet(copy.deepcopy(params), None, arch)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m = m.to(dev).train()
        d = D()
        d.x, d.edge_index, d.edge_attr = (torch.from_numpy(a[k]).to(dev) for k in ("x", "edge_index", "edge_attr"))
        lab = torch.from_numpy(np.asarray(a["labels"])).to(dev).float()
        if name == "bce_lambda":
            c = torch.nn.BCEWithLogitsLoss()
            lf = lambda out, lb: sum(c(t.view(-1), lb) for t in out["classified_edges"])  # noqa: E731
        else:
            tm = TrainMeters(capacity=1 << 16, n_steps=int(a["n_logits"]), device=dev)
            lf = EdgeLoss("BCE", meters=tm)
        step = GraphedTrainStep(m, torch.optim.SGD(m.parameters(), lr=1e-3), lf, warmup=2)
        for _ in range(3):
            step(d, lab)
        res[f"graphed_iter_us_{name}"] = round(event_time(lambda: step(d, lab), args.iters), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
