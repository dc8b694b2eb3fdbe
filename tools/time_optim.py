#!/usr/bin/env python3
"""Times the optimizer step of a graph-replayed training iteration (gnn_cca_amd.training.GraphedTrainStep) in four forms on one
Terrace-shaped batch (64 frames, 4 cameras x 5 detections, config_training.yaml's model):

  a. torch.optim.SGD(momentum=0.9, weight_decay=1e-4)      b. gnn_cca_amd.optim.FusedSGD, the same values
  c. torch.optim.Adam(capturable=True)                     d. gnn_cca_amd.optim.FusedAdam

The four are built in ONE process, each warmed up, and timed in alternating windows (a b c d a b c d ...): `iter_us` is the median
window (device events around `iters` replays, host enqueue included as in training), `spread_us` the min .. max over the windows of the
same form -- the noise any difference between two forms has to exceed.  `update_us` is `optimizer.step()` alone, captured into its own
graph and replayed back to back; `launches` counts the kernels of one replayed iteration (torch.profiler); `update_MB` is what the
update has to move (parameters, gradients and state read, parameters and state written), with the time that takes at HBM peak.

    python tools/time_optim.py [--frames 64] [--iters 200] [--windows 7]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0   # MI355X


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    import bench
    from gnn_cca_amd.optim import FusedAdam, FusedSGD
    from gnn_cca_amd.training import GraphedTrainStep

    cams, per = 4, 5
    n_g = cams * per
    rows, cols = [], []
    for f in range(args.frames):
        idx = np.arange(f * n_g, (f + 1) * n_g)
        cam = np.repeat(np.arange(cams), per)
        i, j = np.meshgrid(idx, idx, indexing="ij")
        m = cam[i - f * n_g] != cam[j - f * n_g]
        rows.append(i[m])
        cols.append(j[m])
    ei = np.stack([np.concatenate(rows), np.concatenate(cols)])
    n, e = args.frames * n_g, ei.shape[1]
    rng = np.random.default_rng(0)
    x = rng.standard_normal((n, 2048)).astype(np.float32)
    x /= np.linalg.norm(x, axis=0, keepdims=True)

    class D:
        pass

    d = D()
    d.x, d.edge_index = torch.from_numpy(x).cuda(), torch.from_numpy(ei).cuda()
    d.edge_attr = torch.from_numpy(rng.random((e, 4)).astype(np.float32)).cuda()
    labels = torch.from_numpy((rng.random(e) < 0.2).astype(np.float32)).cuda()
    crit = torch.nn.BCEWithLogitsLoss()
    loss_fn = lambda out, lab: sum(crit(t.view(-1), lab) for t in out["classified_edges"])  # noqa: E731
    params = bench.graph_net_params(cls_bn=False)
    forms = {
        "a_torch_sgd": lambda ps: torch.optim.SGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4),
        "b_fused_sgd": lambda ps: FusedSGD(ps, lr=1e-3, momentum=0.9, weight_decay=1e-4),
        "c_torch_adam_capturable": lambda ps: torch.optim.Adam(ps, lr=1e-4, capturable=True),
        "d_fused_adam": lambda ps: FusedAdam(ps, lr=1e-4),
    }
    steps, res = {}, {"frames": args.frames, "nodes": n, "edges": e, "iters_per_window": args.iters, "windows": args.windows}
    for name, make in forms.items():
        model = bench.build_model(copy.deepcopy(params), n_g).cuda().train()
        opt = make(model.parameters())
        step = GraphedTrainStep(model, opt, loss_fn, warmup=3)
        for _ in range(4 + 20):     # three eager, the capture, then replays
            step(d, labels)
        torch.cuda.synchronize()
        assert len(step._graphs) == 1
        steps[name] = (model, opt, step)
    n_par = sum(p.numel() for p in steps["a_torch_sgd"][0].parameters())
    res["parameters"], res["tensors"] = n_par, len(list(steps["a_torch_sgd"][0].parameters()))

    times = {name: [] for name in forms}
    for _ in range(args.windows):
        for name in forms:
            times[name].append(window(lambda: steps[name][2](d, labels), args.iters))
    for name, ts in times.items():
        res[name] = {"iter_us": round(statistics.median(ts), 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)]}

    # the update alone: optimizer.step() on the gradients of the last iteration, in a graph of its own, replayed back to back
    for name, (model, opt, step) in steps.items():
        for p in model.parameters():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        if hasattr(opt, "sync_hyperparameters"):
            opt.sync_hyperparameters()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
        for _ in range(20):
            g.replay()
        ts = [window(g.replay, args.iters) for _ in range(3)]
        res[name]["update_us"] = round(statistics.median(ts), 2)
        words = 5 if "sgd" in name else 7       # p, g, state read; p, state written
        res[name]["update_MB"] = round(4 * words * n_par / 1e6, 2)
        res[name]["update_us_at_hbm_peak"] = round(4 * words * n_par / (HBM_PEAK_TBPS * 1e12) * 1e6, 2)
        steps[name] = (model, opt, step, g)

    # kernels per replayed iteration / per replayed update
    try:
        from torch.profiler import ProfilerActivity, profile
        for name, (model, opt, step, g) in steps.items():
            for key, fn in (("launches", lambda: step(d, labels)), ("update_launches", g.replay)):
                torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                kernels = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
                           and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower()]
                res[name][key] = len(kernels)
    except Exception as exc:   # the profiler is optional: the times above stand without it
        res["launch_count_error"] = repr(exc)[:200]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
