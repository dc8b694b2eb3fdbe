#!/usr/bin/env python3
"""Times what the input gradients (x.grad, edge_attr.grad in train mode: row N3) add to the backward of config_training.yaml's model, on

  terrace : the Terrace-shaped 64-frame batch (4 cameras x 5 detections per frame: 1280 nodes, 19 200 edges)
  node4096: the node side of one dense N = 4096 graph -- 4096 nodes joined by a ring of 4096 edges, so that the edge kernels are
            negligible and what is timed is the node encoder's backward, where d x lives

in four forms, each captured whole into a HIP graph of its own (device time: no host enqueue in the figures; a captured backward has to be
captured together with its forward, so the forward is timed on its own and subtracted):

  f. the training forward and the loss alone
  a. forward + backward to the parameters only (what the backward was before inputs could require grad); backward = a - f
  b. forward + backward to the parameters, x and edge_attr; what the input gradients add = b - a
  c. torch.mm(gz1_like [N, 128], W1 [128, 2048]): the yardstick for the d x product alone

The forms are timed in alternating windows (f a b c f a b c ...): the median window with min .. max over the windows of the same form.
`dx_MB` is what the d x kernel writes (N x D x 4 bytes) with the time that takes at HBM peak, `dx_us_at_f32_matrix_peak` the time of its
2 N F1 D flops on the fp32 matrix pipe.

    python tools/time_input_grads.py [--iters 200] [--windows 7]
"""
import argparse
import copy
import faulthandler
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0        # MI355X
F32_MATRIX_PEAK_TF = 157.3


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def terrace_batch(frames=64, cams=4, per=5):
    n_g = cams * per
    cam = np.repeat(np.arange(cams), per)
    i, j = np.meshgrid(np.arange(n_g), np.arange(n_g), indexing="ij")
    keep = cam[i] != cam[j]
    ei = np.concatenate([np.stack([i[keep], j[keep]]) + f * n_g for f in range(frames)], axis=1)
    return frames * n_g, ei.astype(np.int64), n_g


def ring(n):
    i = np.arange(n)
    return n, np.stack([i, (i + 1) % n]).astype(np.int64), n


def captured(fn, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    faulthandler.enable()
    import bench

    class D:
        pass

    crit = torch.nn.BCEWithLogitsLoss()
    params = bench.graph_net_params(cls_bn=False)
    res = {"iters_per_window": args.iters, "windows": args.windows}
    for name, (n, ei, n_g) in (("terrace", terrace_batch()), ("node4096", ring(4096))):
        e = ei.shape[1]
        rng = np.random.default_rng(0)
        x = rng.standard_normal((n, 2048)).astype(np.float32)
        x /= np.linalg.norm(x, axis=0, keepdims=True)
        model = bench.build_model(copy.deepcopy(params), n_g).cuda().train()
        xs, eas = torch.from_numpy(x).cuda(), torch.from_numpy(rng.random((e, 4)).astype(np.float32)).cuda()
        plain, req = D(), D()
        plain.edge_index = req.edge_index = torch.from_numpy(ei).cuda()
        plain.x, plain.edge_attr = xs, eas
        req.x, req.edge_attr = xs.clone().requires_grad_(), eas.clone().requires_grad_()
        labels = torch.from_numpy((rng.random(e) < 0.2).astype(np.float32)).cuda()
        loss_of = lambda data: sum(crit(t.view(-1), labels) for t in model(data)["classified_edges"])  # noqa: E731
        ps = [p for p in model.parameters() if p.requires_grad]
        w1 = model.encoder.node_mlp.fc_layers[0].weight.detach()
        f1, dim = w1.shape
        gz1 = torch.randn(n, f1, device="cuda")

        def forward_only():
            with torch.no_grad():
                return loss_of(plain)

        forms = {
            "f_forward": forward_only,
            "a_params_only": lambda: torch.autograd.grad(loss_of(plain), ps),
            "b_params_and_inputs": lambda: torch.autograd.grad(loss_of(req), ps + [req.x, req.edge_attr]),
            "c_torch_mm_dx": lambda: torch.mm(gz1, w1),
        }
        graphs = {}
        for k, fn in forms.items():
            print(f"{name}: capturing {k}", file=sys.stderr, flush=True)
            graphs[k] = captured(fn)
        times = {k: [] for k in forms}
        for _ in range(args.windows):
            for k in forms:
                times[k].append(window(graphs[k].replay, args.iters))
        r = {"nodes": n, "edges": e, "node_in": dim, "F1": f1}
        for k, ts in times.items():
            r[k] = {"us": round(statistics.median(ts), 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)]}
        r["backward_params_only_us"] = round(r["a_params_only"]["us"] - r["f_forward"]["us"], 2)
        r["backward_with_inputs_us"] = round(r["b_params_and_inputs"]["us"] - r["f_forward"]["us"], 2)
        r["b_minus_a_us"] = round(r["b_params_and_inputs"]["us"] - r["a_params_only"]["us"], 2)
        r["dx_MB"] = round(4 * n * dim / 1e6, 2)
        r["dx_us_at_hbm_peak"] = round(4 * n * dim / (HBM_PEAK_TBPS * 1e12) * 1e6, 2)
        r["dx_us_at_f32_matrix_peak"] = round(2.0 * n * f1 * dim / (F32_MATRIX_PEAK_TF * 1e12) * 1e6, 2)
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
