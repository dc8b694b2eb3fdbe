#!/usr/bin/env python3
"""Times the backward of the graph build (gnncca_build_edges_backward + gnncca_normalize_columns_backward behind build_graph_batch)
against torch autograd of the reference's own op sequence on the same GPU (F.normalize, gathers, F.pairwise_distance,
F.cosine_similarity -- inference.py:189-190, 222-226), on
  terrace : 64 frames, 1229 detections on 4 cameras, about 21 930 edges, R = 2048   (a Terrace batch)
  f512x32 : 512 frames x 32 detections (4 cameras x 8), 393 216 edges, R = 256

    python tools/time_graph_grads.py            # every step in a child process of its own, each under its own time limit
    python tools/time_graph_grads.py --step terrace:ours

Prints one JSON line per step: microseconds per backward and per forward + backward (median of 5 rounds of 20, after 10 warm-ups; HIP
events around each round).  A step that fails or runs out of time ends the run: nothing else is started on the GPU after it.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ["terrace:ours", "terrace:torch", "f512x32:ours", "f512x32:torch"]
LIMIT_S = 240


def batch(shape):
    rng = np.random.default_rng(3)
    if shape == "terrace":
        sizes = np.clip(np.rint(rng.normal(19.2, 9.0, 64)), 4, 48).astype(np.int64)
        while sizes.sum() != 1229:                       # adjust to exactly 1229 detections
            k = rng.integers(0, 64)
            sizes[k] += 1 if sizes.sum() < 1229 else (-1 if sizes[k] > 4 else 0)
        r = 2048
    else:
        sizes, r = np.full(512, 32, dtype=np.int64), 256
    id_cam = np.concatenate([np.arange(s) * 4 // s for s in sizes])    # four cameras, camera-major, as even as the size allows
    n = int(sizes.sum())
    return dict(sizes=sizes, id_cam=id_cam, n=n, r=r, ids=rng.integers(0, 12, n), xw=rng.uniform(-10, 10, n), yw=rng.uniform(-10, 10, n),
                max_dist=rng.uniform(10, 90, len(sizes)), node=rng.standard_normal((n, 256)).astype(np.float32),
                reid=(rng.standard_normal((n, r)) + 0.5).astype(np.float32))


def time_us(fn, rounds=5, iters=20, warmup=10):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) * 1000.0 / iters)
    return float(np.median(out))


def run_step(step):
    import torch
    import torch.nn.functional as F
    from gnn_cca_amd.graph_build import build_graph_batch
    shape, which = step.split(":")
    b = batch(shape)
    node = torch.from_numpy(b["node"]).cuda().requires_grad_()
    reid = torch.from_numpy(b["reid"]).cuda().requires_grad_()
    with torch.no_grad():
        ref = build_graph_batch(b["xw"], b["yw"], b["ids"], b["id_cam"], b["sizes"], b["max_dist"], node, reid)
    ei, dist = ref.edge_index, ref.edge_attr[:, :2].clone()
    e = int(ei.shape[1])
    gen = torch.Generator(device="cuda").manual_seed(1)
    gx = torch.randn(node.shape, device="cuda", generator=gen)
    gea = torch.randn((e, 4), device="cuda", generator=gen)

    if which == "ours":
        def forward():
            g = build_graph_batch(b["xw"], b["yw"], b["ids"], b["id_cam"], b["sizes"], b["max_dist"], node, reid)
            return g.x, g.edge_attr
    else:
        def forward():
            rn, x = F.normalize(reid, p=2, dim=0), F.normalize(node, p=2, dim=0)
            a, c = rn[ei[0]], rn[ei[1]]
            emb = F.pairwise_distance(a, c).view(-1, 1)
            cos = F.cosine_similarity(a, c).view(-1, 1)
            return x, torch.cat((dist, emb, cos), dim=1)

    def both():
        node.grad = reid.grad = None
        x, ea = forward()
        torch.autograd.backward([x, ea], [gx, gea])

    x, ea = forward()

    def backward():
        node.grad = reid.grad = None
        torch.autograd.backward([x, ea], [gx, gea], retain_graph=True)

    res = dict(step=step, n=b["n"], e=e, r=b["r"], backward_us=round(time_us(backward), 1), forward_backward_us=round(time_us(both), 1))
    print(json.dumps(res), flush=True)


def main():
    if "--step" in sys.argv:
        run_step(sys.argv[sys.argv.index("--step") + 1])
        return 0
    for step in STEPS:   # a fresh process per step, each under its own limit; the first failure ends the run
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {LIMIT_S} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"{step}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
