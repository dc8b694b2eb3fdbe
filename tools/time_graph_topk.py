#!/usr/bin/env python3
"""Times the capped graph build (build_graph_batch(top_k=k): gnncca_plan_frames_ex + gnncca_build_edges_topk) and the eval forward of the
headline model (bench.graph_net_params: L = 4, resnet50 node encoder) on the graph it gives, for k in {4, 8, 16, dense}, on
  terrace   : 64 frames, 1229 detections on 4 cameras, about 21 930 edges dense, R = 2048   (a Terrace batch)
  dense1024 : one frame of 1024 detections on 4 cameras (deg = 768), 786 432 edges dense, R = 2048
`dense` is build_graph_batch without top_k: the comparison point, measured in the same run on the same machine.

    python tools/time_graph_topk.py            # every step in a child process of its own, each under its own time limit
    python tools/time_graph_topk.py --step terrace:8:ground

Prints one JSON line per step: E, microseconds per build (host planning + upload + launches, as a caller pays for them) and per model
forward (median of 5 rounds of 20, after 10 warm-ups; HIP events around each round).  A step that fails or runs out of time ends the
run: nothing else is started on the GPU after it.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_graph_grads import batch as terrace_batch, time_us  # noqa: E402

STEPS = [f"{shape}:{k}:{rank}" for shape in ("terrace", "dense1024") for k, rank in
         (("dense", "ground"), ("4", "ground"), ("8", "ground"), ("16", "ground"), ("8", "reid"))]
LIMIT_S = 240


def batch(shape):
    if shape == "terrace":
        b = terrace_batch("terrace")
        b["node"] = np.random.default_rng(4).standard_normal((b["n"], 2048)).astype(np.float32)
        return b
    rng = np.random.default_rng(3)
    n, r = 1024, 2048
    return dict(sizes=np.array([n], dtype=np.int64), id_cam=np.arange(n) * 4 // n, n=n, r=r, ids=rng.integers(0, 300, n),
                xw=rng.uniform(-30, 30, n), yw=rng.uniform(-30, 30, n), max_dist=np.array([85.0]),
                node=rng.standard_normal((n, 2048)).astype(np.float32), reid=(rng.standard_normal((n, r)) + 0.5).astype(np.float32))


def run_step(step):
    import torch

    import bench
    from gnn_cca_amd.graph_build import build_graph_batch
    shape, k, rank = step.split(":")
    b = batch(shape)
    kw = {} if k == "dense" else dict(top_k=int(k), rank_by=rank)
    node, reid = torch.from_numpy(b["node"]).cuda(), torch.from_numpy(b["reid"]).cuda()
    model = bench.build_model(bench.graph_net_params(), int(b["sizes"].max())).cuda().eval()

    def build():
        return build_graph_batch(b["xw"], b["yw"], b["ids"], b["id_cam"], b["sizes"], b["max_dist"], node, reid, **kw)

    g = build()
    with torch.no_grad():
        res = dict(step=step, n=b["n"], e=int(g.edge_index.shape[1]), build_us=round(time_us(build), 1),
                   forward_us=round(time_us(lambda: model(g)), 1))
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
