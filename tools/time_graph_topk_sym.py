#!/usr/bin/env python3
"""Times the symmetric capped graph build (build_graph_batch(top_k=k, symmetric='union' | 'mutual'): gnncca_plan_frames_ex +
gnncca_build_edges_topk_sym_count + one read-back of the edge count + gnncca_build_edges_topk_sym_emit) and the eval forward of the
headline model (bench.graph_net_params: L = 4, resnet50 node encoder) on the graph it gives, for k in {4, 8, 16} ranked by ground
distance, on the two batches of tools/time_graph_topk.py:
  terrace   : 64 frames, 1229 detections on 4 cameras, about 21 930 edges dense, R = 2048   (a Terrace batch)
  dense1024 : one frame of 1024 detections on 4 cameras (deg = 768), 786 432 edges dense, R = 2048
`directed` is build_graph_batch(top_k=k) without `symmetric`: the comparison point, measured in the same process on the same machine.

    python tools/time_graph_topk_sym.py            # every step in a child process of its own, each under its own time limit
    python tools/time_graph_topk_sym.py --step terrace:8

Prints one JSON line per step and mode: E, microseconds per build (host planning + upload + launches + for the symmetric modes the wait
for the edge count, as a caller pays for them) and per model forward (median of 5 rounds of 20, after 10 warm-ups; HIP events around each
round).  A step that fails or runs out of time ends the run: nothing else is started on the GPU after it.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_graph_grads import time_us  # noqa: E402
from time_graph_topk import batch  # noqa: E402

STEPS = [f"{shape}:{k}" for shape in ("terrace", "dense1024") for k in (4, 8, 16)]
MODES = (None, "union", "mutual")
LIMIT_S = 240


def run_step(step):
    import torch

    import bench
    from gnn_cca_amd.graph_build import build_graph_batch
    shape, k = step.split(":")
    b = batch(shape)
    node, reid = torch.from_numpy(b["node"]).cuda(), torch.from_numpy(b["reid"]).cuda()
    model = bench.build_model(bench.graph_net_params(), int(b["sizes"].max())).cuda().eval()
    for mode in MODES:
        def build():
            return build_graph_batch(b["xw"], b["yw"], b["ids"], b["id_cam"], b["sizes"], b["max_dist"], node, reid, top_k=int(k),
                                     rank_by="ground", symmetric=mode)

        g = build()
        with torch.no_grad():
            res = dict(step=step, mode=mode or "directed", n=b["n"], e=int(g.edge_index.shape[1]), build_us=round(time_us(build), 1),
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
