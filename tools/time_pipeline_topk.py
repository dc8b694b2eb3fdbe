#!/usr/bin/env python3
"""Times a batch of frames from detections to identity clusters on a capped graph, one native call against the step-by-step path, with the
headline model (bench.graph_net_params: L = 4, resnet50 node encoder), for k in {dense, 4, 8, 16} (ranking by ground distance), on
  terrace   : 64 frames, 1229 detections on 4 cameras, about 21 930 edges dense, R = 2048   (a Terrace batch)
  dense1024 : one frame of 1024 detections on 4 cameras (deg = 768), 786 432 edges dense, R = 2048
(the batches of tools/time_graph_topk.py).  Per step, in one process:
  one_call  : FramePipeline(model, top_k=k)(...)                       gnncca_plan_frames_ex + gnncca_frames_forward_topk
  stepwise  : build_graph_batch(top_k=k) -> model -> threshold -> prune_and_cluster, measured TWICE (before and after one_call); the
              difference of the two repetitions is the run's own spread, the margin a gain has to be read against
`dense` is top_k=None on both sides (gnncca_frames_forward against the dense step-by-step path).

    python tools/time_pipeline_topk.py            # every step in a child process of its own, each under its own time limit
    python tools/time_pipeline_topk.py --step terrace:8

Prints one JSON line per step: E and milliseconds per batch on the host clock, two ways, each after 10 warm-ups:
  one_call_ms / stepwise_ms / spread_ms                   : ONE batch at a time, the device synchronised before the batch is issued and after
                                                            it; the median of 30 batches.  The GPU chain's own length is inside every
                                                            sample, so host savings show only where the host is the longer of the two.
  stream_one_call_ms / stream_stepwise_ms / stream_spread_ms : 20 batches issued back to back between two synchronisations (how bench.py's
                                                            terrace_pipeline leg runs, the mode the one-call form is built for); the median
                                                            of 7 such rounds, per batch.
A step that fails or runs out of time ends the run: nothing else is started on the GPU after it.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_graph_topk import batch  # noqa: E402

STEPS = [f"{shape}:{k}" for shape in ("terrace", "dense1024") for k in ("dense", "4", "8", "16")]
LIMIT_S = 240
BATCHES, WARMUP = 30, 10
ROUNDS, PER_ROUND = 7, 20


def ms_per_batch(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(BATCHES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def ms_per_batch_stream(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(PER_ROUND):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / PER_ROUND)
    return float(np.median(out))


def run_step(step):
    import torch

    import bench
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.postprocess import prune_and_cluster, threshold
    shape, k = step.split(":")
    b = batch(shape)
    kw = {} if k == "dense" else dict(top_k=int(k), rank_by="ground")
    node, reid = torch.from_numpy(b["node"]).cuda(), torch.from_numpy(b["reid"]).cuda()
    model = bench.build_model(bench.graph_net_params(), int(b["sizes"].max())).cuda().eval()
    args = (b["xw"], b["yw"], b["ids"], b["id_cam"], b["sizes"], b["max_dist"], node, reid)

    def stepwise():
        g = build_graph_batch(*args, **kw)
        with torch.no_grad():
            out = model(g)
        probs, preds = threshold(out["classified_edges"][-1])
        return g, out, prune_and_cluster(g.edge_index, preds, g.x.shape[0], g.node_ptr_dev, g.edge_ptr_dev)

    # random weights put every logit on one side of 0: centre them so that pruning and clustering have work to do
    with torch.no_grad():
        g, out, _ = stepwise()
        sd = model.state_dict()
        last_bias = [q for q in sd if q.startswith("classifier.") and q.endswith(".bias")][-1]
        sd[last_bias] -= out["classified_edges"][-1].median()
        model.load_state_dict(sd)
    pipe = FramePipeline(model, **kw)
    r, (_, _, post) = pipe(*args), stepwise()
    torch.cuda.synchronize()
    if r._d2h is None or not (torch.equal(r.pruned, post["pruned"]) and torch.equal(r.labels, post["labels"])):
        raise SystemExit(f"{step}: the one-call path was not taken or disagrees with the step-by-step path")
    first, s_first = ms_per_batch(stepwise), ms_per_batch_stream(stepwise)
    one, s_one = ms_per_batch(lambda: pipe(*args)), ms_per_batch_stream(lambda: pipe(*args))
    second, s_second = ms_per_batch(stepwise), ms_per_batch_stream(stepwise)
    res = dict(step=step, n=b["n"], e=int(g.edge_index.shape[1]), one_call_ms=round(one, 4), stepwise_ms=[round(first, 4), round(second, 4)],
               spread_ms=round(abs(first - second), 4), one_call_faster=bool(one < min(first, second)),
               stream_one_call_ms=round(s_one, 4), stream_stepwise_ms=[round(s_first, 4), round(s_second, 4)],
               stream_spread_ms=round(abs(s_first - s_second), 4), stream_one_call_faster=bool(s_one < min(s_first, s_second)))
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
