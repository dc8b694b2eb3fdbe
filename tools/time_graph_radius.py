#!/usr/bin/env python3
"""Times the radius-gated graph (build_graph_batch / FramePipeline radius=r) against the dense one on batches of 64 frames whose cameras,
identities and ground-plane positions are the real-geometry fixture's (tests/golden/terrace_geometry.npz: the EPFL-Terrace annotations
projected onto the ground plane); the embeddings are synthetic (node 2048, reid 2048 wide), as in the other tools.  Two batches:
  consecutive : 64 consecutive frames from the middle of the sequence (what a per-batch loop over the sequence sees)
  largest     : the 64 frames with the most detections (up to 34 per frame: the host plan's pair loop at its longest)
Model: the headline one (bench.graph_net_params: L = 4, resnet50 node encoder).  Per batch, in one process of its own:

  plan     host time of gnncca_plan_frames_radius(r) and of gnncca_plan_frames into a host buffer: the median of 300 calls, alternating
  build    the build launch alone -- gnncca_build_edges_radius(r) and gnncca_build_edges on the uploaded images, outputs preallocated --
           between two device events around 50 launches, the median of 9 such rounds, alternating
  pipeline the whole one-call pipeline per batch, FramePipeline(model, radius=r) against the dense FramePipeline(model) call on the same
           batch: host clock, (a) one batch between two device synchronisations, median of 30; (b) 20 batches back to back between two
           synchronisations, median of 7 rounds, per batch.  The dense call is measured before AND after the gated one: the difference
           of its two figures is the run's own spread, the margin a ratio has to be read against.
at radii 60, 80, 100 and inf (ground units).  Per radius it also prints E, the kept fraction and the recall of same-identity edges,
the latter two from ranking.PooledCurve(keep='le') on the dense batch's ground distance (edge_attr[:, 0], thresholds r / max_dist).

    python tools/time_graph_radius.py                  # each batch in a child process, under its own time limit
    python tools/time_graph_radius.py --step largest

Prints one JSON line per (batch, radius).  A step that fails or runs out of time ends the run: nothing else is started on the GPU after it.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("consecutive", "largest")
RADII = (60.0, 80.0, 100.0, math.inf)
LIMIT_S = 300
MAX_DIST = 100.0
BATCHES, WARMUP = 30, 10
ROUNDS, PER_ROUND = 7, 20


def batch(which, seed=0):
    z = np.load(os.path.join(ROOT, "tests", "golden", "terrace_geometry.npz"))
    ptr = z["node_ptr"].astype(np.int64)
    sizes = np.diff(ptr)
    frames = np.arange(len(sizes) // 2 - 32, len(sizes) // 2 + 32) if which == "consecutive" else np.sort(np.argsort(-sizes, kind="stable")[:64])
    idx = np.concatenate([np.arange(ptr[q], ptr[q + 1]) for q in frames])
    rng = np.random.default_rng(seed)
    n = len(idx)
    return dict(sizes=sizes[frames].copy(), n=n, id_cam=z["cam"][idx].astype(np.int64), ids=z["person"][idx].astype(np.int64),
                xw=z["xw"][idx].astype(np.float64), yw=z["yw"][idx].astype(np.float64), max_dist=np.full(64, MAX_DIST),
                node=rng.standard_normal((n, 2048)).astype(np.float32), reid=rng.standard_normal((n, 2048)).astype(np.float32))


def plan_us(b, radius):
    """(gated, dense) host microseconds per plan call."""
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    n, g = b["n"], len(b["sizes"])
    nbytes = lib.gnncca_plan_frames_bytes(n, g)
    image = np.empty(nbytes, np.uint8)
    args = (b["xw"].ctypes.data, b["yw"].ctypes.data, b["ids"].ctypes.data, b["id_cam"].ctypes.data, n, b["sizes"].ctypes.data, b["max_dist"].ctypes.data, g)
    gated, dense = [], []
    for k in range(320):
        t0 = time.perf_counter()
        lib.gnncca_plan_frames_radius(*args, radius, 0, image.ctypes.data, nbytes)
        t1 = time.perf_counter()
        lib.gnncca_plan_frames(*args, image.ctypes.data, nbytes)
        t2 = time.perf_counter()
        if k >= 20:
            gated.append((t1 - t0) * 1e6), dense.append((t2 - t1) * 1e6)
    return float(np.median(gated)), float(np.median(dense))


def build_us(gated_batch, dense_batch, radius):
    """(gated, dense) device microseconds per build launch."""
    import ctypes as C

    import torch

    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.frames import _raw_stream
    lib = nat.lib()
    dev = dense_batch.x.device
    reid = dense_batch.reid_embeds
    n, r_dim = reid.shape

    def launcher(b, gated):
        staged, layout = b._frames
        fr = layout.frames(staged.data_ptr())
        e = int(b.edge_index.shape[1])
        ei, ea, el = torch.empty_like(b.edge_index), torch.empty_like(b.edge_attr), torch.empty_like(b.edge_labels)

        def go():
            if gated:
                st = lib.gnncca_build_edges_radius(C.byref(fr), reid.data_ptr(), r_dim, n, e, 0, radius, 0, ei.data_ptr(), ea.data_ptr(), el.data_ptr(), _raw_stream(dev))
            else:
                st = lib.gnncca_build_edges(C.byref(fr), reid.data_ptr(), r_dim, n, e, 0, ei.data_ptr(), ea.data_ptr(), el.data_ptr(), _raw_stream(dev))
            if st:
                nat.check(st, "gnncca_build_edges")
        go()
        torch.cuda.synchronize()
        if not (torch.equal(ei, b.edge_index) and torch.equal(el, b.edge_labels)):
            raise SystemExit("the timed launch disagrees with build_graph_batch")
        return go

    go_g, go_d = launcher(gated_batch, True), launcher(dense_batch, False)
    out = {True: [], False: []}
    for _ in range(9):
        for gated, go in ((True, go_g), (False, go_d)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(50):
                go()
            t1.record()
            t1.synchronize()
            out[gated].append(t0.elapsed_time(t1) * 1e3 / 50)
    return float(np.median(out[True])), float(np.median(out[False]))


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


def run_step(which):
    import torch

    import bench
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.ranking import PooledCurve
    b = batch(which)
    node, reid = torch.from_numpy(b["node"]).cuda(), torch.from_numpy(b["reid"]).cuda()
    args = (b["xw"], b["yw"], b["ids"], b["id_cam"], b["sizes"], b["max_dist"], node, reid)
    model = bench.build_model(bench.graph_net_params(), int(b["sizes"].max())).cuda().eval()
    dense_batch = build_graph_batch(*args)
    # random weights put every logit on one side of 0: centre them so that pruning and clustering have work to do
    with torch.no_grad():
        out = model(dense_batch)
        sd = model.state_dict()
        last_bias = [q for q in sd if q.startswith("classifier.") and q.endswith(".bias")][-1]
        sd[last_bias] -= out["classified_edges"][-1].median()
        model.load_state_dict(sd)
    e_dense = int(dense_batch.edge_index.shape[1])
    finite = [r for r in RADII if math.isfinite(r)]
    curve = PooledCurve([r / MAX_DIST for r in finite], keep="le").add(dense_batch, dense_batch.edge_attr[:, 0]).result()
    dense_pipe = FramePipeline(model)
    for radius in RADII:
        gated_batch = build_graph_batch(*args, radius=radius)
        e = int(gated_batch.edge_index.shape[1])
        pipe = FramePipeline(model, radius=radius)
        r = pipe(*args)
        torch.cuda.synchronize()
        if r._d2h is None or int(r.batch.edge_index.shape[1]) != e:
            raise SystemExit(f"{which} r={radius}: the one-call path was not taken")
        if math.isfinite(radius):
            k = finite.index(radius)
            kept, recall = float((curve["TP"][k] + curve["FP"][k]) / e_dense), float(curve["R"][k])
        else:
            kept, recall = e / e_dense, 1.0
        plan_g, plan_d = plan_us(b, radius)
        build_g, build_d = build_us(gated_batch, dense_batch, radius)
        d1, sd1 = ms_per_batch(lambda: dense_pipe(*args)), ms_per_batch_stream(lambda: dense_pipe(*args))
        g1, sg1 = ms_per_batch(lambda: pipe(*args)), ms_per_batch_stream(lambda: pipe(*args))
        d2, sd2 = ms_per_batch(lambda: dense_pipe(*args)), ms_per_batch_stream(lambda: dense_pipe(*args))
        print(json.dumps(dict(batch=which, radius=radius if math.isfinite(radius) else "inf", n=b["n"], e_dense=e_dense, e=e, kept=round(kept, 4),
                              recall_same_identity=round(recall, 4), plan_us=round(plan_g, 2), plan_dense_us=round(plan_d, 2),
                              build_us=round(build_g, 2), build_dense_us=round(build_d, 2),
                              pipeline_ms=round(g1, 4), pipeline_dense_ms=[round(d1, 4), round(d2, 4)],
                              stream_pipeline_ms=round(sg1, 4), stream_pipeline_dense_ms=[round(sd1, 4), round(sd2, 4)])), flush=True)


def main():
    if "--step" in sys.argv:
        run_step(sys.argv[sys.argv.index("--step") + 1])
        return 0
    for step in STEPS:   # a fresh process per batch, each under its own limit; the first failure ends the run
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
