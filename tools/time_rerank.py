#!/usr/bin/env python3
"""Time the three launches of gnn_cca_amd.rerank against the float32 numpy oracle (tests/rerank_oracle.py); prints ONE JSON line.

Batch: 64 Terrace-shaped frames (19 .. 34 detections on 4 cameras, every cross-camera pair an edge, reid width 256: clustered
embeddings, persons x cameras + noise).  GPU sides: frame_distances, rerank_frames (k1=20, k2=6, lam=0.3), rank_predictions (rank 1) and
the whole rank_baseline, each warmed up, then timed as `reps` back-to-back calls that end in ONE device synchronise, host clock around
them, several rounds; the line carries every round's figure, the median and the spread (max - min).  `--big` adds one batch of 64 frames
of 128 detections (the LDS limit: one workgroup per CU).  The oracle runs once on the host: it is the reference's algorithm in numpy
with its Python loops, not an optimised CPU implementation, and its time says what the loops cost, nothing more.  The times are
reported; nothing is asserted about them.

    python tools/time_rerank.py [--rounds 5] [--reps 50] [--big]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_batch(torch, sizes, width=256, cams=4, seed=0):
    from gnn_cca_amd.graph_build import build_graph_batch
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)
    n = int(sizes.sum())
    id_cam = np.concatenate([np.arange(s) % cams for s in sizes])
    ids = np.concatenate([np.arange(s) // cams for s in sizes])
    centres = rng.normal(0, 1, size=(int(ids.max()) + 1, width))
    reid = (centres[ids] + 0.6 * rng.normal(0, 1, size=(n, width))).astype(np.float32)
    node = torch.from_numpy(rng.standard_normal((n, 32)).astype(np.float32)).cuda()
    b = build_graph_batch(rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), ids, id_cam, sizes, rng.uniform(10, 90, len(sizes)), node,
                          torch.from_numpy(reid).cuda())
    return b, id_cam


def timed(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def summary(vals):
    return {"rounds_ms": [round(v, 4) for v in vals], "median_ms": round(float(np.median(vals)), 4),
            "spread_ms": round(float(max(vals) - min(vals)), 4)}


def measure(torch, b, rounds, reps):
    from gnn_cca_amd.rerank import frame_distances, rank_baseline, rank_predictions, rerank_frames
    dist = frame_distances(b)
    rer = rerank_frames(dist)
    sides = {"frame_distances": lambda: frame_distances(b), "rerank_frames": lambda: rerank_frames(dist),
             "rank_predictions": lambda: rank_predictions(b, rer, 1), "rank_baseline": lambda: rank_baseline(b)}
    for fn in sides.values():
        fn()
    res = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            res[k].append(timed(torch, fn, reps))
    return {k: summary(v) for k, v in res.items()}, dist, rer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--big", action="store_true", help="also 64 frames of 128 detections")
    args = ap.parse_args()
    import torch
    import rerank_oracle as oracle

    if not torch.cuda.is_available():
        raise SystemExit("tools/time_rerank.py measures on the GPU; no device found")
    sizes = np.random.default_rng(1).integers(19, 35, size=64)
    b, cam = make_batch(torch, sizes)
    out = {"frames": 64, "nodes": int(b.node_ptr[-1]), "edges": int(b.edge_index.shape[1]), "largest_frame": int(sizes.max()),
           "reps": args.reps}
    gpu, dist, rer = measure(torch, b, args.rounds, args.reps)
    out["gpu"] = gpu
    x = b.reid_embeds.cpu().numpy()
    ei = b.edge_index.cpu().numpy()
    t0 = time.perf_counter()
    d32 = [m.astype(np.float32) for m in oracle.frame_distances(x, b.node_ptr, np.float32)]
    t1 = time.perf_counter()
    r32 = oracle.rerank_frames(d32, 20, 6, 0.3, np.float32)
    t2 = time.perf_counter()
    p = oracle.rank_predictions(r32, b.node_ptr, cam, ei, 1)
    t3 = time.perf_counter()
    out["oracle_float32_ms"] = {"frame_distances": round((t1 - t0) * 1e3, 1), "rerank_frames": round((t2 - t1) * 1e3, 1),
                                "rank_predictions": round((t3 - t2) * 1e3, 1)}
    got = [rer.frame(g).cpu().numpy() for g in range(len(rer))]
    out["max_abs_diff_vs_oracle32"] = float(max(np.abs(a - w).max() for a, w in zip(got, oracle.rerank_frames(
        [dist.frame(g).cpu().numpy() for g in range(len(dist))], 20, 6, 0.3, np.float32))))
    out["predicted_edges"] = int(p.sum())
    if args.big:
        bb, _ = make_batch(torch, np.full(64, 128), seed=2)
        out["big"] = {"nodes": int(bb.node_ptr[-1]), "edges": int(bb.edge_index.shape[1]), "gpu": measure(torch, bb, args.rounds, args.reps)[0]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
