#!/usr/bin/env python3
"""Time postprocess.strong_clusters (one memset, one launch: the strongly connected components of the unpruned predictions) against
postprocess.prune_and_cluster (the parent's device chain: plan, plan finish, prune, components -- the yardstick) and against scipy's
connected_components(connection='strong') per frame after a copy back, on the same batches; prints ONE JSON line.  One MI355X.

Batches (synthetic, no model): frames of C cameras x D detections with every cross-camera ordered pair an edge, predictions thresholded
from noisy identity logits (where(same identity, 1.0, -2.0) + N(0, 1.5): the tests' noisy frames) --
    terrace   64 frames of 4 x 8 detections  (2048 nodes, 49 152 edges)
    wide      16 frames of 4 x 32 detections (2048 nodes, 196 608 edges)

Method: a window is --calls back-to-back calls under the host clock, ending in ONE synchronise; the same window between two GPU events
gives the device time.  The sides alternate inside a round, over --rounds rounds; the line carries every round's figure, the median and
the spread (max - min).  scipy's side includes the copy of edge_index and predictions to the host, which is what a caller without the
kernel pays.

    python tools/time_strong_clusters.py [--calls 50] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(vals):
    return {"rounds_ms": [round(v, 4) for v in vals], "median_ms": round(float(np.median(vals)), 4),
            "spread_ms": round(float(max(vals) - min(vals)), 4)}


def make_batch(rng, g, cams, per_cam):
    n = cams * per_cam
    cam = np.repeat(np.arange(cams), per_cam)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    m = cam[i] != cam[j]
    src, dst = i[m], j[m]                                  # row-major: the reference's edge order
    eis, preds = [], []
    for q in range(g):
        ident = rng.integers(0, max(n // 4, 2), size=n)
        logits = np.where(ident[src] == ident[dst], 1.0, -2.0) + rng.normal(0, 1.5, size=len(src))
        eis.append(np.stack([src, dst]) + q * n)
        preds.append((logits >= 0).astype(np.int64))
    node_ptr = (np.arange(g + 1) * n).tolist()
    edge_ptr = (np.arange(g + 1) * len(src)).tolist()
    return np.concatenate(eis, axis=1), np.concatenate(preds), node_ptr, edge_ptr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("at least 5 rounds")
    import scipy.sparse as sp
    import torch
    from scipy.sparse.csgraph import connected_components

    from gnn_cca_amd.postprocess import prune_and_cluster, strong_clusters

    if not torch.cuda.is_available():
        raise SystemExit("tools/time_strong_clusters.py measures on the GPU; no device found")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = {"metric": "ms per call on one batch", "calls_per_window": args.calls, "rounds": args.rounds}
    for name, (g, cams, per_cam) in (("terrace_64x32", (64, 4, 8)), ("wide_16x128", (16, 4, 32))):
        ei, pred, node_ptr, edge_ptr = make_batch(rng, g, cams, per_cam)
        n, width = node_ptr[-1], cams * per_cam
        ei_d, pred_d = torch.from_numpy(ei).to(dev), torch.from_numpy(pred).to(dev)
        nptr, eptr = torch.tensor(node_ptr, dtype=torch.int32, device=dev), torch.tensor(edge_ptr, dtype=torch.int32, device=dev)

        def strong():
            return strong_clusters(ei_d, pred_d, n, nptr, eptr, max_frame_nodes=width)

        def pruned():
            return prune_and_cluster(ei_d, pred_d, n, nptr, eptr)

        def scipy_side():
            e_h, p_h = ei_d.cpu().numpy(), pred_d.cpu().numpy().astype(bool)
            out = []
            for q in range(g):
                k0, k1, v0 = edge_ptr[q], edge_ptr[q + 1], node_ptr[q]
                a, b = e_h[0, k0:k1][p_h[k0:k1]] - v0, e_h[1, k0:k1][p_h[k0:k1]] - v0
                m = sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(width, width)).tocsr()
                out.append(connected_components(m, directed=True, connection="strong"))
            return out

        def window(fn, calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            keep = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(calls):
                keep.append(fn())
            b.record()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / calls, a.elapsed_time(b) / calls

        # what is being timed: the two partitions of this batch, and that the kernel accepted every frame
        s, p = strong(), pruned()
        torch.cuda.synchronize()
        if int(s["flags"].sum().item()):
            raise SystemExit("strong_clusters refused a frame of this batch: nothing to time")
        for fn in (strong, pruned):    # warm-up: code objects, the allocator's blocks
            window(fn, args.calls)
        scipy_calls = max(args.calls // 10, 2)
        window(scipy_side, 2)
        got = {"strong_host_clock": [], "strong_gpu_events": [], "prune_and_cluster_host_clock": [], "prune_and_cluster_gpu_events": [],
               "scipy_host_clock": []}
        for r in range(args.rounds):
            order = (strong, pruned) if r % 2 == 0 else (pruned, strong)
            for fn in order:
                host, events = window(fn, args.calls)
                key = "strong" if fn is strong else "prune_and_cluster"
                got[key + "_host_clock"].append(host), got[key + "_gpu_events"].append(events)
            got["scipy_host_clock"].append(window(scipy_side, scipy_calls)[0])
        entry = {"frames": g, "nodes_per_frame": width, "nodes": n, "edges": int(ei.shape[1]), "active_edges": int(pred.sum()),
                 "clusters_strong": int(s["n_clusters"].item()), "clusters_pruned": int(p["n_clusters"].item()),
                 "scipy_calls_per_window": scipy_calls}
        entry.update({k: summary(v) for k, v in got.items()})
        entry["prune_and_cluster_over_strong_host_clock"] = round(float(np.median(got["prune_and_cluster_host_clock"]) /
                                                                        np.median(got["strong_host_clock"])), 2)
        entry["scipy_over_strong_host_clock"] = round(float(np.median(got["scipy_host_clock"]) / np.median(got["strong_host_clock"])), 2)
        res[name] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
