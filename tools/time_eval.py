#!/usr/bin/env python3
"""Time gnn_cca_amd.evaluation.evaluate_frames against host scoring of the same frames; prints ONE JSON line.

Two batches: 64 Terrace-shaped frames (4 cameras x ~5 detections, every cross-camera pair an edge) and 512 frames of 128 nodes.  The
device time is events around many back-to-back launches (per batch); the host time is scikit-learn's five calls per frame plus the
P / R / F counts when scikit-learn is importable, otherwise the test restatement (tests/helpers/eval_oracle.py), on host copies.

    python tools/time_eval.py [--iters 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def make_batch(rng, sizes, cams=4):
    from gnn_cca_amd.sharding import GraphBatch
    node_ptr, edge_ptr, src, dst, lab, pred, labels = [0], [0], [], [], [], [], []
    for n in sizes:
        v0 = node_ptr[-1]
        cam = rng.integers(0, cams, size=n)
        ident = rng.integers(0, max(n // 4, 1), size=n)
        a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        keep = cam[a] != cam[b]
        s, d = a[keep], b[keep]
        gt = (ident[s] == ident[d]).astype(np.float32)
        p = (rng.random(len(s)) < np.where(gt == 1, 0.85, 0.05)).astype(np.int64)
        part = ident.copy()
        moved = rng.random(n) < 0.2
        part[moved] = rng.integers(0, n, size=int(moved.sum())) + n
        first = {}
        for v, c in enumerate(part.tolist()):
            first.setdefault(c, v)
        labels.append(np.array([first[c] + v0 for c in part.tolist()], np.int32))
        src.append(s + v0)
        dst.append(d + v0)
        lab.append(gt)
        pred.append(p)
        node_ptr.append(v0 + n)
        edge_ptr.append(edge_ptr[-1] + len(s))
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    b = GraphBatch(None, torch.from_numpy(ei).cuda(), None, edge_ptr, node_ptr)
    b.edge_labels = torch.from_numpy(np.concatenate(lab)).cuda()
    b.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    b.edge_ptr_dev = torch.tensor(edge_ptr, dtype=torch.int32).cuda()
    return b, torch.from_numpy(np.concatenate(pred)).cuda(), torch.from_numpy(np.concatenate(labels)).cuda()


def host_scoring(b, pred, labels, max_frames):
    """Seconds per frame of the host path on copies of the first `max_frames` frames, and which path it was."""
    ei, lab, pr, lb = b.edge_index.cpu().numpy(), b.edge_labels.cpu().numpy(), pred.cpu().numpy(), labels.cpu().numpy()
    import eval_oracle as eo
    try:
        from sklearn import metrics
        what = "sklearn"
    except ImportError:
        metrics, what = None, "restatement"
    g = min(max_frames, len(b.node_ptr) - 1)
    t0 = time.perf_counter()
    for q in range(g):
        v0, v1, k0, k1 = b.node_ptr[q], b.node_ptr[q + 1], b.edge_ptr[q], b.edge_ptr[q + 1]
        src, dst = ei[0, k0:k1] - v0, ei[1, k0:k1] - v0
        if metrics is None:
            eo.eval_frame(src, dst, lab[k0:k1], pr[k0:k1], lb[v0:v1], v1 - v0)
        else:
            eo.p_r_f(pr[k0:k1], lab[k0:k1])
            gt = eo.components(v1 - v0, src, dst, lab[k0:k1] == 1)
            p = lb[v0:v1]
            metrics.adjusted_rand_score(gt, p)
            metrics.adjusted_mutual_info_score(gt, p)
            metrics.homogeneity_score(gt, p)
            metrics.completeness_score(gt, p)
            metrics.v_measure_score(gt, p)
    return (time.perf_counter() - t0) / max(g, 1), what


def time_device(b, pred, labels, iters):
    from gnn_cca_amd.evaluation import evaluate_frames
    for _ in range(5):
        evaluate_frames(b, pred, labels)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        evaluate_frames(b, pred, labels)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-frames", type=int, default=64)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    res = {"metric": "evaluate_frames"}
    for name, sizes in (("terrace64", rng.integers(16, 24, size=64)), ("frames512x128", np.full(512, 128))):
        b, pred, labels = make_batch(rng, sizes)
        us = time_device(b, pred, labels, args.iters)
        host_s, what = host_scoring(b, pred, labels, args.host_frames)
        g = len(sizes)
        res[name] = {"frames": g, "nodes": int(b.node_ptr[-1]), "edges": int(b.edge_ptr[-1]), "device_us_per_batch": round(us, 2),
                     "host_path": what, "host_ms_per_frame": round(host_s * 1e3, 3), "host_ms_per_batch": round(host_s * 1e3 * g, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
