#!/usr/bin/env python3
"""Time ranking.rank_metrics (K = 1 and K = 4) and one PooledCurve.add against the host loops they replace; prints ONE JSON line.

The host loops are what a user had before: copy the scores and labels back, then per frame scikit-learn's roc_auc_score and
average_precision_score (frames with one class skipped, as they must be); and for the pooled curve numpy's loop over 100 thresholds as
main.py:141-175 runs it -- `dist <= t`, the four counts, P / R / F -- on the copied vector.  scikit-learn missing: the device sides are
timed alone and the line says so.

Batch: the joint sweep's (tools/time_sweep.py): 64 frames of 4 cameras x 8 detections, every cross-camera pair an edge (768 per frame,
49152 in all); the scores are the four columns of edge_attr (K = 1: the ReID distance, column 2, positive='low').  Method: every side
is warmed up, then timed as `reps` back-to-back repetitions that end in ONE device synchronise, host clock around them; the sides
alternate inside a round, several rounds; the line carries every round's figure, the median and the spread (max - min over the rounds).
Before anything is timed the device rows are compared with scikit-learn's numbers (1e-11) and the pooled counts with the loop's (equal).

    python tools/time_rank_metrics.py [--rounds 7] [--reps 50] [--host-reps 2] [--frames 64] [--cams 4] [--per-cam 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from time_sweep import make_batch, summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="device calls per timed window")
    ap.add_argument("--host-reps", type=int, default=2, help="whole host loops per timed window")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--per-cam", type=int, default=8)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the tree whose gnn_cca_amd is timed")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_rank_metrics.py measures on the GPU; no device found")
    from gnn_cca_amd.ranking import PooledCurve, rank_metrics
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
    except ImportError:
        roc_auc_score = average_precision_score = None

    b, _ = make_batch(torch, args.frames, args.cams, args.per_cam)
    ptr = np.asarray(b.edge_ptr)
    cols = [b.edge_attr[:, q] for q in range(4)]
    positive = ["low", "low", "low", "low"]
    dist = cols[2]
    ths = np.arange(0.01, 1.01, 0.01) * float(dist.max())     # main.py:141 normalises by the data set's maximum; here the thresholds scale
    curve = PooledCurve(ths, keep="le")

    def host_rank(k):
        lab = b.edge_labels.cpu().numpy()
        out = np.full((k, len(ptr) - 1, 2), np.nan)
        for q in range(k):
            s = -cols[q].cpu().numpy().astype(np.float64)
            for g in range(len(ptr) - 1):
                l, v = lab[ptr[g]:ptr[g + 1]], s[ptr[g]:ptr[g + 1]]
                if 0 < l.sum() < len(l):
                    out[q, g] = roc_auc_score(l, v), average_precision_score(l, v)
        return out

    def host_pool():
        d, lab = dist.cpu().numpy().astype(np.float64), b.edge_labels.cpu().numpy()
        pos, neg = lab == 1, lab == 0
        rows = []
        for t in ths:
            pred = d <= t
            tp, fp = int((pred & pos).sum()), int((pred & neg).sum())
            fn, tn = int(pos.sum()) - tp, int(neg.sum()) - fp
            p = tp / (tp + fp) if tp + fp else 0
            r = tp / (tp + fn) if tp + fn else 0
            rows.append((tp, fp, fn, tn, p, r, 2 * (p * r) / (p + r) if p + r else 0))
        return rows

    sides = {"rank_k1": (lambda: rank_metrics(b, dist, "low"), args.reps), "rank_k4": (lambda: rank_metrics(b, cols, positive), args.reps),
             "pool_add": (lambda: curve.add(b, dist), args.reps), "host_pool": (host_pool, args.host_reps)}
    if roc_auc_score is not None:
        sides["host_rank_k1"] = (lambda: host_rank(1), args.host_reps)
        sides["host_rank_k4"] = (lambda: host_rank(4), args.host_reps)
        rows, want = rank_metrics(b, cols, positive).cpu().numpy(), host_rank(4)
        ok = ~np.isnan(want[:, :, 0])
        if not (np.array_equal(ok, ~np.isnan(rows[:, :, 4])) and np.abs(rows[:, :, 4:6][ok] - want[ok]).max() <= 1e-11):
            raise SystemExit("rank_metrics and scikit-learn disagree: nothing to time")
    res = PooledCurve(ths, keep="le").add(b, dist).result()
    if [(int(a), int(c), int(d), int(e)) for a, c, d, e in zip(res["TP"], res["FP"], res["FN"], res["TN"])] != [r[:4] for r in host_pool()]:
        raise SystemExit("the pooled curve and the host loop disagree: nothing to time")
    for fn, _ in sides.values():   # warm-up: every shape and kernel of the timed windows
        fn()
        fn()
    got = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, (fn, reps) in sides.items():   # the sides alternate inside a round
            got[k].append(timed(torch, fn, reps))
    out = {"metric": "ranking scores, ms per call on one batch", "frames": len(ptr) - 1, "edges": int(b.edge_index.shape[1]),
           "frame_edges": int(np.diff(ptr).max()), "thresholds": len(ths), "rounds": args.rounds,
           "scikit_learn": roc_auc_score is not None}
    out.update({k: summary(v) for k, v in got.items()})
    for dev, host in (("rank_k1", "host_rank_k1"), ("rank_k4", "host_rank_k4"), ("pool_add", "host_pool")):
        if host in got:
            out[f"{host}_over_{dev}"] = round(float(np.median(got[host]) / np.median(got[dev])), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
