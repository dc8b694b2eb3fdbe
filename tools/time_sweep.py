#!/usr/bin/env python3
"""Time calibration.sweep_thresholds against the loop it replaces; prints ONE JSON line.

The loop is what a user had before: per threshold, the predictions at the threshold, `prune_and_cluster`, `evaluate_frames` -- the
functions the sweep's results are defined by, which the sweep did not change, so the loop is the yardstick.  Two forms of it are timed:
`loop_at` makes the predictions with `postprocess.threshold(logits, at=t)` (one launch; only a tree that has the switch), `loop_torch`
with `(probs.double() >= t)` in torch (what a tree without the switch can do).  With `--parent PATH` (a checkout of the parent commit
with its library built) a child process times `loop_torch` there too, before and after this tree's rounds.

Batch: 64 frames of 4 cameras x 8 detections, every cross-camera pair an edge (graph_build.build_graph_batch); the scores are the
sigmoid of seeded random logits; thresholds np.arange(0.01, 1.01, 0.01), as main.py:143 sweeps them.  Method: every side is warmed up,
then timed as `reps` back-to-back repetitions that end in ONE device synchronise, host clock around them; the sides alternate inside a
round, several rounds; the line carries every round's figure, the median and the spread (max - min over the rounds).

    python tools/time_sweep.py [--rounds 7] [--reps 20] [--loop-reps 3] [--parent PATH]

`--partition exclusive` times the sweep of the camera-exclusive partition (sweep_thresholds(partition='exclusive')) the same way, on the
same batch, against ITS loop: per threshold `postprocess.exclusive_clusters(at=t)` and `evaluate_frames` of its predictions and labels,
over np.arange(0.01, 1.00, 0.01) (the rule's thresholds lie strictly inside (0, 1)).  Both functions of that loop are older than the
sweep and untouched by it.

`--joint TAxTB` (say 100x100, main.py's own 0.01 step on two axes) times calibration.sweep_grid over a TA x TB grid on the same batch --
edge_attr[:, 0] < a AND edge_attr[:, 2] < b, the axes spread evenly over each column's range -- against ITS loop: per point the two
float64 comparisons in torch, `prune_and_cluster`, `evaluate_frames`, all older than the joint sweep and untouched by it.  A whole
loop is TA * TB points: --loop-reps 1 is plenty.  It also times folding `--acc-batches` such row sets into a JointSweepAccumulator
(`accumulate`: one add per batch) against keeping a copy of each and reducing them once with torch (`keep_rows`: clone, cat, sum),
both on the device alone; prints the bytes each way holds there; and times one result() (`result_ms`: the synchronisation, the copy
and the host's T dicts).

`--partition strong` times the sweep over the STRONGLY CONNECTED clusters (sweep_thresholds(partition='strong'), nothing pruned) on two
batches, tools/time_strong_clusters.py's shapes: 64 frames x 32 detections and 16 frames x 128 detections.  Its loop is per threshold
`postprocess.threshold(logits, at=t)`, `postprocess.strong_clusters`, `evaluate_frames` -- all older than the sweep and untouched by it
-- and the 'components' sweep of the same scores is timed next to it (another partition: mutual pairs; not the same rows).  With
`--joint TAxTB` the same for sweep_grid(partition='strong') against per point two float64 comparisons, `strong_clusters`,
`evaluate_frames`, and sweep_grid over the components.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def make_batch(torch, frames, cams, per_cam):
    from gnn_cca_amd.graph_build import build_graph_batch
    rng = np.random.default_rng(0)
    n = frames * cams * per_cam
    sizes = np.full(frames, cams * per_cam)
    id_cam = np.tile(np.repeat(np.arange(cams), per_cam), frames)
    ids = rng.integers(0, per_cam + 2, size=n)
    node = torch.from_numpy(rng.standard_normal((n, 32)).astype(np.float32)).cuda()
    reid = torch.from_numpy(rng.standard_normal((n, 32)).astype(np.float32)).cuda()
    b = build_graph_batch(rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), ids, id_cam, sizes, rng.uniform(10, 90, frames), node, reid)
    logits = torch.randn(b.edge_index.shape[1], generator=torch.Generator().manual_seed(0)).cuda()
    return b, logits


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


def time_exclusive(torch, args, b, probs):
    from gnn_cca_amd.calibration import sweep_thresholds
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import exclusive_clusters
    ths = np.arange(0.01, 1.00, 0.01)
    n, widest = int(b.node_ptr[-1]), int(np.diff(b.node_ptr).max())

    def loop():
        rows = []
        for t in ths:
            ex = exclusive_clusters(b.edge_index, probs, b.cam_dev, n, b.node_ptr_dev, b.edge_ptr_dev, at=float(t), max_frame_nodes=widest)
            rows.append(evaluate_frames(b, ex["predictions"], ex["labels"]))
        return rows

    def sweep():
        return sweep_thresholds(b, probs, ths, partition="exclusive")

    if not torch.equal(sweep(), torch.stack(loop())):   # (no NaN rows in this batch)
        raise SystemExit("the exclusive sweep and its loop disagree: nothing to time")
    sides = {"sweep_exclusive": (sweep, args.reps), "loop_exclusive": (loop, args.loop_reps)}
    for fn, _ in sides.values():   # warm-up: every shape and kernel of the timed windows
        fn()
        fn()
    got = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, (fn, reps) in sides.items():   # the sides alternate inside a round
            got[k].append(timed(torch, fn, reps))
    res = {"metric": "threshold sweep of the camera-exclusive partition, ms per 99 thresholds", "frames": len(b.node_ptr) - 1, "nodes": n,
           "edges": int(b.edge_index.shape[1]), "thresholds": len(ths), "rounds": args.rounds}
    res.update({k: summary(v) for k, v in got.items()})
    res["loop_over_sweep"] = round(float(np.median(got["loop_exclusive"]) / np.median(got["sweep_exclusive"])), 1)
    print(json.dumps(res))


def time_joint(torch, args, b):
    from gnn_cca_amd.calibration import JointSweepAccumulator, grid_points, sweep_grid
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import prune_and_cluster
    try:
        ta, tb = (int(v) for v in args.joint.lower().split("x"))
    except ValueError:
        raise SystemExit("--joint takes TAxTB, such as 100x100") from None
    n, g = int(b.node_ptr[-1]), len(b.node_ptr) - 1
    s0, s1 = b.edge_attr[:, 0], b.edge_attr[:, 2]
    axes = [np.linspace(float(s.min()), float(s.max()), t + 1)[1:] for s, t in ((s0, ta), (s1, tb))]
    pts, shape = grid_points(axes)
    d0, d1 = s0.double(), s1.double()

    def loop():
        rows = []
        for a, c in pts:
            preds = ((d0 < float(a)) & (d1 < float(c))).to(torch.int64)
            post = prune_and_cluster(b.edge_index, preds, n, b.node_ptr_dev, b.edge_ptr_dev)
            rows.append(evaluate_frames(b, post["pruned"], post["labels"]))
        return rows

    def grid():
        return sweep_grid(b, [s0, s1], axes, ["lt", "lt"])

    rows = grid()
    if not torch.equal(rows.reshape(len(pts), g, 16), torch.stack(loop())):   # (no NaN rows in this batch)
        raise SystemExit("the joint sweep and its loop disagree: nothing to time")
    flat = rows.reshape(len(pts), g, 16)

    acc = JointSweepAccumulator(pts)

    def accumulate():   # the device side of a data set: one launch per batch, nothing of the batch kept
        for _ in range(args.acc_batches):
            acc.add(flat)

    def keep_rows():    # (a data set's batches are distinct tensors: each one is held until the reduction)
        kept = [flat.clone() for _ in range(args.acc_batches)]
        return torch.cat(kept, dim=1).sum(dim=1)

    sides = {"grid": (grid, args.reps), "loop": (loop, args.loop_reps), "accumulate": (accumulate, args.acc_reps),
             "keep_rows": (keep_rows, args.acc_reps)}
    for fn, _ in sides.values():   # warm-up: every shape and kernel of the timed windows (the loop ran once above)
        fn()
    got = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, (fn, reps) in sides.items():   # the sides alternate inside a round
            got[k].append(timed(torch, fn, reps))
    res = {"metric": f"joint sweep, ms per {ta} x {tb} grid", "frames": g, "nodes": n, "edges": int(b.edge_index.shape[1]), "points": len(pts),
           "rounds": args.rounds, "acc_batches": args.acc_batches, "accumulator_device_bytes": (len(pts) * 16 + 1) * 8,
           "kept_rows_device_bytes": args.acc_batches * len(pts) * g * 16 * 8}
    res.update({k: summary(v) for k, v in got.items()})
    t0 = time.perf_counter()
    acc.result()   # one synchronisation, one copy, then the host's part: T dicts of aggregates and the micro scores
    res["result_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
    res["loop_over_grid"] = round(float(np.median(got["loop"]) / np.median(got["grid"])), 1)
    print(json.dumps(res))


def time_strong(torch, args):
    from gnn_cca_amd.calibration import grid_points, sweep_grid, sweep_thresholds
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import strong_clusters, threshold
    out = {"metric": "sweep over the strongly connected clusters, ms per sweep", "rounds": args.rounds, "batches": {}}
    for frames, per_cam in ((64, 8), (16, 32)):
        b, logits = make_batch(torch, frames, 4, per_cam)
        n, g, widest = int(b.node_ptr[-1]), frames, int(np.diff(b.node_ptr).max())
        probs, _ = threshold(logits)

        def clusters_rows(preds):
            post = strong_clusters(b.edge_index, preds, n, b.node_ptr_dev, b.edge_ptr_dev, max_frame_nodes=widest)
            return evaluate_frames(b, preds, post["labels"])

        if args.joint:
            try:
                ta, tb = (int(v) for v in args.joint.lower().split("x"))
            except ValueError:
                raise SystemExit("--joint takes TAxTB, such as 100x100") from None
            s0, s1 = b.edge_attr[:, 0], probs          # a symmetric ground distance AND an asymmetric score: directed cycles exist
            axes = [np.linspace(float(s.min()), float(s.max()), t + 1)[1:] for s, t in ((s0, ta), (s1, tb))]
            pts, _ = grid_points(axes)
            d0, d1 = s0.double(), s1.double()
            points = len(pts)

            def loop():
                return [clusters_rows(((d0 < float(a)) & (d1 >= float(c))).to(torch.int64)) for a, c in pts]

            def sweep():
                return sweep_grid(b, [s0, s1], axes, ["lt", "ge"], partition="strong")

            def components():
                return sweep_grid(b, [s0, s1], axes, ["lt", "ge"])
        else:
            ths = np.arange(0.01, 1.00, 0.01)   # (99: `threshold(at=t)` takes thresholds strictly inside (0, 1))
            points = len(ths)

            def loop():
                return [clusters_rows(threshold(logits, at=float(t))[1]) for t in ths]

            def sweep():
                return sweep_thresholds(b, probs, ths, partition="strong")

            def components():
                return sweep_thresholds(b, probs, ths)

        rows = sweep().reshape(points, g, 16)
        if not torch.equal(rows, torch.stack(loop())):   # (no NaN rows in these batches)
            raise SystemExit("the strong sweep and its loop disagree: nothing to time")
        differ = int((rows != components().reshape(points, g, 16)).any(dim=2).sum())
        sides = {"sweep_strong": (sweep, args.reps), "loop_strong": (loop, args.loop_reps), "sweep_components": (components, args.reps)}
        for fn, _ in sides.values():   # warm-up: every shape and kernel of the timed windows (each side also ran once above)
            fn()
        got = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, (fn, reps) in sides.items():   # the sides alternate inside a round
                got[k].append(timed(torch, fn, reps))
        res = {"frames": g, "nodes": n, "edges": int(b.edge_index.shape[1]), "points": points,
               "cells_where_strong_rows_differ_from_components": differ, "cells": points * g}
        res.update({k: summary(v) for k, v in got.items()})
        res["loop_over_sweep"] = round(float(np.median(got["loop_strong"]) / np.median(got["sweep_strong"])), 1)
        out["batches"][f"{frames}x{4 * per_cam}"] = res
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="sweeps per timed window")
    ap.add_argument("--loop-reps", type=int, default=3, help="whole loops (100 thresholds each) per timed window")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the tree whose gnn_cca_amd is timed")
    ap.add_argument("--loop-only", action="store_true", help="time loop_torch alone (what a child run in the parent's tree does)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its loop_torch is timed in a child process")
    ap.add_argument("--partition", choices=("components", "exclusive", "strong"), default="components", help="which partition's sweep is timed")
    ap.add_argument("--joint", default=None, metavar="TAxTB", help="time sweep_grid over a TA x TB grid against its per-point loop")
    ap.add_argument("--acc-reps", type=int, default=200, help="--joint: accumulate / keep_rows calls per timed window (a call is well under 1 ms)")
    ap.add_argument("--acc-batches", type=int, default=8, help="--joint: row sets folded into the accumulator / kept, per timed call")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import prune_and_cluster, threshold

    if not torch.cuda.is_available():
        raise SystemExit("tools/time_sweep.py measures on the GPU; no device found")
    if args.partition == "strong":
        return time_strong(torch, args)
    ths = np.arange(0.01, 1.01, 0.01)
    b, logits = make_batch(torch, 64, 4, 8)
    n = int(b.node_ptr[-1])
    probs, _ = threshold(logits)
    if args.joint:
        return time_joint(torch, args, b)
    if args.partition == "exclusive":
        return time_exclusive(torch, args, b, probs)

    def one(preds):
        post = prune_and_cluster(b.edge_index, preds, n, b.node_ptr_dev, b.edge_ptr_dev)
        return evaluate_frames(b, post["pruned"], post["labels"])

    def loop_torch():
        return [one((probs.double() >= float(t)).to(torch.int64)) for t in ths]

    sides = {"loop_torch": (loop_torch, args.loop_reps)}
    if not args.loop_only:
        from gnn_cca_amd.calibration import sweep_thresholds

        def loop_at():   # (`threshold(at=t)` takes t strictly inside (0, 1): the sweep's last point, 1.0, is compared in torch)
            return [one(threshold(logits, at=float(t))[1] if t < 1.0 else (probs.double() >= float(t)).to(torch.int64)) for t in ths]

        sides = {"sweep": (lambda: sweep_thresholds(b, probs, ths), args.reps), "loop_at": (loop_at, args.loop_reps), **sides}
        rows = sweep_thresholds(b, probs, ths)
        want = torch.stack(loop_at())
        if not (torch.equal(rows, want) and torch.equal(want, torch.stack(loop_torch()))):   # (no NaN rows in this batch)
            raise SystemExit("the sweep and the loop disagree: nothing to time")

    def parent_run():
        if not args.parent:
            return None
        cmd = [sys.executable, os.path.abspath(__file__), "--root", args.parent, "--loop-only", "--rounds", str(max(args.rounds // 2, 2)),
               "--loop-reps", str(args.loop_reps)]
        return json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])["loop_torch"]

    before = parent_run()
    for fn, _ in sides.values():   # warm-up: every shape and kernel of the timed windows
        fn()
        fn()
    got = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, (fn, reps) in sides.items():
            got[k].append(timed(torch, fn, reps))
    after = parent_run()
    res = {"metric": "threshold sweep, ms per 100 thresholds", "frames": 64, "nodes": n, "edges": int(b.edge_index.shape[1]),
           "thresholds": len(ths), "rounds": args.rounds, "root": "parent" if args.loop_only else "this tree"}
    res.update({k: summary(v) for k, v in got.items()})
    if before is not None:
        res["parent_loop_torch_before"], res["parent_loop_torch_after"] = before, after
    if "sweep" in got:
        res["loop_at_over_sweep"] = round(float(np.median(got["loop_at"]) / np.median(got["sweep"])), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
