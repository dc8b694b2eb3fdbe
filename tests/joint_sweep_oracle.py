"""The joint sweep's rule (csrc/eval_sweep_joint.cuh, include/gnncca_mpn.h) and the accumulation order of gnncca_eval_rows_accumulate,
restated with numpy on host arrays.  The scoring of a partition is tests/helpers/eval_oracle.py's (the restatement of evaluate.hip)."""
import operator
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import eval_oracle as eo  # noqa: E402

CMP = {"ge": operator.ge, "gt": operator.gt, "le": operator.le, "lt": operator.lt}


def thresholds(points, frame_div, g):
    """th[t][k] of frame g: points[t][k] / frame_div[k][g] in float64 (one IEEE division), points[t][k] itself without divisors."""
    points = np.asarray(points, dtype=np.float64)
    if frame_div is None:
        return points
    return points / np.asarray(frame_div, dtype=np.float64)[:, g][None, :]


def active_edges(scores, keep, th):
    """[E] bool: every condition holds, the float32 score widened to float64 and compared in float64 (a NaN is never active)."""
    on = np.ones(len(scores[0]), dtype=bool)
    with np.errstate(invalid="ignore"):
        for s, c, t in zip(scores, keep, th):
            on &= CMP[c](np.asarray(s, dtype=np.float32).astype(np.float64), np.float64(t))
    return on


def kept_edges(edge_index, edge_ptr, active):
    """[E] int64: active, and the reverse edge of the SAME frame exists and is active."""
    ei = np.asarray(edge_index)
    frame_of = np.searchsorted(np.asarray(edge_ptr), np.arange(ei.shape[1]), side="right")
    where = {}
    for k, (a, b) in enumerate(ei.T.tolist()):
        where.setdefault((a, b, int(frame_of[k])), k)
    kept = np.zeros(ei.shape[1], dtype=np.int64)
    for k, (a, b) in enumerate(ei.T.tolist()):
        r = where.get((b, a, int(frame_of[k])))
        kept[k] = int(active[k] and r is not None and active[r])
    return kept


def sweep_joint(edge_index, edge_labels, node_ptr, edge_ptr, scores, points, keep, frame_div=None):
    """-> (rows float64 [T, G, 16], labels int64 [T, N], kept int64 [T, E]) of the rule, frame by frame and point by point."""
    ei = np.asarray(edge_index, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64)
    g_count, n, e = len(node_ptr) - 1, int(node_ptr[-1]), ei.shape[1]
    rows = np.zeros((len(points), g_count, 16))
    labels = np.tile(np.arange(n, dtype=np.int64), (len(points), 1))
    kept = np.zeros((len(points), e), dtype=np.int64)
    for t in range(len(points)):
        active = np.zeros(e, dtype=bool)
        for g in range(g_count):
            k0, k1 = int(edge_ptr[g]), int(edge_ptr[g + 1])
            th = thresholds(points, frame_div, g)[t]
            active[k0:k1] = active_edges([np.asarray(s)[k0:k1] for s in scores], keep, th)
        kept[t] = kept_edges(ei, edge_ptr, active)
        for g in range(g_count):
            v0, v1, k0, k1 = int(node_ptr[g]), int(node_ptr[g + 1]), int(edge_ptr[g]), int(edge_ptr[g + 1])
            labels[t, v0:v1] = v0 + eo.components(v1 - v0, ei[0, k0:k1] - v0, ei[1, k0:k1] - v0, kept[t, k0:k1])
        rows[t], _ = eo.eval_batch(ei, np.asarray(edge_labels), kept[t], labels[t], node_ptr, edge_ptr)
    return rows, labels, kept


def accumulate(sums, rows):
    """gnncca_eval_rows_accumulate: sums[t][c] = ((sums[t][c] + rows[t][0][c]) + rows[t][1][c]) + ..., float64, frames ascending."""
    sums = np.array(sums, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    for g in range(rows.shape[1]):
        sums = sums + rows[:, g, :]
    return sums


def accumulator_result(batches):
    """What JointSweepAccumulator.result() holds after add() of every [T, G_i, 16] array in `batches`: (sums, frames, means)."""
    sums = np.zeros((batches[0].shape[0], 16))
    frames = 0
    for rows in batches:
        sums = accumulate(sums, rows)
        frames += rows.shape[1]
    return sums, frames, sums / np.float64(frames)
