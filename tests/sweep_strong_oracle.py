"""The rule of the sweep over the strongly connected clusters (csrc/eval_sweep_strong.cuh, include/gnncca_mpn.h), restated with numpy on
host arrays: float64 comparisons against the widened float32 scores (tests/joint_sweep_oracle.py's), nothing pruned, the strongly connected
components of a frame's active in-frame edges (oracle/post_oracle.py: scipy), the scoring of tests/helpers/eval_oracle.py.  And the golden
frames of tests/golden/post_unpruned.npz as one batch."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import eval_oracle as eo  # noqa: E402
import joint_sweep_oracle as jo  # noqa: E402
from oracle import post_oracle as po  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "post_unpruned.npz")


def strong_labels(edge_index, node_ptr, edge_ptr, predictions):
    """labels [N]: per frame, the smallest batch-global id of the strongly connected component over the frame's predicted edges whose
    two ends lie in the frame."""
    ei = np.asarray(edge_index, dtype=np.int64)
    labels = np.arange(int(node_ptr[-1]), dtype=np.int64)
    for g in range(len(node_ptr) - 1):
        v0, v1, k0, k1 = int(node_ptr[g]), int(node_ptr[g + 1]), int(edge_ptr[g]), int(edge_ptr[g + 1])
        src, dst = ei[0, k0:k1] - v0, ei[1, k0:k1] - v0
        inside = (src >= 0) & (src < v1 - v0) & (dst >= 0) & (dst < v1 - v0)
        on = inside & (np.asarray(predictions[k0:k1]) == 1)
        if v1 > v0:
            labels[v0:v1] = v0 + po.clusters(np.stack([src[on], dst[on]]), np.ones(int(on.sum()), np.int64), v1 - v0)[0]
    return labels


def sweep_strong(edge_index, edge_labels, node_ptr, edge_ptr, scores, points, keep, frame_div=None):
    """-> (rows float64 [T, G, 16], labels int64 [T, N], predictions int64 [T, E]) of the rule, frame by frame and point by point."""
    ei = np.asarray(edge_index, dtype=np.int64)
    points = np.asarray(points, dtype=np.float64)
    g_count, n, e = len(node_ptr) - 1, int(node_ptr[-1]), ei.shape[1]
    rows = np.zeros((len(points), g_count, 16))
    labels = np.zeros((len(points), n), dtype=np.int64)
    preds = np.zeros((len(points), e), dtype=np.int64)
    for t in range(len(points)):
        for g in range(g_count):
            k0, k1 = int(edge_ptr[g]), int(edge_ptr[g + 1])
            th = jo.thresholds(points, frame_div, g)[t]
            preds[t, k0:k1] = jo.active_edges([np.asarray(s)[k0:k1] for s in scores], keep, th)
        labels[t] = strong_labels(ei, node_ptr, edge_ptr, preds[t])
        rows[t], _ = eo.eval_batch(ei, np.asarray(edge_labels), preds[t], labels[t], node_ptr, edge_ptr)
    return rows, labels, preds


def golden_frames():
    """[(name, n, edge_index [2, E] frame-local, probs float32 [E], getter)] of the 26 frames."""
    z = np.load(GOLDEN)
    out = []
    for name in (str(s) for s in z["names"]):
        g = lambda k, name=name: z[f"{name}::{k}"]   # noqa: E731
        out.append((name, int(g("n_nodes")), g("edge_index").astype(np.int64), g("probs").astype(np.float32), g))
    return out


def golden_batch(frames=None, seed=7):
    """The golden frames as ONE batch on the host -> dict(edge_index [2, E], probs float32 [E], edge_labels float32 [E], node_ptr,
    edge_ptr).  The golden holds no ground-truth identities: edge_labels = 1 where the two ends share a seeded random identity."""
    frames = golden_frames() if frames is None else frames
    rng = np.random.default_rng(seed)
    node_ptr, edge_ptr, eis, probs, labs = [0], [0], [], [], []
    for _, n, ei, pr, _ in frames:
        ident = rng.integers(0, max(n // 2, 1) + 1, size=n)
        eis.append(ei + node_ptr[-1])
        probs.append(pr)
        labs.append((ident[ei[0]] == ident[ei[1]]).astype(np.float32))
        node_ptr.append(node_ptr[-1] + n)
        edge_ptr.append(edge_ptr[-1] + ei.shape[1])
    return dict(edge_index=np.concatenate(eis, axis=1), probs=np.concatenate(probs), edge_labels=np.concatenate(labs), node_ptr=node_ptr,
                edge_ptr=edge_ptr)
