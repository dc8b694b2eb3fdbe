"""Numpy restatement of the capped graph build (build_graph_batch(top_k=k, rank_by=...)), written from its definition, not from the
kernel.  TEST INFRASTRUCTURE.

Definition: take the dense build (oracle.graph_oracle: the reference's complete cross-camera graph); for every source keep the
min(k, deg) out-edges of smallest key, ties to the smaller destination node id; mask the dense edge list (the kept edges stay in the
dense order).  Keys: 'ground' the ground-plane L2 distance in float64 before the division by max_dist; 'reid' the fp32
F.pairwise_distance value of the normalised reid rows (the `emb` attribute).
Backward: the selection is piecewise constant, so the gradient is the dense build's with a zero upstream gradient on every dropped edge
(tests/helpers/graph_grad_oracle.py's per-edge formulas, in float64).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import graph_grad_oracle as ggo  # noqa: E402
from oracle import graph_oracle  # noqa: E402


def dense(a, reid_n=None):
    """(edge_index, edge_attr, edge_labels) of the dense build of a fixture-shaped dict (raw embeddings; CPU normalisation)."""
    if reid_n is None:
        reid_n = graph_oracle.normalize_columns(a["reid_embeds_raw"])
    return graph_oracle.build(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], reid_n,
                              bool(a["only_appearance"]), bool(a["only_dist"]))


def keys(a, ei, rank_by, reid_n=None):
    """The ranking key of every dense edge: float64 [E] ('ground') or float32 [E] ('reid')."""
    r, c = ei
    if rank_by == "ground":
        xw, yw = np.asarray(a["xw"], np.float64), np.asarray(a["yw"], np.float64)
        dx, dy = xw[r] - xw[c], yw[r] - yw[c]
        return np.sqrt(dx * dx + dy * dy)
    if rank_by != "reid":
        raise ValueError(rank_by)
    if reid_n is None:
        reid_n = graph_oracle.normalize_columns(a["reid_embeds_raw"])
    # the emb column of the FULL attribute set, whatever the case emits
    _, attr, _ = graph_oracle.build(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], reid_n, False, False)
    return attr[:, 2]


def segments(ei):
    """[(start, stop)] of every source's contiguous run in the dense edge list."""
    src = ei[0]
    if src.size == 0:
        return []
    cut = np.flatnonzero(np.diff(src) != 0) + 1
    return list(zip(np.concatenate([[0], cut]).tolist(), np.concatenate([cut, [src.size]]).tolist()))


def select(ei, key, k):
    """bool [E]: the kept edges."""
    keep = np.zeros(ei.shape[1], dtype=bool)
    for s0, s1 in segments(ei):
        order = np.lexsort((ei[1, s0:s1], key[s0:s1]))   # by key, ties by destination id
        keep[s0 + order[:min(k, s1 - s0)]] = True
    return keep


def near_ties(ei, key, k, rel=1e-6):
    """Sources whose k-th and (k+1)-th smallest keys are closer than `rel` relative: a last-ulp difference between two evaluations
    of the key could flip their selection."""
    out = []
    for s0, s1 in segments(ei):
        if s1 - s0 <= k:
            continue
        ks = np.sort(np.asarray(key[s0:s1], np.float64))
        lo, hi = ks[k - 1], ks[k]
        if hi - lo < rel * max(abs(hi), np.finfo(np.float64).tiny):
            out.append(int(ei[0, s0]))
    return out


def degrees(a):
    """deg of every node (cross-camera candidates in its own frame), by node id."""
    cams = np.asarray(a["id_cam"])
    out, off = np.zeros(len(cams), np.int64), 0
    for n in np.asarray(a["graph_sizes"]).tolist():
        c = cams[off:off + n]
        out[off:off + n] = n - (c[:, None] == c[None, :]).sum(axis=1)
        off += n
    return out


def build(a, k, rank_by, reid_n=None):
    """(edge_index, edge_attr, edge_labels, keep) of the capped build; `keep` masks the dense edge list."""
    ei, attr, lab = dense(a, reid_n)
    keep = select(ei, keys(a, ei, rank_by, reid_n), k)
    return ei[:, keep], attr[keep], lab[keep], keep


def edge_ptr(a, k):
    """Per-frame edge ranges [G + 1] of the capped build: E_g = sum over the frame's nodes of min(k, deg)."""
    deg = np.minimum(degrees(a), k)
    node_ptr = np.concatenate([[0], np.cumsum(np.asarray(a["graph_sizes"], np.int64))])
    return np.concatenate([[0], np.cumsum([deg[node_ptr[g]:node_ptr[g + 1]].sum() for g in range(len(node_ptr) - 1)])]).astype(np.int64)


def backward(a, keep, g_edge_attr_kept, g_x=None):
    """(d_node, d_reid) in float64 of the capped build: upstream gradient `g_edge_attr_kept` [E_k, 4 or 2] on the kept edges."""
    g = np.zeros((keep.size, np.asarray(g_edge_attr_kept).shape[1]), np.float64)
    g[keep] = g_edge_attr_kept
    return ggo.graph_build_backward(a, np.float64, g_x=g_x, g_ea=g)


# ---- the synthetic cases the CPU and the GPU tests share ----
def _case(sizes_cams, xw, yw, reid, node_dim=8, seed=0, **modes):
    rng = np.random.default_rng(seed)
    id_cam = np.concatenate([np.asarray(c) for c in sizes_cams]).astype(np.int64)
    n = len(id_cam)
    return dict(graph_sizes=np.array([len(c) for c in sizes_cams], dtype=np.int64), id_cam=id_cam, id=rng.integers(0, 4, n),
                xw=np.asarray(xw, np.float64), yw=np.asarray(yw, np.float64), max_dist=rng.uniform(10, 50, len(sizes_cams)),
                node_embeds_raw=rng.standard_normal((n, node_dim)).astype(np.float32), reid_embeds_raw=np.asarray(reid, np.float32),
                only_appearance=np.bool_(modes.get("only_appearance", False)), only_dist=np.bool_(modes.get("only_dist", False)))


def degree_steps_case(seed=21):
    """Frame 0: cameras of 3, 2 and 1 detections -> deg 3, 4 and 5 (with k = 4: deg < k, deg == k, deg == k + 1; a camera of one
    detection).  Frame 1: two detections on one camera (no cross-camera partner: zero out-edges).  Frame 2: interleaved cameras."""
    rng = np.random.default_rng(seed)
    cams = [[0, 0, 0, 1, 1, 2], [3, 3], [1, 0, 2, 0, 1, 1, 2]]
    n = sum(len(c) for c in cams)
    return _case(cams, rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.standard_normal((n, 36)) + 0.5, seed=seed)


def frame100_case(seed=31):
    """One frame of 100 detections on three interleaved cameras: deg = 66 or 67 > 64, so a source's candidates fill more than one
    64-slot chunk (the golden 70-detection frame has deg 55: its FRAME spans two chunks, its candidates do not)."""
    rng = np.random.default_rng(seed)
    n = 100
    return _case([np.arange(n) % 3], rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.standard_normal((n, 20)) + 0.5, seed=seed)


def ties_case():
    """One frame with exact ties in both keys.  Detection 0 (camera 0) sits at the origin; detections 1 .. 4 (camera 1) at distance
    exactly 1 from it (integer coordinates) with IDENTICAL reid rows; 5 and 6 (camera 2) are farther away in both keys.  Detection 7
    (camera 0) at (0, 0) too, with detection 0's reid row: it ties with 0 as a destination of everyone else."""
    xw = [0, 1, 0, -1, 0, 3, 0, 0]
    yw = [0, 0, 1, 0, -1, 4, 2, 0]
    rng = np.random.default_rng(5)
    base, near, far = rng.standard_normal(20), rng.standard_normal(20) * 0.1, rng.standard_normal((2, 20)) * 3
    reid = np.stack([base, base + near, base + near, base + near, base + near, base + far[0], base + far[1], base])
    return _case([[0, 1, 1, 1, 1, 2, 2, 0]], xw, yw, reid, seed=6)


def wide_frame_case(deg, r=4, seed=9):
    """One frame: one detection on camera 0 and `deg` on camera 1 -- a source with exactly `deg` candidates, `deg` sources with one."""
    rng = np.random.default_rng(seed)
    n = deg + 1
    return _case([[0] + [1] * deg], rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.standard_normal((n, r)) + 0.5, node_dim=4, seed=seed)
