"""Numpy restatement of the radius-gated graph build (build_graph_batch(radius=r, radius_unit=...)), written from its definition in
include/gnncca_mpn.h, not from the kernel or the host plan.  TEST INFRASTRUCTURE.

Definition: take the dense build's edge list (oracle.graph_oracle.edge_list: the reference's complete cross-camera graph); for the
edge (i, j) of frame g
    dx = xw[i] - xw[j];  dy = yw[i] - yw[j];  a = dx * dx;  b = dy * dy;  s = a + b          (float64, every operation rounded once)
    t  = radius ('ground')  or  radius * max_dist[g] ('max_dist', one rounded product);  t2 = t * t
keep it iff s <= t2 (a NaN compares false).  The kept edges stay in the dense order.  Each numpy statement below is one IEEE operation
per element with its own rounding: numpy never fuses two ufunc calls.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import graph_oracle  # noqa: E402

UNITS = ("ground", "max_dist")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def squared_distance(xw, yw, ei):
    """s of every edge: float64 [E], two products and one sum, each rounded once."""
    xw, yw = np.asarray(xw, np.float64), np.asarray(yw, np.float64)
    r, c = ei
    with np.errstate(invalid="ignore", over="ignore"):
        dx = xw[r] - xw[c]
        dy = yw[r] - yw[c]
        a = dx * dx
        b = dy * dy
        return a + b


def threshold2(radius, unit, max_dist):
    """t2 per frame: float64 [G]."""
    md = np.asarray(max_dist, np.float64)
    if unit not in UNITS:
        raise ValueError(unit)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.full(md.shape, np.float64(radius)) if unit == "ground" else np.float64(radius) * md
        return t * t


def keep_mask(xw, yw, id_cam, graph_sizes, max_dist, radius, unit="ground", ei=None):
    """(dense edge_index [2, E], keep bool [E])."""
    sizes = np.asarray(graph_sizes, np.int64)
    if ei is None:
        ei = graph_oracle.edge_list(np.asarray(id_cam), sizes.tolist()) if len(sizes) else np.zeros((2, 0), np.int64)
    graph_of = np.repeat(np.arange(len(sizes)), sizes)
    s = squared_distance(xw, yw, ei)
    t2 = threshold2(radius, unit, max_dist)[graph_of[ei[0]]] if ei.shape[1] else np.zeros(0)
    with np.errstate(invalid="ignore"):
        keep = s <= t2
    return ei, keep


def edge_ptrs(ei, keep, id_cam, graph_sizes):
    """(edge_ptr [N + 1] by source POSITION -- sources in the order the dense list emits them: frame-major, cameras in ascending id
    inside a frame, node id ascending inside a camera -- and edge_ptr_g [G + 1]) of the kept list."""
    sizes = np.asarray(graph_sizes, np.int64)
    n = int(sizes.sum())
    cams = np.asarray(id_cam, np.int64)
    graph_of = np.repeat(np.arange(len(sizes)), sizes)
    order = np.lexsort((np.arange(n), cams, graph_of))          # position -> node id
    per_node = np.bincount(ei[0][keep], minlength=n).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum(per_node[order])])
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    per_frame = np.array([per_node[node_ptr[g]:node_ptr[g + 1]].sum() for g in range(len(sizes))], np.int64)
    return edge_ptr, np.concatenate([[0], np.cumsum(per_frame)])


def build(a, radius, unit="ground", reid_n=None):
    """(edge_index, edge_attr, edge_labels, keep) of the gated build of a fixture-shaped dict; `keep` masks the dense edge list."""
    if reid_n is None:
        reid_n = graph_oracle.normalize_columns(a["reid_embeds_raw"])
    ei, attr, lab = graph_oracle.build(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], reid_n,
                                       bool(a.get("only_appearance", False)), bool(a.get("only_dist", False)))
    _, keep = keep_mask(a["xw"], a["yw"], a["id_cam"], a["graph_sizes"], a["max_dist"], radius, unit, ei=ei)
    return ei[:, keep], attr[keep], lab[keep], keep


# ---- the Terrace fixture (tests/golden/terrace_geometry.npz) and the cases the CPU and the GPU tests share ----
def terrace(first=None):
    """The fixture's arrays, optionally its first `first` frames: dict(frame, node_ptr, id_cam, id, xw, yw, graph_sizes)."""
    z = np.load(os.path.join(GOLDEN, "terrace_geometry.npz"))
    g = len(z["frame"]) if first is None else first
    ptr = z["node_ptr"][:g + 1].astype(np.int64)
    n = int(ptr[-1])
    return dict(frame=z["frame"][:g], node_ptr=ptr, graph_sizes=np.diff(ptr), id_cam=z["cam"][:n].astype(np.int64), id=z["person"][:n].astype(np.int64),
                xw=z["xw"][:n].astype(np.float64), yw=z["yw"][:n].astype(np.float64))


def with_embeddings(a, reid_dim=16, node_dim=8, seed=0, max_dist=None, **modes):
    """A fixture-shaped dict made complete for build(): synthetic embeddings (the repository holds no image), max_dist, the mode flags."""
    rng = np.random.default_rng(seed)
    n, g = len(a["id_cam"]), len(a["graph_sizes"])
    out = dict(a)
    out["max_dist"] = np.full(g, 20.0) if max_dist is None else np.asarray(max_dist, np.float64)
    out["reid_embeds_raw"] = (rng.standard_normal((n, reid_dim)) + 0.5).astype(np.float32)
    out["node_embeds_raw"] = rng.standard_normal((n, node_dim)).astype(np.float32)
    out["only_appearance"], out["only_dist"] = bool(modes.get("only_appearance", False)), bool(modes.get("only_dist", False))
    return out


def case(cams, xw, yw, ids=None, seed=0, **kw):
    """A batch from per-frame camera lists and concatenated positions."""
    rng = np.random.default_rng(seed)
    id_cam = np.concatenate([np.asarray(c, np.int64) for c in cams]) if cams else np.zeros(0, np.int64)
    n = len(id_cam)
    a = dict(graph_sizes=np.array([len(c) for c in cams], np.int64), id_cam=id_cam, id=rng.integers(0, 5, n) if ids is None else np.asarray(ids, np.int64),
             xw=np.asarray(xw, np.float64), yw=np.asarray(yw, np.float64))
    return with_embeddings(a, seed=seed, **kw)


LATTICE_OFFSETS = [(3, 4), (4, 3), (-3, 4), (5, 12), (12, 5), (-5, 12), (0, 5), (0, 13), (5, 0), (13, 0), (5, 1), (1, 5), (4, 4), (6, 0), (12, 6), (13, 1), (1, 13), (9, 10)]


def lattice_case(**kw):
    """Frames on an integer lattice.  Frame f: an anchor on camera 0 at an integer point and eighteen detections on cameras 1 .. 3 at the
    offsets above from it -- |offset|^2 is 25 (3-4-5, kept at equality by radius 5), 169 (5-12-13, kept at equality by radius 13), or the
    next lattice value (26 = 5^2 + 1^2 above 25, 170 = 13^2 + 1^2 above 169: dropped) and beyond.  Three frames with different anchors.  In the 'max_dist' unit
    max_dist = 0.5 with radius 10 (26) gives the same t = 5 (13)."""
    cams, xs, ys = [], [], []
    for ax, ay in ((0, 0), (7, -3), (-100, 250)):
        cams.append([0] + [1 + k % 3 for k in range(len(LATTICE_OFFSETS))])
        xs += [ax] + [ax + dx for dx, _ in LATTICE_OFFSETS]
        ys += [ay] + [ay + dy for _, dy in LATTICE_OFFSETS]
    return case(cams, xs, ys, **kw)


def recall_table(a, radii):
    """([(radius, kept edges, kept same-identity edges)], E, same-identity edges, largest same-identity distance) of a geometry dict, in
    ground units."""
    ei, _ = keep_mask(a["xw"], a["yw"], a["id_cam"], a["graph_sizes"], np.ones(len(a["graph_sizes"])), np.inf)
    pos = np.asarray(a["id"])[ei[0]] == np.asarray(a["id"])[ei[1]]
    s = squared_distance(a["xw"], a["yw"], ei)
    out = []
    for r in radii:
        keep = s <= np.float64(r) * np.float64(r)
        out.append((r, int(keep.sum()), int((keep & pos).sum())))
    return out, int(pos.size), int(pos.sum()), float(np.sqrt(s[pos].max()))
