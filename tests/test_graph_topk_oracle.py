"""Capped graph build (build_graph_batch(top_k=k)): the numpy restatement (tests/helpers/graph_topk_oracle.py) on the golden graph cases,
and the host planner's capped edge ranges (gnncca_plan_frames_ex, a HOST function of the C-ABI library) against it.  CPU only.  Home of
what test_gpu_graph_topk.py shares with it: the case list and the check that no golden case holds a near tie."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_graph_grads_oracle import load_grads

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import graph_topk_oracle as gto  # noqa: E402

GOLDEN_CASES = ["one_frame", "batch3", "interleaved", "frame70", "camera_only", "only_appearance", "only_dist"]
KS = [1, 2, 3, 8]
RANKS = ["ground", "reid"]
SYNTHETIC = ["degree_steps", "frame100"]      # tests/helpers/graph_topk_oracle.py


def load(name):
    if name == "degree_steps":
        return gto.degree_steps_case()
    if name == "frame100":
        return gto.frame100_case()
    if name == "ties":
        return gto.ties_case()
    return load_grads(name)


@pytest.mark.parametrize("name", GOLDEN_CASES + SYNTHETIC)
def test_oracle_properties(name):
    a = load(name)
    ei, attr, lab = gto.dense(a)
    deg = gto.degrees(a)
    assert int(deg.sum()) == ei.shape[1]
    for rank_by in RANKS:
        # k >= max deg: the dense arrays exactly
        for k in (int(deg.max()), 10 ** 6):
            ei_k, attr_k, lab_k, keep = gto.build(a, k, rank_by)
            assert keep.all() and np.array_equal(ei_k, ei) and np.array_equal(attr_k, attr) and np.array_equal(lab_k, lab)
        for k in KS + [4]:
            ei_k, attr_k, lab_k, keep = gto.build(a, k, rank_by)
            assert ei_k.shape[1] == int(np.minimum(deg, k).sum()) == int(gto.edge_ptr(a, k)[-1])      # E == sum min(k, deg)
            assert np.array_equal(ei_k, ei[:, keep]) and np.array_equal(attr_k, attr[keep])              # a subsequence of the dense list
            assert np.array_equal(np.bincount(ei_k[0], minlength=len(deg)), np.minimum(deg, k))
            if k == 1:                                                                                     # one edge per non-isolated source
                assert np.array_equal(np.sort(ei_k[0]), np.flatnonzero(deg > 0))
            # every kept edge's key is <= every dropped edge's key of the same source
            key = gto.keys(a, ei, rank_by)
            for s0, s1 in gto.segments(ei):
                kept, dropped = key[s0:s1][keep[s0:s1]], key[s0:s1][~keep[s0:s1]]
                assert dropped.size == 0 or kept.max() <= dropped.min()


def test_degree_steps_case_has_the_degrees_it_promises():
    a = gto.degree_steps_case()
    deg = gto.degrees(a)
    assert deg[:6].tolist() == [3, 3, 3, 4, 4, 5] and deg[6:8].tolist() == [0, 0]
    assert {3, 4, 5} <= set(deg.tolist())      # with k = 4: deg < k, deg == k, deg == k + 1
    assert gto.degrees(gto.frame100_case()).min() > 64


def test_ties_go_to_the_smaller_destination_id():
    a = gto.ties_case()
    for rank_by in RANKS:
        ei, _, _ = gto.dense(a)
        key = gto.keys(a, ei, rank_by)
        from0 = ei[0] == 0
        assert np.unique(key[from0 & (ei[1] <= 4)]).size == 1, "detections 1 .. 4 must tie exactly as candidates of detection 0"
        assert key[from0 & (ei[1] > 4)].min() > key[from0 & (ei[1] <= 4)].max()
        for k, want in ((1, [1]), (2, [1, 2]), (3, [1, 2, 3]), (4, [1, 2, 3, 4])):
            ei_k = gto.build(a, k, rank_by)[0]
            assert ei_k[1][ei_k[0] == 0].tolist() == want, (rank_by, k)
        ei_1 = gto.build(a, 1, rank_by)[0]
        for src in (1, 2, 3, 4):   # detections 0 and 7 tie as their candidates
            assert ei_1[1][ei_1[0] == src].tolist() == [0]


@pytest.mark.parametrize("name", GOLDEN_CASES + SYNTHETIC)
def test_no_case_holds_a_near_tie(name):
    """test_gpu_graph_topk.py compares selections exactly; it may skip a source whose k-th and (k+1)-th keys are within 1e-6 relative
    (a last-ulp difference between the GPU's and this oracle's key could flip it) -- and asserts that it skipped none.  Checked here."""
    a = load(name)
    ei, _, _ = gto.dense(a)
    for rank_by in RANKS:
        key = gto.keys(a, ei, rank_by)
        for k in KS + [4]:
            assert gto.near_ties(ei, key, k) == [], (name, rank_by, k)


def _native_capped_plan(a, k):
    """gnncca_plan_frames_ex -> (E, edge_ptr [N + 1], edge_ptr_g [G + 1], src_order, max_deg) of its staging image."""
    import ctypes as C

    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    xw, yw, md = (np.ascontiguousarray(a[v], np.float64) for v in ("xw", "yw", "max_dist"))
    ids, cams, sizes = (np.ascontiguousarray(a[v], np.int64) for v in ("id", "id_cam", "graph_sizes"))
    n, g = len(cams), len(sizes)
    nbytes = lib.gnncca_plan_frames_bytes(n, g)
    buf = np.full(nbytes + 16, 0xAB, np.uint8)
    max_deg = C.c_int32(-1)
    e = lib.gnncca_plan_frames_ex(xw.ctypes.data, yw.ctypes.data, ids.ctypes.data, cams.ctypes.data, n, sizes.ctypes.data, md.ctypes.data, g, k,
                                  buf.ctypes.data, nbytes, C.byref(max_deg))
    assert np.all(buf[nbytes:] == 0xAB), "wrote beyond the size it asked for"
    i32 = buf[8 * (3 * n + g):nbytes].view(np.int32)
    return (int(e), i32[4 * n + g + 1:5 * n + g + 2].copy(), i32[5 * n + g + 2:5 * n + 2 * g + 3].copy(), i32[3 * n + g + 1:4 * n + g + 1].copy(),
            max_deg.value, buf[:nbytes].copy())


@pytest.mark.parametrize("name", GOLDEN_CASES + SYNTHETIC)
def test_native_capped_plan_matches_the_oracle_counts(name):
    from gnn_cca_amd import _native as nat
    a = load(name)
    deg = gto.degrees(a)
    for k in KS + [4, int(max(deg.max(), 1)), 10 ** 6]:
        e, edge_ptr, edge_ptr_g, src_order, max_deg, _ = _native_capped_plan(a, k)
        want = np.minimum(deg, k)[src_order]
        assert e == int(want.sum()) and max_deg == int(deg.max())
        assert np.array_equal(edge_ptr, np.concatenate([[0], np.cumsum(want)]))
        assert np.array_equal(edge_ptr_g, gto.edge_ptr(a, k))
    # top_k == 0 is gnncca_plan_frames, byte for byte; a negative cap is refused
    lib = nat.lib()
    xw, yw, md = (np.ascontiguousarray(a[v], np.float64) for v in ("xw", "yw", "max_dist"))
    ids, cams, sizes = (np.ascontiguousarray(a[v], np.int64) for v in ("id", "id_cam", "graph_sizes"))
    n, g = len(cams), len(sizes)
    nbytes = lib.gnncca_plan_frames_bytes(n, g)
    buf = np.zeros(nbytes, np.uint8)
    e0 = lib.gnncca_plan_frames(xw.ctypes.data, yw.ctypes.data, ids.ctypes.data, cams.ctypes.data, n, sizes.ctypes.data, md.ctypes.data, g,
                                buf.ctypes.data, nbytes)
    e, _, _, _, _, image = _native_capped_plan(a, 0)
    assert e == e0 == int(deg.sum()) and np.array_equal(image, buf)
    assert _native_capped_plan(a, -1)[0] == -nat.ERR_INVALID_ARG
