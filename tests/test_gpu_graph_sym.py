"""Symmetric capped graph build on the GPU: build_graph_batch(top_k=k, rank_by=..., symmetric='union' | 'mutual')
(gnncca_build_edges_topk_sym_count / _emit; csrc/graph_topk_sym.cuh) against the numpy restatement of its definition
(tests/helpers/graph_sym_oracle.py) and against the GPU's own dense build, whose bits a kept edge must carry.

Shapes: those of test_gpu_graph_topk.py -- the golden cases (frame70: the frame spans two 64-detection chunks, so a bit row has two words;
a detection without a cross-camera partner), `degree_steps` (a frame without an edge inside a batch), `frame100` (a two-word bit row with
deg > 64), the exact-tie frame with its kept sets stated, one frame at the degree limit (4096: 65-word rows) and one above it, and a
batch without any edge.  The selections are compared exactly: no case holds a near tie (test_graph_sym_oracle.py), and the test asserts
that it skipped no source.  Gradients: the criterion and yardstick of test_gpu_graph_topk.py (e_gpu <= 5 e_ref_max + 2^-23), imported."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_graph_grads import check
from test_gpu_graph_topk import MAX_DEG, build, dense, grads, same_batch
from test_graph_grads_oracle import e_ref_max
from test_graph_sym_oracle import CASES, MODES, TIES_K1, by_source, case
from test_graph_topk_oracle import KS, RANKS, load

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import graph_sym_oracle as gso  # noqa: E402
import graph_topk_oracle as gto  # noqa: E402

pytestmark = pytest.mark.gpu


def closed_under_reversal(ei):
    have = set(map(tuple, ei.T.tolist()))
    return all((d, s) in have for s, d in have)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rank_by", RANKS)
@pytest.mark.parametrize("name", CASES)
def test_selection(name, rank_by, mode):
    a, c, full = load(name), case(name), dense(name)
    skipped = 0
    for k in KS:
        if name != "ties":      # (`ties` holds exact ties only: equal bits, decided by the destination id on both sides)
            skipped += len(gto.near_ties(c.ei, c.key[rank_by], k))
        ei_k, _, lab_k, keep = c.build(k, rank_by, mode)
        b = build(a, top_k=k, rank_by=rank_by, symmetric=mode)
        got_ei = b.edge_index.cpu().numpy()
        assert got_ei.shape == ei_k.shape, (k, got_ei.shape, ei_k.shape)
        assert np.array_equal(got_ei, ei_k), k
        assert np.array_equal(b.edge_labels.cpu().numpy(), lab_k), k
        assert closed_under_reversal(got_ei), k
        # the attributes: the GPU's own dense rows at the kept positions, bit for bit
        assert torch.equal(b.edge_attr, full.edge_attr[torch.from_numpy(np.flatnonzero(keep)).cuda()]), k
        assert b.edge_ptr == c.edge_ptr(keep).tolist() and b.edge_ptr_dev.cpu().tolist() == b.edge_ptr
        assert b.node_ptr == full.node_ptr and torch.equal(b.node_ptr_dev, full.node_ptr_dev)
        assert torch.equal(b.y, full.y) and torch.equal(b.x, full.x)
        # mutual <= D <= union, on the GPU's own directed list
        d = set(map(tuple, build(a, top_k=k, rank_by=rank_by).edge_index.cpu().numpy().T.tolist()))
        mine = set(map(tuple, got_ei.T.tolist()))
        assert mine >= d if mode == "union" else mine <= d, k
    assert skipped == 0, "a case holds a near tie (test_graph_sym_oracle.py checks that none does)"


@pytest.mark.parametrize("name", CASES)
def test_dense_equivalence(name):
    """top_k >= max deg is the dense build, bit for bit, in both modes and both ranking keys."""
    a, want = load(name), dense(name)
    for k in (int(max(gto.degrees(a).max(), 1)), 10 ** 6):
        for rank_by in RANKS:
            for mode in MODES:
                same_batch(build(a, top_k=k, rank_by=rank_by, symmetric=mode), want)


def test_stated_tie_sets():
    a = gto.ties_case()
    for rank_by in RANKS:
        for mode in MODES:
            ei = build(a, top_k=1, rank_by=rank_by, symmetric=mode).edge_index.cpu().numpy()
            assert by_source(ei) == TIES_K1[rank_by][mode], (rank_by, mode)
    # detection 0 keeps 1 and 2 at k = 2; 2 keeps 0 and 7: the pair (0, 2) becomes mutual, (0, 3) stays one-way
    for rank_by in RANKS:
        got = by_source(build(a, top_k=2, rank_by=rank_by, symmetric="mutual").edge_index.cpu().numpy())
        assert got[0] == [1, 2] and got[2][0] == 0 and 3 not in got, rank_by


def test_degree_limit():
    """One source with exactly 4096 candidates (the documented maximum; its bit row has 65 words) is closed right; 4097 is refused before
    any launch."""
    from gnn_cca_amd import _native as nat
    a = gto.wide_frame_case(MAX_DEG)
    c = gso.Case(a)
    b = build(a, top_k=3, rank_by="ground", symmetric="union")
    ei_k, _, lab_k, keep = c.build(3, "ground", "union")
    assert np.array_equal(b.edge_index.cpu().numpy(), ei_k) and np.array_equal(b.edge_labels.cpu().numpy(), lab_k)
    assert b.edge_ptr == [0, int(keep.sum())] == b.edge_ptr_dev.cpu().tolist() and int(keep.sum()) == 2 * MAX_DEG      # every detection keeps 0
    m = build(a, top_k=3, rank_by="ground", symmetric="mutual").edge_index.cpu().numpy()
    assert np.array_equal(m, c.build(3, "ground", "mutual")[0]) and m.shape[1] == 6
    over = gto.wide_frame_case(MAX_DEG + 1)
    with pytest.raises(NotImplementedError):
        build(over, top_k=3, symmetric="union")
    sizes = np.array([10], np.int64)
    fr = nat.Frames()
    st = nat.lib().gnncca_build_edges_topk_sym_count(None, None, 4, 10, sizes.ctypes.data, 1, 3, 0, MAX_DEG + 1, 1, None, 0, None, None)
    assert st == nat.ERR_INVALID_ARG      # a null frames pointer is caught first
    st = nat.lib().gnncca_build_edges_topk_sym_count(fr, None, 4, 10, sizes.ctypes.data, 1, 3, 0, MAX_DEG + 1, 1, None, 0, None, None)
    assert st == nat.ERR_UNSUPPORTED
    st = nat.lib().gnncca_build_edges_topk_sym_count(fr, None, 4, 10, sizes.ctypes.data, 1, 3, 0, 5, 3, None, 0, None, None)
    assert st == nat.ERR_INVALID_ARG      # an unknown closure
    assert nat.lib().gnncca_build_edges_topk_sym_bytes(sizes.ctypes.data, 1) == 16 * 10 + 4 * 10 + 8      # two 10-word matrices, 10 counts, to 16 B
    assert nat.lib().gnncca_build_edges_topk_sym_bytes(np.array([70, 3], np.int64).ctypes.data, 2) == 16 * (140 + 3) + 4 * 73 + 12


def test_a_batch_without_an_edge():
    """E = 0 is legal: empty tensors, no fault.  With a symmetric key the globally nearest cross-camera pair is always mutual, so a
    'mutual' result is empty exactly when the dense graph is: frames whose detections share one camera."""
    a = gto.degree_steps_case()
    n = len(a["id_cam"])
    only = {k: (v[6:8] if np.ndim(v) and len(v) == n else v) for k, v in a.items()}
    only["graph_sizes"], only["max_dist"] = np.array([1, 1], np.int64), a["max_dist"][:2]
    for mode in MODES:
        for rank_by in RANKS:
            b = build(only, top_k=2, rank_by=rank_by, symmetric=mode)
            torch.cuda.synchronize()
            assert b.edge_index.shape == (2, 0) and b.edge_attr.shape == (0, 4) and b.edge_labels.shape == (0,)
            assert b.edge_ptr == [0, 0, 0] == b.edge_ptr_dev.cpu().tolist() and b.node_ptr == [0, 1, 2]
    b = build(only, req_grad=True, top_k=2, symmetric="mutual")
    (b.x.sum() + b.edge_attr.sum()).backward()
    torch.cuda.synchronize()
    assert b._inputs[1].grad is None or not b._inputs[1].grad.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["batch3", "frame70", "camera_only", "only_appearance"])
def test_gradients_against_the_float64_oracle(name, mode):
    a, c = load(name), case(name)
    worst = e_ref_max()
    for rank_by in RANKS:
        keep = c.keep(2, rank_by, mode)
        d_node, d_reid = grads(a, keep, top_k=2, rank_by=rank_by, symmetric=mode)
        assert d_node is not None and d_reid is not None, "build_graph_batch(symmetric=...) cut the autograd chain"
        rn, rr = gto.backward(a, keep, a["g_edge_attr"][keep])
        check(f"{name} {mode} {rank_by} d_node", d_node.cpu().numpy(), rn, worst["d_node"], factor=5)
        check(f"{name} {mode} {rank_by} d_reid", d_reid.cpu().numpy(), rr, worst["d_reid"], factor=5)
        again = grads(a, keep, top_k=2, rank_by=rank_by, symmetric=mode)
        assert torch.equal(again[0], d_node) and torch.equal(again[1], d_reid), "two runs must agree bit for bit"


def test_two_runs_give_identical_bits():
    a = load("frame70")
    for mode in MODES:
        one, two = (build(a, top_k=3, rank_by="reid", symmetric=mode) for _ in range(2))
        same_batch(one, two)


def test_capture_is_refused_before_anything_is_launched(monkeypatch):
    from gnn_cca_amd import frames, graph_build as gbm
    a = load("batch3")
    node = torch.from_numpy(a["node_embeds_raw"]).cuda()
    reid = torch.from_numpy(a["reid_embeds_raw"]).cuda()
    scratch = torch.zeros(8, device="cuda")
    build(a, top_k=3, symmetric="union")      # the library and the staging ring exist
    torch.cuda.synchronize()

    def no_staging(self, nbytes):
        raise AssertionError("the refusal must come before the plan and the upload")

    monkeypatch.setattr(frames._Staging, "take", no_staging)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="captured"):
        with torch.cuda.graph(graph):
            scratch.add_(1.0)      # (the capture is not empty)
            gbm.build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid, top_k=3, symmetric="union")
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert build(a, top_k=3, symmetric="union").edge_index.shape[1] > 0      # and the eager call works afterwards
