"""Capped graph build on the GPU: build_graph_batch(top_k=k, rank_by=...) (gnncca_plan_frames_ex, gnncca_build_edges_topk,
gnncca_build_edges_topk_backward; csrc/graph_topk.cuh) against the numpy restatement of its definition
(tests/helpers/graph_topk_oracle.py) and against the GPU's own dense build, whose bits a kept edge must carry.

Shapes: the golden cases (a 70-detection frame: the frame spans two 64-detection chunks; a detection without a cross-camera partner)
plus `degree_steps` (deg 3, 4, 5 against k = 4; a camera of one detection; a frame with no edge), `frame100` (deg 66 / 67: a source's
candidates fill more than one 64-slot chunk), an exact-tie frame, and one frame at the documented degree limit (4096) and one just above.
Gradients: the criterion and the yardstick of test_gpu_graph_grads.py for shapes without a fixture (e_gpu <= 5 e_ref_max + 2^-23),
read from that file -- the same arithmetic on fewer edges.
"""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from test_gpu_graph_grads import check
from test_graph_grads_oracle import e_ref_max
from test_graph_topk_oracle import GOLDEN_CASES, KS, RANKS, SYNTHETIC, load

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import graph_topk_oracle as gto  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_DEG = 4096


def build(a, req_grad=False, **kw):
    from gnn_cca_amd.graph_build import build_graph_batch
    node = torch.from_numpy(a["node_embeds_raw"]).cuda().requires_grad_(req_grad)
    reid = torch.from_numpy(a["reid_embeds_raw"]).cuda().requires_grad_(req_grad)
    b = build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid,
                          only_appearance=bool(a["only_appearance"]), only_dist=bool(a["only_dist"]), **kw)
    b._inputs = (node, reid)
    return b


_dense = {}


def dense(name):
    """The GPU's dense build of a case, computed once and left unchanged."""
    if name not in _dense:
        _dense[name] = build(load(name))
        torch.cuda.synchronize()
    return _dense[name]


def same_batch(got, want):
    assert torch.equal(got.edge_index, want.edge_index) and torch.equal(got.edge_attr, want.edge_attr)
    assert torch.equal(got.edge_labels, want.edge_labels) and torch.equal(got.x, want.x) and torch.equal(got.y, want.y)
    assert got.edge_ptr == want.edge_ptr and got.node_ptr == want.node_ptr
    assert torch.equal(got.edge_ptr_dev, want.edge_ptr_dev) and torch.equal(got.node_ptr_dev, want.node_ptr_dev)


@pytest.mark.parametrize("name", GOLDEN_CASES + SYNTHETIC + ["ties"])
def test_dense_equivalence(name):
    """top_k >= max deg is the dense build, bit for bit, in both ranking modes."""
    a, want = load(name), dense(name)
    for k in (int(max(gto.degrees(a).max(), 1)), 10 ** 6):
        for rank_by in RANKS:
            same_batch(build(a, top_k=k, rank_by=rank_by), want)


@pytest.mark.parametrize("rank_by", RANKS)
@pytest.mark.parametrize("name", GOLDEN_CASES + SYNTHETIC)
def test_selection(name, rank_by):
    a, full = load(name), dense(name)
    ei, _, _ = gto.dense(a)
    key = gto.keys(a, ei, rank_by)
    skipped = 0
    for k in KS + [4]:
        near = set(gto.near_ties(ei, key, k))      # sources a last-ulp key difference could flip: compared only if there are none
        skipped += len(near)
        ei_k, _, lab_k, keep = gto.build(a, k, rank_by)
        b = build(a, top_k=k, rank_by=rank_by)
        got_ei = b.edge_index.cpu().numpy()
        assert got_ei.shape == ei_k.shape, (k, got_ei.shape, ei_k.shape)
        use = ~np.isin(ei_k[0], list(near))
        assert np.array_equal(got_ei[:, use], ei_k[:, use]), k
        assert np.array_equal(b.edge_labels.cpu().numpy()[use], lab_k[use]), k
        # the attributes: the GPU's own dense rows at the kept positions, bit for bit
        want_attr = full.edge_attr[torch.from_numpy(np.flatnonzero(keep)).cuda()]
        assert torch.equal(b.edge_attr[torch.from_numpy(use).cuda()], want_attr[torch.from_numpy(use).cuda()]), k
        assert b.edge_ptr == gto.edge_ptr(a, k).tolist() and b.edge_ptr_dev.cpu().tolist() == b.edge_ptr
        assert b.node_ptr == full.node_ptr and torch.equal(b.y, full.y) and torch.equal(b.x, full.x)
    assert skipped == 0, "a case holds a near tie (test_graph_topk_oracle.py checks that none does)"


def test_ties_go_to_the_smaller_destination_id():
    a = gto.ties_case()
    for rank_by in RANKS:
        for k, want in ((1, [1]), (2, [1, 2]), (3, [1, 2, 3]), (4, [1, 2, 3, 4])):
            ei = build(a, top_k=k, rank_by=rank_by).edge_index.cpu().numpy()
            assert ei[1][ei[0] == 0].tolist() == want, (rank_by, k)
        ei = build(a, top_k=1, rank_by=rank_by).edge_index.cpu().numpy()
        for src in (1, 2, 3, 4):      # detections 0 and 7 tie as their candidates
            assert ei[1][ei[0] == src].tolist() == [0], (rank_by, src)
    # ground keys are float64 on both sides: the whole selection is the oracle's, ties included
    for k in (1, 2, 3):
        assert np.array_equal(build(a, top_k=k).edge_index.cpu().numpy(), gto.build(a, k, "ground")[0])


def test_degree_limit():
    """One source with exactly 4096 candidates (the documented maximum) is selected right; 4097 is refused before any launch."""
    from gnn_cca_amd import _native as nat
    a = gto.wide_frame_case(MAX_DEG)
    for k in (3, 100):
        b = build(a, top_k=k, rank_by="ground")
        ei_k, _, lab_k, _ = gto.build(a, k, "ground")
        assert np.array_equal(b.edge_index.cpu().numpy(), ei_k) and np.array_equal(b.edge_labels.cpu().numpy(), lab_k)
    same_batch(build(a, top_k=MAX_DEG, rank_by="reid"), build(a))
    over = gto.wide_frame_case(MAX_DEG + 1)
    with pytest.raises(NotImplementedError):
        build(over, top_k=3)
    st = nat.lib().gnncca_build_edges_topk(None, None, 4, 10, 10, 0, 3, 0, MAX_DEG + 1, None, None, None, None)
    assert st == nat.ERR_INVALID_ARG      # a null frames pointer is caught first
    fr = nat.Frames()
    st = nat.lib().gnncca_build_edges_topk(fr, None, 4, 10, 10, 0, 3, 0, MAX_DEG + 1, None, None, None, None)
    assert st == nat.ERR_UNSUPPORTED
    assert build(over).edge_index.shape[1] == 2 * (MAX_DEG + 1)      # the dense build has no such limit


def grads(a, keep, **kw):
    b = build(a, req_grad=True, **kw)
    g_ea = torch.from_numpy(np.ascontiguousarray(a["g_edge_attr"][keep])).cuda()
    torch.autograd.backward([b.x, b.edge_attr], [torch.from_numpy(a["g_x"]).cuda(), g_ea])
    torch.cuda.synchronize()
    node, reid = b._inputs
    return node.grad, reid.grad


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("name", ["batch3", "frame70", "camera_only", "only_appearance"])
def test_gradients_against_the_float64_oracle(name, k):
    a = load(name)
    worst = e_ref_max()
    for rank_by in RANKS:
        keep = gto.build(a, k, rank_by)[3]
        d_node, d_reid = grads(a, keep, top_k=k, rank_by=rank_by)
        assert d_node is not None and d_reid is not None, "build_graph_batch(top_k=...) cut the autograd chain"
        rn, rr = gto.backward(a, keep, a["g_edge_attr"][keep])
        check(f"{name} k={k} {rank_by} d_node", d_node.cpu().numpy(), rn, worst["d_node"], factor=5)
        check(f"{name} k={k} {rank_by} d_reid", d_reid.cpu().numpy(), rr, worst["d_reid"], factor=5)
        again = grads(a, keep, top_k=k, rank_by=rank_by)
        assert torch.equal(again[0], d_node) and torch.equal(again[1], d_reid), "two runs must agree bit for bit"


def test_gradients_only_dist_and_dense_equivalence():
    a = load("only_dist")
    keep = gto.build(a, 2, "reid")[3]
    d_node, d_reid = grads(a, keep, top_k=2, rank_by="reid")
    assert d_node is not None and (d_reid is None or not d_reid.any())      # as the dense path: no attribute depends on the reid table
    for name in ("batch3", "frame70", "only_appearance"):
        a = load(name)
        everything = np.ones(a["g_edge_attr"].shape[0], dtype=bool)
        dn, dr = grads(a, everything)
        dn_k, dr_k = grads(a, everything, top_k=int(gto.degrees(a).max()))
        assert torch.equal(dn, dn_k) and torch.equal(dr, dr_k), name
    # an input that does not require grad gets none, and the outputs carry no graph
    b = build(load("batch3"), top_k=3)
    assert b.edge_attr.grad_fn is None and not b.edge_attr.requires_grad


def test_downstream_mpn_postprocess_evaluation():
    """The capped batch is an ordinary graph to the rest of the stack."""
    from gnn_cca_amd import MOTMPNet, postprocess
    from gnn_cca_amd.evaluation import evaluate_frames
    from oracle.mpn_oracle import load_case
    a = dict(load("batch3"))
    params, arch, sd, _ = load_case(os.path.join(GOLDEN_DIR, "n8_sum.npz"))      # node_in 64 weights
    n = len(a["id_cam"])
    a["node_embeds_raw"] = np.random.default_rng(5).standard_normal((n, 64)).astype(np.float32)
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda()
    b = build(a, top_k=3)
    e_k = int(np.minimum(gto.degrees(a), 3).sum())
    assert b.edge_index.shape == (2, e_k)
    plain = types.SimpleNamespace(x=b.x.clone(), edge_index=b.edge_index.clone(), edge_attr=b.edge_attr.clone())
    for train in (False, True):
        m.train(train)
        with torch.no_grad():
            out, ref = m(b)["classified_edges"], m(plain)["classified_edges"]
        for o, r in zip(out, ref):
            assert o.shape == (e_k, 1) and torch.isfinite(o).all() and torch.equal(o, r)
    m.eval()
    with torch.no_grad():
        logits = m(b)["classified_edges"][-1]
    _, preds = postprocess.threshold(logits)
    post = postprocess.prune_and_cluster(b.edge_index, preds, n, b.node_ptr_dev, b.edge_ptr_dev)
    rows = evaluate_frames(b, post["pruned"], post["labels"])
    torch.cuda.synchronize()
    assert post["pruned"].shape == (e_k,) and rows.shape == (len(a["graph_sizes"]), 16)
    # a directed graph: pruning keeps an active edge only where its reverse was kept (and is active) too
    ei, pruned = b.edge_index.cpu().numpy(), post["pruned"].cpu().numpy().astype(bool)
    have = set(map(tuple, ei.T.tolist()))
    assert all((d, s) in have for s, d in ei.T[pruned].tolist())


def test_capture_and_replay(monkeypatch):
    """The capped build inside a HIP graph (nothing on the path synchronises), replayed with different embeddings in the static inputs."""
    from gnn_cca_amd import frames, graph_build as gbm
    a = load("batch3")
    monkeypatch.setattr(frames, "_staging", {})      # an event recorded during a capture must not be waited on by a later, eager batch
    node = torch.from_numpy(a["node_embeds_raw"]).cuda()
    reid = torch.from_numpy(a["reid_embeds_raw"]).cuda()

    def step():
        return gbm.build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid, top_k=3, rank_by="reid")

    for _ in range(frames._Staging.SLOTS):      # every slot of the ring gets its pinned buffer and event outside the capture
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        reid.copy_(torch.randn(reid.shape, generator=gen) + 0.5)
        node.copy_(torch.randn(node.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (static.edge_index, static.edge_attr, static.edge_labels, static.x)]
        eager = step()
        torch.cuda.synchronize()
        for g, w in zip(got, (eager.edge_index, eager.edge_attr, eager.edge_labels, eager.x)):
            assert torch.equal(g, w)


def test_argument_errors_raise_before_any_launch():
    a = load("one_frame")
    for bad in (0, -1, 2.0, 2.5, "3", True):
        with pytest.raises(ValueError):
            build(a, top_k=bad)
    with pytest.raises(ValueError):
        build(a, top_k=2, rank_by="cosine")
    with pytest.raises(ValueError):
        build(a, rank_by="cosine")
    assert build(a, top_k=np.int64(2)).edge_index.shape[1] == int(np.minimum(gto.degrees(a), 2).sum())
