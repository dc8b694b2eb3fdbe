"""Radius-gated graph build on the GPU: build_graph_batch(radius=r, radius_unit=...) (gnncca_plan_frames_radius, gnncca_build_edges_radius,
gnncca_build_edges_topk_backward; csrc/graph_radius.cuh) against the numpy restatement of its definition (tests/graph_radius_oracle.py).

Bit for bit against the oracle: edge_index, edge_labels, edge_ptr / edge_ptr_dev and the ground-plane attributes (float64 operations that
IEEE rounds one way, cast to fp32).  The reid attributes are fp32 sums whose order is the kernel's: they are compared, bit for bit, with
the GPU's own dense rows at the kept positions -- "a kept edge carries the dense build's bits" -- whose own parity the dense tests pin.
Gradients: torch autograd in float64 over the same kept edges, at the criterion test_gpu_graph_topk.py uses for the capped build's gradients
(test_gpu_graph_grads.check with factor 5 on e_ref_max: e_gpu <= 5 e_ref_max + 2^-23)."""
import math

import numpy as np
import pytest
import torch

import graph_radius_oracle as gro
from test_gpu_graph_grads import check
from test_graph_grads_oracle import e_ref_max

pytestmark = pytest.mark.gpu


def build(a, req_grad=False, **kw):
    from gnn_cca_amd.graph_build import build_graph_batch
    node = torch.from_numpy(a["node_embeds_raw"]).cuda().requires_grad_(req_grad)
    reid = torch.from_numpy(a["reid_embeds_raw"]).cuda().requires_grad_(req_grad)
    b = build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid,
                          only_appearance=bool(a["only_appearance"]), only_dist=bool(a["only_dist"]), **kw)
    b._inputs = (node, reid)
    return b


def bits(t):
    return t.contiguous().view(torch.int32)


def same_batch(got, want):
    assert torch.equal(got.edge_index, want.edge_index) and torch.equal(bits(got.edge_attr), bits(want.edge_attr))
    assert torch.equal(got.edge_labels, want.edge_labels) and torch.equal(got.x, want.x) and torch.equal(got.y, want.y)
    assert got.edge_ptr == want.edge_ptr and got.node_ptr == want.node_ptr
    assert torch.equal(got.edge_ptr_dev, want.edge_ptr_dev) and torch.equal(got.node_ptr_dev, want.node_ptr_dev)
    assert torch.equal(got.reid_embeds, want.reid_embeds)


def against_oracle(a, radius, unit="ground", dense=None):
    """Builds the gated batch and compares it with the oracle's list (and with the GPU's dense rows): -> (batch, keep mask)."""
    dense = build(a) if dense is None else dense
    ei, attr, lab, keep = gro.build(a, radius, unit)
    b = build(a, radius=radius, radius_unit=unit)
    torch.cuda.synchronize()
    e = int(keep.sum())
    assert b.edge_index.shape == (2, e) and b.edge_labels.shape == (e,) and b.edge_attr.shape == (e, dense.edge_attr.shape[1])
    assert np.array_equal(b.edge_index.cpu().numpy(), ei) and np.array_equal(b.edge_labels.cpu().numpy(), lab)
    where = torch.from_numpy(np.flatnonzero(keep)).cuda()
    assert torch.equal(bits(b.edge_attr), bits(dense.edge_attr[where]))
    if not a["only_appearance"]:      # the ground-plane columns: the oracle's bits
        assert np.array_equal(b.edge_attr[:, :2].cpu().numpy().view(np.int32), np.ascontiguousarray(attr[:, :2]).view(np.int32))
    _, edge_ptr_g = gro.edge_ptrs(gro.graph_oracle.edge_list(a["id_cam"], a["graph_sizes"].tolist()), keep, a["id_cam"], a["graph_sizes"])
    assert b.edge_ptr == edge_ptr_g.tolist() and b.edge_ptr_dev.cpu().tolist() == b.edge_ptr
    assert b.node_ptr == dense.node_ptr and torch.equal(b.y, dense.y) and torch.equal(b.x, dense.x)
    return b, keep


@pytest.mark.parametrize("unit,radii,max_dist", [("ground", (5, 13), 30.0), ("max_dist", (10, 26), 0.5)])
def test_boundary_on_the_integer_lattice(unit, radii, max_dist):
    a = gro.lattice_case(max_dist=np.full(3, max_dist))
    dense = build(a)
    ei = gro.graph_oracle.edge_list(a["id_cam"], a["graph_sizes"].tolist())
    s = gro.squared_distance(a["xw"], a["yw"], ei)
    frame_of = np.repeat(np.arange(3), a["graph_sizes"])[ei[0]]
    for r, at, beyond in zip(radii, (25.0, 169.0), (26.0, 170.0)):
        _, keep = against_oracle(a, r, unit, dense)
        for f in range(3):      # every frame: a pair kept at equality, a pair dropped at the next lattice distance
            kept_at, dropped_beyond = keep[(frame_of == f) & (s == at)], keep[(frame_of == f) & (s == beyond)]
            assert kept_at.size >= 2 and kept_at.all() and dropped_beyond.size >= 2 and not dropped_beyond.any(), (r, f)


def shaped(sizes, n_cams, seed, one_camera_frame=False, **kw):
    rng = np.random.default_rng(seed)
    cams = [rng.integers(0, n_cams, s) for s in sizes]
    if one_camera_frame:
        cams[0] = np.full(sizes[0], 2)
    n = int(sum(sizes))
    return gro.case(cams, rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), seed=seed, max_dist=rng.uniform(10, 50, len(sizes)), **kw)


SHAPES = [
    # frame sizes, cameras, attribute mode, reid width
    ((1,), 1, {}, 4),
    ((2,), 2, {}, 6),
    ((63,), 3, {}, 256),
    ((64,), 4, dict(only_appearance=True), 6),
    ((65,), 2, dict(only_dist=True), 4),
    ((129,), 4, {}, 6),
    ((129,), 3, dict(only_appearance=True), 256),
    ((1, 130), 2, {}, 4),
    ((1, 130), 4, dict(only_dist=True), 256),
    ((40, 7, 65), 3, {}, 256),      # the first frame on one camera (below)
]


@pytest.mark.parametrize("sizes,n_cams,modes,reid_dim", SHAPES)
def test_shapes(sizes, n_cams, modes, reid_dim):
    a = shaped(sizes, n_cams, seed=len(sizes) * 100 + sizes[-1] + reid_dim, one_camera_frame=len(sizes) == 3, reid_dim=reid_dim, **modes)
    dense = build(a)
    for r, unit in ((6.0, "ground"), (0.25, "max_dist")):
        b, keep = against_oracle(a, r, unit, dense)
        if max(sizes) > 2 and n_cams > 1:
            assert 0 < keep.sum() < keep.size      # the gate bites
    if len(sizes) == 3:
        assert b.edge_ptr[1] == 0      # the frame whose detections share one camera has no edge


def test_extremes():
    # radius 0: coincident cross-camera points are kept, distinct ones dropped
    a = gro.case([[0, 1, 2, 0, 1]], [3.5, 3.5, 3.5, 3.5, 3.5 + 2 ** -40], [-1.25, -1.25, -1.25, -1.25, -1.25])
    b, keep = against_oracle(a, 0.0)
    assert b.edge_index.cpu().numpy().T.tolist() == [[0, 1], [0, 2], [3, 1], [3, 2], [1, 0], [1, 2], [1, 3], [2, 0], [2, 1], [2, 3]]
    # a radius that keeps nothing: E = 0, empty outputs, edge_ptr all zero, no launch error
    a = shaped((5, 9), 3, seed=4)
    b, keep = against_oracle(a, 1e-9)
    assert not keep.any() and b.edge_index.shape == (2, 0) and b.edge_attr.shape == (0, 4) and b.edge_labels.shape == (0,)
    assert b.edge_ptr == [0, 0, 0] and not b.edge_ptr_dev.any()
    torch.cuda.synchronize()
    # radius inf: the dense build, bit for bit, on every output, in both units and every mode
    for modes in ({}, dict(only_appearance=True), dict(only_dist=True)):
        a = shaped((70, 1, 12), 4, seed=5, **modes)
        dense = build(a)
        for unit in gro.UNITS:
            same_batch(build(a, radius=math.inf, radius_unit=unit), dense)
        same_batch(build(a, radius=1e30), dense)
    # one NaN and one inf position: the oracle's list
    a = shaped((12,), 3, seed=6)
    a["xw"][3], a["yw"][7] = np.nan, np.inf
    for r in (4.0, 1e150, math.inf):      # (1e150 squared is finite: it keeps every finite pair and still drops the inf position's)
        b, keep = against_oracle(a, r)
        ei = b.edge_index.cpu().numpy()
        assert not (ei == 3).any()      # every pair with the NaN position is dropped
        assert (ei == 7).any() == (r == math.inf)      # the inf position's pairs are kept by radius inf alone


_terrace = {}


def random_positions_terrace_sizes():
    """64 frames whose sizes and camera ids are the Terrace fixture's (frames of 8 to 34 detections), positions random."""
    if not _terrace:
        t = gro.terrace()
        rng = np.random.default_rng(12)
        pick = rng.choice(np.flatnonzero((t["graph_sizes"] >= 8) & (t["graph_sizes"] <= 34)), 64, replace=False)
        cams = [t["id_cam"][t["node_ptr"][q]:t["node_ptr"][q + 1]] for q in pick]
        n = sum(len(c) for c in cams)
        _terrace["a"] = gro.case(cams, rng.uniform(0, 300, n), rng.uniform(0, 300, n), seed=12, max_dist=np.full(64, 100.0))
    return _terrace["a"]


def test_closure_under_reversal():
    from gnn_cca_amd.postprocess import prune_and_cluster
    a = random_positions_terrace_sizes()
    assert len(a["graph_sizes"]) == 64 and a["graph_sizes"].min() >= 8 and a["graph_sizes"].max() <= 34
    b, keep = against_oracle(a, 80.0)
    assert 0 < keep.sum() < keep.size
    ei = b.edge_index.cpu().numpy()
    pairs = set(map(tuple, ei.T.tolist()))
    assert pairs == {(d, s) for s, d in pairs} and len(pairs) == ei.shape[1]
    post = prune_and_cluster(b.edge_index, torch.ones(ei.shape[1], dtype=torch.int64, device="cuda"), len(a["id_cam"]), b.node_ptr_dev, b.edge_ptr_dev)
    torch.cuda.synchronize()
    assert bool(post["pruned"].all())      # no active edge lacks an active reverse


def test_capture_and_replay(monkeypatch):
    """The gated build inside a HIP graph (nothing on the path synchronises), replayed with different embeddings in the static inputs."""
    from gnn_cca_amd import frames
    a = shaped((20, 33, 9), 4, seed=8)
    monkeypatch.setattr(frames, "_staging", {})      # an event recorded during a capture must not be waited on by a later, eager batch
    node = torch.from_numpy(a["node_embeds_raw"]).cuda()
    reid = torch.from_numpy(a["reid_embeds_raw"]).cuda()

    def step():
        from gnn_cca_amd.graph_build import build_graph_batch
        return build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid, radius=7.0)

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
        assert eager.edge_index.shape[1] > 0
        for g, w in zip(got, (eager.edge_index, eager.edge_attr, eager.edge_labels, eager.x)):
            assert torch.equal(g, w)


def torch_grads(a, ei, g_x, g_ea):
    """(d_node, d_reid) in float64: torch autograd through the reference's statements over the edges `ei`."""
    import torch.nn.functional as F
    node = torch.from_numpy(a["node_embeds_raw"]).double().requires_grad_()
    reid = torch.from_numpy(a["reid_embeds_raw"]).double().requires_grad_()
    x, rn = F.normalize(node, p=2, dim=0), F.normalize(reid, p=2, dim=0)
    r, c = torch.from_numpy(ei[0]), torch.from_numpy(ei[1])
    emb, cos = F.pairwise_distance(rn[r], rn[c]), F.cosine_similarity(rn[r], rn[c])
    g = torch.from_numpy(g_ea).double()
    col = 0 if a["only_appearance"] else 2
    ((x * torch.from_numpy(g_x).double()).sum() + (emb * g[:, col]).sum() + (cos * g[:, col + 1]).sum()).backward()
    return node.grad.numpy(), reid.grad.numpy()


def gpu_grads(a, g_x, g_ea, **kw):
    b = build(a, req_grad=True, **kw)
    assert b.edge_attr.shape == g_ea.shape
    torch.autograd.backward([b.x, b.edge_attr], [torch.from_numpy(g_x).cuda(), torch.from_numpy(g_ea).cuda()])
    torch.cuda.synchronize()
    node, reid = b._inputs
    return b, node.grad, reid.grad


@pytest.mark.parametrize("modes", [{}, dict(only_appearance=True)])
def test_gradients_reach_the_raw_embeddings(modes):
    a = shaped((21, 7, 70), 3, seed=9, reid_dim=36, node_dim=24, **modes)
    rng = np.random.default_rng(10)
    worst = e_ref_max()
    n_attr = 2 if modes else 4
    for r, unit in ((6.0, "ground"), (0.2, "max_dist")):
        ei, _, _, keep = gro.build(a, r, unit)
        assert 0 < keep.sum() < keep.size
        g_x = rng.standard_normal(a["node_embeds_raw"].shape).astype(np.float32)
        g_ea = rng.standard_normal((int(keep.sum()), n_attr)).astype(np.float32)
        b, d_node, d_reid = gpu_grads(a, g_x, g_ea, radius=r, radius_unit=unit)
        assert d_node is not None and d_reid is not None, "build_graph_batch(radius=...) cut the autograd chain"
        assert np.array_equal(b.edge_index.cpu().numpy(), ei)
        rn, rr = torch_grads(a, ei, g_x, g_ea)
        check(f"radius {r} {unit} {modes} d_node", d_node.cpu().numpy(), rn, worst["d_node"], factor=5)
        check(f"radius {r} {unit} {modes} d_reid", d_reid.cpu().numpy(), rr, worst["d_reid"], factor=5)
        again = gpu_grads(a, g_x, g_ea, radius=r, radius_unit=unit)
        assert torch.equal(again[1], d_node) and torch.equal(again[2], d_reid), "two runs must agree bit for bit"


def test_gradients_at_radius_inf_are_the_dense_builds_and_corner_cases():
    rng = np.random.default_rng(11)
    for modes in ({}, dict(only_appearance=True)):
        a = shaped((21, 7, 70), 3, seed=9, reid_dim=36, node_dim=24, **modes)
        e = gro.graph_oracle.edge_list(a["id_cam"], a["graph_sizes"].tolist()).shape[1]
        g_x = rng.standard_normal(a["node_embeds_raw"].shape).astype(np.float32)
        g_ea = rng.standard_normal((e, 2 if modes else 4)).astype(np.float32)
        _, dn, dr = gpu_grads(a, g_x, g_ea)
        _, dn_r, dr_r = gpu_grads(a, g_x, g_ea, radius=math.inf)
        assert torch.equal(dn, dn_r) and torch.equal(dr, dr_r), modes
    # only_dist: no attribute depends on the reid table
    a = shaped((21, 7), 3, seed=9, only_dist=True)
    keep = gro.build(a, 6.0)[3]
    _, dn, dr = gpu_grads(a, rng.standard_normal(a["node_embeds_raw"].shape).astype(np.float32),
                          rng.standard_normal((int(keep.sum()), 2)).astype(np.float32), radius=6.0)
    assert dn is not None and (dr is None or not dr.any())
    # E = 0: zero gradient on the reid table, the node gradient is the normalisation's
    a = shaped((5, 9), 3, seed=4)
    _, dn, dr = gpu_grads(a, rng.standard_normal(a["node_embeds_raw"].shape).astype(np.float32), np.zeros((0, 4), np.float32), radius=1e-9)
    assert dn is not None and dr is not None and not dr.any()
    # an input that does not require grad gets none, and the outputs carry no graph
    b = build(a, radius=6.0)
    assert b.edge_attr.grad_fn is None and not b.edge_attr.requires_grad
