"""Backward of row N1 on the GPU: gradients of build_graph_batch / normalize_columns with respect to the RAW embeddings
(gnncca_build_edges_backward, gnncca_normalize_columns_backward; csrc/graph_grads.cuh) against torch autograd through the reference's own
statements (tests/golden/graph_grads/*.npz: fp32 and fp64 runs) and, at shapes without a fixture, against the numpy restatement in fp64.

Criterion (the project's, test_gpu_input_grads.py): e(t) = max|t - t64| / max|t64|; the GPU must satisfy e_gpu <= 4 e_ref + 2^-23 with
e_ref the reference's own fp32 run against its fp64 run (two fp32 evaluations with different summation orders each sit about e_ref from
the truth).  Shapes without a fixture: e_gpu <= 5 e_ref_max + 2^-23, e_ref_max the largest e_ref over the fixtures.  Every test prints
its figures before it asserts.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_graph_grads_oracle import CASES, e_ref_max, load_grads
from test_input_grads_oracle import EPS, rel_err

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import graph_grad_oracle as ggo  # noqa: E402

pytestmark = pytest.mark.gpu


def run(a, req_node=True, req_reid=True, normalize=True, no_grad=False):
    """One build + backward with the fixture's upstream gradients: (batch, d_node, d_reid) -- the latter two numpy or None."""
    from gnn_cca_amd.graph_build import build_graph_batch
    node = torch.from_numpy(a["node_embeds_raw"]).cuda().requires_grad_(req_node)
    reid = torch.from_numpy(a["reid_embeds_raw"]).cuda().requires_grad_(req_reid)
    kw = dict(only_appearance=bool(a["only_appearance"]), only_dist=bool(a["only_dist"]), normalize=normalize)
    if no_grad:
        with torch.no_grad():
            return build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid, **kw), None, None
    b = build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid, **kw)
    pairs = [(b.x, a["g_x"]), (b.edge_attr, a["g_edge_attr"])] + ([(b.reid_embeds, a["g_reid"])] if "g_reid" in a else [])
    pairs = [(t, torch.from_numpy(np.asarray(g)).cuda()) for t, g in pairs if t.requires_grad]
    if pairs:
        torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
    torch.cuda.synchronize()
    g = lambda t: None if t.grad is None else t.grad.cpu().numpy()
    return b, g(node), g(reid)


def check(what, got, ref64, e_ref, factor=4):
    e_gpu, bound = rel_err(got, ref64), factor * e_ref + EPS
    print(f"{what}: e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  e_gpu / e_ref {e_gpu / e_ref if e_ref > 0 else float('nan'):.2f}  ratio to bound {e_gpu / bound:.3f}")
    assert np.isfinite(got).all() and e_gpu <= bound, (what, e_gpu, e_ref)


@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(name):
    a = load_grads(name)
    b, d_node, d_reid = run(a)
    assert d_node is not None, "node_embeds.grad missing: build_graph_batch cut the autograd chain"
    assert np.array_equal(b.edge_index.cpu().numpy(), a["edge_index"])
    assert d_node.shape == a["d_node64"].shape
    check(f"{name} d_node", d_node, a["d_node64"], rel_err(a["d_node32"], a["d_node64"]))
    if bool(a["only_dist"]):   # no edge attribute depends on the reid table: no gradient (None) or exactly zero
        assert d_reid is None or not d_reid.any()
        return
    assert d_reid is not None, "reid_embeds.grad missing: build_graph_batch cut the autograd chain"
    check(f"{name} d_reid", d_reid, a["d_reid64"], rel_err(a["d_reid32"], a["d_reid64"]))


def test_normalize_columns_beyond_4096_rows_and_two_matrices():
    """4100 x 16 alone (the three-kernel form), and two matrices in one call (the one-launch form; 77 x 2048 and 77 x 20)."""
    from gnn_cca_amd.graph_build import normalize_columns
    worst = e_ref_max()["d_node"]
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((4100, 16), generator=gen) + 0.3
    gy = torch.randn((4100, 16), generator=gen)
    xg = x.cuda().requires_grad_()
    normalize_columns(xg).backward(gy.cuda())
    assert xg.grad is not None, "normalize_columns cut the autograd chain"
    check("4100 x 16", xg.grad.cpu().numpy(), ggo.normalize_backward(x.numpy(), gy.numpy(), np.float64), worst, factor=5)
    a, b = torch.randn((77, 2048), generator=gen) + 0.3, torch.randn((77, 20), generator=gen)
    ga, gb = torch.randn((77, 2048), generator=gen), torch.randn((77, 20), generator=gen)
    ag, bg = a.cuda().requires_grad_(), b.cuda().requires_grad_()
    ya, yb = normalize_columns(ag, bg)
    torch.autograd.backward([ya, yb], [ga.cuda(), gb.cuda()])
    check("77 x 2048 (pair)", ag.grad.cpu().numpy(), ggo.normalize_backward(a.numpy(), ga.numpy(), np.float64), worst, factor=5)
    check("77 x 20 (pair)", bg.grad.cpu().numpy(), ggo.normalize_backward(b.numpy(), gb.numpy(), np.float64), worst, factor=5)
    # one of the pair alone: the other's .grad stays None, the same bits
    a2, b2 = a.cuda().requires_grad_(), b.cuda()
    ya2, _ = normalize_columns(a2, b2)
    ya2.backward(ga.cuda())
    assert b2.grad is None and torch.equal(a2.grad, ag.grad)


def synthetic(sizes_cams, r, d, seed, **modes):
    rng = np.random.default_rng(seed)
    id_cam = np.concatenate([np.asarray(c) for c in sizes_cams])
    n = len(id_cam)
    sizes = np.array([len(c) for c in sizes_cams], dtype=np.int64)
    a = dict(graph_sizes=sizes, id_cam=id_cam.astype(np.int64), id=rng.integers(0, 6, n), xw=rng.uniform(-8, 8, n), yw=rng.uniform(-8, 8, n),
             max_dist=rng.uniform(10, 50, len(sizes)), node_embeds_raw=rng.standard_normal((n, d)).astype(np.float32),
             reid_embeds_raw=(rng.standard_normal((n, r)) + 0.5).astype(np.float32),
             only_appearance=np.bool_(modes.get("only_appearance", False)), only_dist=np.bool_(modes.get("only_dist", False)))
    e = int(sum(len(c) ** 2 - (np.bincount(np.asarray(c)) ** 2).sum() for c in sizes_cams))
    a["g_x"] = rng.standard_normal((n, d)).astype(np.float32)
    a["g_edge_attr"] = rng.standard_normal((e, 2 if (a["only_appearance"] or a["only_dist"]) else 4)).astype(np.float32)
    return a


THREE_FRAMES = [[0] * 7 + [1] * 6 + [2] * 8, [0, 1, 2, 1, 0, 2, 2], [1] * 9 + [3] * 10]   # 21 + 7 + 19 nodes: tiles straddle frames


def test_three_frames_r2048_against_oracle():
    a = synthetic(THREE_FRAMES, 2048, 24, 11)
    _, d_node, d_reid = run(a)
    assert d_node is not None and d_reid is not None
    rn, rr = ggo.graph_build_backward(a, np.float64)
    worst = e_ref_max()
    check("3 frames R=2048 d_node", d_node, rn, worst["d_node"], factor=5)
    check("3 frames R=2048 d_reid", d_reid, rr, worst["d_reid"], factor=5)


def test_normalize_false_against_oracle():
    a = synthetic(THREE_FRAMES, 36, 8, 12)
    _, d_node, d_reid = run(a, normalize=False)
    assert d_node is not None and d_reid is not None
    rn, rr = ggo.graph_build_backward(a, np.float64, normalize_inputs=False)
    assert np.array_equal(d_node, a["g_x"])      # x is the caller's tensor: the identity
    check("normalize=False d_reid", d_reid, rr, e_ref_max()["d_reid"], factor=5)


def test_one_input_alone_gets_the_same_bits():
    a = load_grads("batch3")
    _, dn, dr = run(a)
    _, dn_only, none_r = run(a, req_reid=False)
    _, none_n, dr_only = run(a, req_node=False)
    assert dn is not None and dr is not None
    assert none_r is None and none_n is None
    assert np.array_equal(dn_only, dn) and np.array_equal(dr_only, dr)


def test_no_grad_path_is_unchanged():
    a = load_grads("terrace32")
    bg, _, _ = run(a)
    assert bg.x.grad_fn is not None and bg.edge_attr.grad_fn is not None and bg.reid_embeds.grad_fn is not None
    for kw in (dict(no_grad=True), dict(req_node=False, req_reid=False)):
        b, _, _ = run(a, **kw)
        for name in ("x", "edge_attr", "reid_embeds", "edge_index", "edge_labels"):
            t = getattr(b, name)
            assert t.grad_fn is None and not t.requires_grad, name
            assert torch.equal(t, getattr(bg, name).detach()), name
    assert not bg.edge_index.requires_grad and not bg.edge_labels.requires_grad and not bg.y.requires_grad


def test_backward_is_deterministic():
    a = load_grads("frame70")
    _, dn1, dr1 = run(a)
    _, dn2, dr2 = run(a)
    assert dn1 is not None and dr1 is not None
    assert np.array_equal(dn1.view(np.uint32), dn2.view(np.uint32)) and np.array_equal(dr1.view(np.uint32), dr2.view(np.uint32))


def test_chain_rule_trains_a_head_through_the_association_loss():
    """nn.Linear(24, 32) head -> build_graph_batch -> MOTMPNet(train) -> EdgeLoss('BCE') -> backward on the 12-detection frame: the head's
    weight gradient against  oracle(MPN input gradients)  ->  graph_grad_oracle in fp64  ->  d W = d_emb^T raw.
    Bound, built like test_chain_rule_trains_a_projection_in_front_of_the_mpn's: every stage is held to (5 e_ref_max + 2^-23) of its
    output's scale -- the MPN's input gradients (both of them), then the graph build's -- and the final product adds n 2^-24; all relative
    to S = max|d_emb| max_k sum_n |raw[n][k]|."""
    from gnn_cca_amd.loss import EdgeLoss
    from gnn_cca_amd.graph_build import build_graph_batch
    from oracle.mpn_oracle import TorchTrainOracle
    from test_gpu_input_grads import shaped_model
    from test_input_grads_oracle import e_ref_max as mpn_e_ref_max, oracle_input_grads
    a = load_grads("one_frame")
    n = a["node_embeds_raw"].shape[0]
    params, arch, sd, m = shaped_model(32, [128], "sum", False, False, 0.0, n)
    torch.manual_seed(4)
    lin = torch.nn.Linear(24, 32)
    raw = torch.randn(n, 24)
    lin_gpu = copy.deepcopy(lin).cuda()
    emb = lin_gpu(raw.cuda())
    b = build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], emb, emb)
    loss = EdgeLoss("BCE")(m(b), b.edge_labels)
    loss.backward()
    torch.cuda.synchronize()
    assert lin_gpu.weight.grad is not None, "no gradient reached the head in front of the graph build"
    # the oracle chain, from the batch the GPU built (its forward is pinned by test_gpu_graph_build.py)
    ref_loss, rdx, rdea = oracle_input_grads(TorchTrainOracle(params, arch, sd), b.x.detach().cpu().numpy(), a["edge_index"],
                                             b.edge_attr.detach().cpu().numpy(), b.edge_labels.cpu().numpy())
    assert abs(float(loss.detach()) - ref_loss) <= 2e-5
    emb64 = lin(raw).detach().double().numpy()
    case = dict(a, node_embeds_raw=emb64, reid_embeds_raw=emb64)
    dn, dr = ggo.graph_build_backward(case, np.float64, g_x=rdx, g_ea=rdea)
    d_emb = dn + dr
    rgw = d_emb.T @ raw.double().numpy()
    s = float(np.abs(d_emb).max()) * float(raw.abs().sum(0).max())
    mpn, gb = mpn_e_ref_max("sum"), e_ref_max()
    bound = (5 * (mpn["dx"] + mpn["dea"]) + 5 * max(gb.values()) + 2 * EPS + n * 2.0 ** -24) * s
    err = float(np.abs(lin_gpu.weight.grad.cpu().numpy() - rgw).max())
    print(f"chain rule: max|dW - dW_oracle| {err:.3e}  bound {bound:.3e}  max|dW| {np.abs(rgw).max():.3e}")
    assert np.abs(rgw).max() > 0 and err <= bound


def test_forward_and_backward_under_graph_capture(monkeypatch):
    """build_graph_batch + backward captured into one HIP graph on a single stream and replayed: the replay's gradients are bit for bit the
    eager ones, so nothing on the path synchronises (the capture would fail).  The staging ring is private to this test: an event
    recorded during a capture must not be waited on by a later, eager batch."""
    from gnn_cca_amd import frames, graph_build as gbm
    a = load_grads("batch3")
    monkeypatch.setattr(frames, "_staging", {})
    node = torch.from_numpy(a["node_embeds_raw"]).cuda().requires_grad_()
    reid = torch.from_numpy(a["reid_embeds_raw"]).cuda().requires_grad_()
    gx, gea = torch.from_numpy(a["g_x"]).cuda(), torch.from_numpy(a["g_edge_attr"]).cuda()

    def step():
        b = gbm.build_graph_batch(a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], node, reid)
        torch.autograd.backward([b.x, b.edge_attr], [gx, gea])

    for _ in range(frames._Staging.SLOTS):   # every slot of the ring gets its pinned buffer and event outside the capture
        node.grad = reid.grad = None
        step()
    torch.cuda.synchronize()
    assert node.grad is not None and reid.grad is not None
    eager_n, eager_r = node.grad.clone(), reid.grad.clone()
    node.grad = reid.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        node.grad.zero_(), reid.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(node.grad, eager_n) and torch.equal(reid.grad, eager_r)


def test_no_edges_and_double_backward():
    """All detections on one camera (E == 0): a zero reid gradient, the node gradient from x alone, nothing faults.  Double backward
    raises torch's error."""
    a = synthetic([[2] * 5], 16, 8, 13)
    assert a["g_edge_attr"].shape[0] == 0
    b, d_node, d_reid = run(a)
    assert b.edge_index.shape == (2, 0) and d_node is not None
    assert d_reid is not None and d_reid.shape == a["reid_embeds_raw"].shape and not d_reid.any()
    check("E == 0 d_node", d_node, ggo.normalize_backward(a["node_embeds_raw"], a["g_x"], np.float64), e_ref_max()["d_node"], factor=5)
    from gnn_cca_amd.graph_build import build_graph_batch
    c = load_grads("interleaved")
    reid = torch.from_numpy(c["reid_embeds_raw"]).cuda().requires_grad_()
    b = build_graph_batch(c["xw"], c["yw"], c["id"], c["id_cam"], c["graph_sizes"], c["max_dist"], torch.from_numpy(c["node_embeds_raw"]).cuda(), reid)
    g, = torch.autograd.grad(b.edge_attr.sum(), [reid], create_graph=True)
    assert g is not None and g.shape == reid.shape
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g.sum(), [reid])
