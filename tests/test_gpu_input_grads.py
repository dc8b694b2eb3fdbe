"""Row N3 on the GPU, input gradients: loss.backward() through gnn_cca_amd.MOTMPNet in train mode fills data.x.grad and
data.edge_attr.grad like the reference's module does -- both training engines, against the reference's own gradients
(tests/golden/input_grads/igrad_*.npz: fp32 and fp64) and, at sizes that exercise the d x kernel's tiling, against the autograd oracle.

Accuracy criterion (relative: these gradients are small).  Per tensor e(t) = max|t - t64| / max|t64|; the yardstick is the reference's
own fp32 run, e_ref = e(t32); the GPU must satisfy  e_gpu <= 4 e_ref + 2^-23  (two fp32 evaluations with different summation orders
each sit about e_ref from the truth, and the GPU's atomically ordered sums over the edges add one more such term upstream of the
products that form the input gradients).  Shapes without an fp64 fixture: e_gpu_vs_oracle32 <= 5 e_ref_max + 2^-23, e_ref_max the
largest e_ref over the fixtures of the same aggregator.  Every test prints both figures before it asserts.
"""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle.mpn_oracle import TorchTrainOracle, load_case
from test_backward_oracle import load_bwd
from test_input_grads_oracle import EPS, IGRAD_CASES, e_ref_max, load_igrad, oracle_input_grads, rel_err

pytestmark = pytest.mark.gpu


class Data:
    def __init__(self, x, edge_index, edge_attr):
        self.x, self.edge_index, self.edge_attr = x, edge_index, edge_attr


def build(params, arch, sd, engine="auto"):
    from gnn_cca_amd import MOTMPNet
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m.train_engine = engine
    return m.cuda().train()


def loss_of(out, labels):
    crit = torch.nn.BCEWithLogitsLoss(reduction="mean")
    return sum(crit(t.view(-1), labels) for t in out["classified_edges"])  # train.py:80-97


def offset_view(t):
    """`t` on the GPU as a contiguous view that starts 4 bytes into a larger buffer: contiguous by construction, and its base pointer
    is only 4-byte aligned (torch's allocations are 256-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def step(m, a, req_x, req_ea, seed=None, unaligned=False):
    """One forward + backward; returns (loss, logits, x.grad, edge_attr.grad, {parameter gradients}) as numpy / None."""
    if seed is not None:
        m.set_dropout_seed(seed)   # the same masks in every run of one case
    m.zero_grad(set_to_none=True)
    x = torch.from_numpy(np.asarray(a["x"]))
    x = offset_view(x) if unaligned else x.cuda()
    ea = torch.from_numpy(np.asarray(a["edge_attr"])).cuda()
    x.requires_grad_(req_x), ea.requires_grad_(req_ea)
    out = m(Data(x, torch.from_numpy(np.asarray(a["edge_index"])).cuda(), ea))
    loss = loss_of(out, torch.from_numpy(np.asarray(a["labels"])).cuda())
    loss.backward()
    g = lambda t: None if t.grad is None else t.grad.cpu().numpy()
    return (float(loss.detach()), [t.detach().cpu().numpy() for t in out["classified_edges"]], g(x), g(ea),
            {k: p.grad.cpu().numpy() for k, p in m.named_parameters() if p.grad is not None})


def check_fixture_bound(what, got, g, key):
    e_gpu, e_ref = rel_err(got, g[key + "64"]), rel_err(g[key + "32"], g[key + "64"])
    bound = 4 * e_ref + EPS
    print(f"{what}: {key} e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  ratio to bound {e_gpu / bound:.3f}")
    assert e_gpu <= bound, (what, key, e_gpu, e_ref)


@pytest.mark.parametrize("prefix,name", IGRAD_CASES)
def test_input_gradients_match_reference(prefix, name):
    """Every fixture case through the module (fused engine for bwd_*, layer-by-layer for lw_*): both input gradients present and within
    the criterion; parameter gradients and logits as in a run without input gradients; one input alone gets the same gradient."""
    params, arch, sd, _, _, a = load_bwd(name, prefix)
    g = load_igrad(name)
    seed = int(a["dropout_seed"]) if "dropout_seed" in a else None
    m = build(params, arch, sd)
    loss0, logits0, dx0, dea0, pg0 = step(m, a, False, False, seed)
    assert dx0 is None and dea0 is None
    loss, logits, dx, dea, pg = step(m, a, True, True, seed)
    assert dx is not None and dea is not None, "x.grad / edge_attr.grad missing: the backward returned None for the inputs"
    assert dx.shape == a["x"].shape and dea.shape == a["edge_attr"].shape
    check_fixture_bound(name, dx, g, "dx")
    check_fixture_bound(name, dea, g, "dea")
    # asking for the input gradients changes nothing else (tolerances of test_gpu_backward.py / test_gpu_train_layerwise.py:
    # the engines' own atomics reorder sums from run to run)
    tol_logit, tol_grad = (5e-6, 2e-5) if prefix == "bwd_" else (2e-5, 5e-5)
    assert abs(loss - loss0) <= tol_logit
    for t, t0 in zip(logits, logits0):
        assert np.abs(t - t0).max() <= tol_logit
    assert sorted(pg) == sorted(pg0)
    for k in pg0:
        assert np.abs(pg[k] - pg0[k]).max() <= tol_grad * max(1.0, float(np.abs(pg0[k]).max())), k
    # one input alone: the other's .grad stays None, and the one present is the gradient both-required gave (bit for bit given the
    # same upstream gradient; the upstream sums over the edges are atomically ordered, so: within the criterion, and of each other)
    _, _, dx_only, none_ea, _ = step(m, a, True, False, seed)
    _, _, none_x, dea_only, _ = step(m, a, False, True, seed)
    assert none_ea is None and none_x is None and dx_only is not None and dea_only is not None
    check_fixture_bound(name + " (x alone)", dx_only, g, "dx")
    check_fixture_bound(name + " (edge_attr alone)", dea_only, g, "dea")
    for alone, both, key in ((dx_only, dx, "dx"), (dea_only, dea, "dea")):
        bound = 4 * rel_err(g[key + "32"], g[key + "64"]) + EPS
        scale = float(np.abs(g[key + "64"]).max())
        assert np.abs(alone - both).max() <= bound * (scale if scale > 0 else 1.0), key


def cross_camera_edges(cam_sizes):
    """The Terrace topology (tests/golden/make_golden.py: cross_camera_edges): every node to every node of every other camera,
    nodes numbered camera by camera, row-major."""
    cam = np.repeat(np.arange(len(cam_sizes)), cam_sizes)
    i, j = np.meshgrid(np.arange(cam.size), np.arange(cam.size), indexing="ij")
    keep = cam[i] != cam[j]
    return int(cam.size), np.stack([i[keep], j[keep]]).astype(np.int64)


def shaped_model(node_in, node_fc, agg, re_n, re_e, p_enc, n, seed=5):
    """Randomly initialised weights of a node encoder node_in -> node_fc -> 32 (the other shapes as shipped, classifier BatchNorm
    off); the node-MLP is scaled by 1 / out-degree under 'sum' so that activations stay O(1) (make_golden.py does the same)."""
    from gnn_cca_amd import MOTMPNet
    params, arch, _, _ = load_case(os.path.join(GOLDEN_DIR, "n8_sum.npz"))
    params = copy.deepcopy(params)
    params.update(node_agg_fn=agg, reattach_initial_nodes=re_n, reattach_initial_edges=re_e)
    params["classifier_feats_dict"]["use_batchnorm"] = False
    enc = params["encoder_feats_dict"]["nodes"][arch]
    enc.update(node_in_dim=node_in, node_fc_dims=list(node_fc), dropout_p=p_enc)
    torch.manual_seed(seed)
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    with torch.no_grad():
        for prm in m.MPNet.node_model.node_mlp.parameters():
            prm.mul_(1.0 / max(1, n - (n + 3) // 4) if agg == "sum" else 1.0)
    sd = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    return params, arch, sd, m.cuda().train()


SHAPES = [
    # N, node_in, node_fc, agg, reattach_nodes, reattach_edges, p_enc
    (2, 64, [128], "sum", False, False, 0.0),        # 1 + 1 nodes: a partial row tile
    (2, 100, [96], "mean", True, False, 0.2),
    (33, 100, [128], "mean", True, True, 0.2),       # one row tile plus one row; 100 columns: no multiple of 4 or of a tile
    (33, 2048, [96], "max", False, False, 0.2),      # F1 != 128
    (33, 100, [128, 64], "sum", False, True, 0.2),   # three-layer node encoder: the layer-by-layer engine
    (301, 2048, [128], "sum", True, False, 0.0),     # the shipped width; many row tiles, a ragged last one
    (301, 512, [96], "max", False, True, 0.0),       # bdnet_market's width
    (301, 64, [128, 64], "mean", True, True, 0.0),
]


@pytest.mark.parametrize("n,node_in,node_fc,agg,re_n,re_e,p_enc", SHAPES)
def test_shapes_against_oracle(n, node_in, node_fc, agg, re_n, re_e, p_enc):
    """Tile edges of the d x kernel (rows, columns, F1), both engines, all aggregators, both reattach flags, encoder Dropout, and an x
    whose base pointer is only 4-byte aligned -- against torch autograd over the CPU oracle."""
    cams = [1, 1] if n == 2 else [n - 3 * (n // 4), n // 4, n // 4, n // 4]
    nn_, ei = cross_camera_edges(cams)
    assert nn_ == n
    params, arch, sd, m = shaped_model(node_in, node_fc, agg, re_n, re_e, p_enc, n)
    rng = np.random.default_rng(n * 7919 + node_in)
    x = rng.standard_normal((n, node_in)).astype(np.float32)
    x /= np.linalg.norm(x, axis=0, keepdims=True)     # inference.py:189-190 normalises over dim 0
    a = dict(x=x, edge_index=ei, edge_attr=rng.random((ei.shape[1], 4)).astype(np.float32),
             labels=(rng.random(ei.shape[1]) < 0.3).astype(np.float32))
    seed = 9001 if p_enc > 0 else None
    orc = TorchTrainOracle(params, arch, sd, dropout=dict(p_enc=p_enc, p_edge=0.0, p_node=0.0, p_cls=0.0, seed=seed) if seed else None)
    ref_loss, rdx, rdea = oracle_input_grads(orc, a["x"], a["edge_index"], a["edge_attr"], a["labels"])
    assert np.abs(rdx).max() > 0 and np.abs(rdea).max() > 0   # a dead network would make the comparison empty
    loss, _, dx, dea, _ = step(m, a, True, True, seed, unaligned=True)
    assert m._train_path == ("fused" if len(node_fc) == 1 else "layerwise")
    assert dx is not None and dea is not None, "x.grad / edge_attr.grad missing"
    assert abs(loss - ref_loss) <= 2e-5
    worst = e_ref_max(agg)
    for key, got, ref in (("dx", dx, rdx), ("dea", dea, rdea)):
        e, bound = rel_err(got, ref), 5 * worst[key] + EPS
        print(f"N={n} D={node_in} fc={node_fc} {agg}: {key} e_gpu_vs_oracle32 {e:.3e}  e_ref_max {worst[key]:.3e}  "
              f"ratio to bound {e / bound:.3f}")
        assert e <= bound, (key, e, worst[key])


def test_layerwise_engine_gives_the_fused_engines_input_gradients():
    params, arch, sd, _, _, a = load_bwd("terrace32_reatt_e")
    g = load_igrad("terrace32_reatt_e")
    res = {}
    for engine in ("fused", "layerwise"):
        m = build(params, arch, sd, engine=engine)
        _, _, dx, dea, _ = step(m, a, True, True)
        assert m._train_path == engine and dx is not None and dea is not None
        check_fixture_bound(engine, dx, g, "dx")
        check_fixture_bound(engine, dea, g, "dea")
        res[engine] = (dx, dea)
    for i, key in enumerate(("dx", "dea")):
        bound = 4 * rel_err(g[key + "32"], g[key + "64"]) + EPS
        assert np.abs(res["fused"][i] - res["layerwise"][i]).max() <= bound * float(np.abs(g[key + "64"]).max()), key


def test_chain_rule_trains_a_projection_in_front_of_the_mpn():
    """x = Linear(16, 64)(raw) feeds the MPN: after loss.backward() the Linear's weight gradient is the oracle's."""
    params, arch, sd, _, _, a = load_bwd("terrace32_reatt_n")
    n = a["x"].shape[0]
    torch.manual_seed(3)
    lin = torch.nn.Linear(16, 64)
    raw = torch.randn(n, 16)
    ref_loss, rdx, _, rgw = oracle_input_grads(TorchTrainOracle(params, arch, sd), lin(raw), a["edge_index"], a["edge_attr"],
                                               a["labels"], extra=(lin.weight,))
    m = build(params, arch, sd)
    lin_gpu = copy.deepcopy(lin).cuda()
    raw_gpu = raw.cuda()
    x = lin_gpu(raw_gpu)
    out = m(Data(x, torch.from_numpy(a["edge_index"]).cuda(), torch.from_numpy(a["edge_attr"]).cuda()))
    loss = loss_of(out, torch.from_numpy(a["labels"]).cuda())
    loss.backward()
    assert lin_gpu.weight.grad is not None, "no gradient reached the layer in front of the MPN"
    assert abs(float(loss.detach()) - ref_loss) <= 2e-5
    # d W[o][k] = sum_n dx[n][o] raw[n][k]: dx within (5 e_ref_max + 2^-23) max|dx| per element (the criterion), so the sum within that
    # times S = max|dx| max_k sum_n |raw[n][k]|, plus the product's own fp32 rounding, at most n 2^-24 S
    s = float(np.abs(rdx).max()) * float(raw.abs().sum(0).max())
    bound = (5 * e_ref_max("sum")["dx"] + EPS + n * 2.0 ** -24) * s
    err = float(np.abs(lin_gpu.weight.grad.cpu().numpy() - rgw).max())
    print(f"chain rule: max|dW - dW_oracle| {err:.3e}  bound {bound:.3e}  max|dW| {np.abs(rgw).max():.3e}")
    assert np.abs(rgw).max() > 0 and err <= bound


def test_double_backward_raises():
    params, arch, sd, _, _, a = load_bwd("n8_sum")
    m = build(params, arch, sd)
    x = torch.from_numpy(a["x"]).cuda().requires_grad_()
    out = m(Data(x, torch.from_numpy(a["edge_index"]).cuda(), torch.from_numpy(a["edge_attr"]).cuda()))
    loss = loss_of(out, torch.from_numpy(a["labels"]).cuda())
    gx, = torch.autograd.grad(loss, [x], create_graph=True)
    assert gx is not None and gx.shape == x.shape
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.sum(), [x])


def test_no_edges_gives_zero_input_gradient():
    """E == 0: empty logits, and a zero d x of x's shape (no edge, no path from x to a logit) on both engines."""
    params, arch, sd, _, _, a = load_bwd("n8_sum")
    for engine in ("fused", "layerwise"):
        m = build(params, arch, sd, engine=engine)
        x = torch.from_numpy(a["x"]).cuda().requires_grad_()
        ea = torch.zeros((0, a["edge_attr"].shape[1]), device="cuda", requires_grad=True)
        out = m(Data(x, torch.zeros((2, 0), dtype=torch.int64, device="cuda"), ea))
        sum(t.sum() for t in out["classified_edges"]).backward()
        assert x.grad is not None and x.grad.shape == x.shape and float(x.grad.abs().max()) == 0.0, engine
        assert ea.grad is not None and ea.grad.shape == ea.shape, engine


def test_input_gradients_under_graph_capture():
    """Forward + backward with x.requires_grad captured into one HIP graph and replayed on new inputs: nothing on the path
    synchronises or allocates through the C ABI (the capture would fail), and the replay's input gradients are the eager ones."""
    params, arch, sd, _, _, a = load_bwd("terrace32_reatt_n")
    g = load_igrad("terrace32_reatt_n")
    m = build(params, arch, sd)
    ei = torch.from_numpy(a["edge_index"]).cuda()
    labels = torch.from_numpy(a["labels"]).cuda()
    sx = torch.from_numpy(a["x"]).cuda().requires_grad_()
    sea = torch.from_numpy(a["edge_attr"]).cuda().requires_grad_()

    def run():
        loss_of(m(Data(sx, ei, sea)), labels).backward()

    for _ in range(2):   # eager warm-ups: the allocator and the workspace settle
        run()
    m.zero_grad(set_to_none=True)
    sx.grad = sea.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    rng = np.random.default_rng(1)
    x2 = (a["x"] * (1.0 + 0.1 * rng.standard_normal(a["x"].shape))).astype(np.float32)
    ea2 = rng.random(a["edge_attr"].shape).astype(np.float32)
    for xs, eas, ref in ((a["x"], a["edge_attr"], g), (x2, ea2, None), (a["x"], a["edge_attr"], g)):
        with torch.no_grad():
            sx.copy_(torch.from_numpy(xs)), sea.copy_(torch.from_numpy(eas))
        graph.replay()
        torch.cuda.synchronize()
        dx, dea = sx.grad.cpu().numpy().copy(), sea.grad.cpu().numpy().copy()
        if ref is not None:
            check_fixture_bound("replay", dx, ref, "dx")
            check_fixture_bound("replay", dea, ref, "dea")
        else:   # new inputs: the eager gradients of a fresh module on the same batch, within the criterion's bound of each other
            m2 = build(params, arch, sd)
            _, _, edx, edea, _ = step(m2, dict(a, x=xs, edge_attr=eas), True, True)
            for key, got, eager in (("dx", dx, edx), ("dea", dea, edea)):
                bound = 4 * rel_err(g[key + "32"], g[key + "64"]) + EPS
                e = rel_err(got, eager)
                print(f"replay on new inputs: {key} e_vs_eager {e:.3e}  bound {bound:.3e}")
                assert np.abs(eager).max() > 0 and e <= bound, key
