"""A forward is a function of its inputs and weights only.  The module's workspace (MOTMPNet._scratch) is `torch.empty` and
grow-only, so a kernel that reads a region this forward has not written -- a partial slab, a flag word, a padded edge slot -- reads
whatever the last forward or allocation left there, and its result can change from call to call while a test on a fresh process
still passes.  Every case here runs a forward, fills every byte of the module's workspaces with a pattern, runs the same forward
again, and requires BIT FOR BIT the same logits and graph flags.  0x7F makes every float 3.4e38 and 0x41 makes it 12.1 (finite and
positive: a NaN pattern would not do, the kernels' ReLU maps a negative NaN to 0)."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle.mpn_oracle import load_case

pytestmark = pytest.mark.gpu

POISON = (0x7F, 0x41)


class Data:
    def __init__(self, x, edge_index, edge_attr):
        self.x, self.edge_index, self.edge_attr = x, edge_index, edge_attr


def poison_workspaces(m, byte):
    """Overwrite every workspace of `m` (all streams' ones) with `byte`, on the current stream."""
    assert len(m._workspaces) > 0
    for ws in m._workspaces.values():
        ws.fill_(byte)


def assert_poison_invariant(m, d, ref=None):
    """Logits and graph flags of `m(d)` are unchanged after the workspace is poisoned with each pattern.  `ref`: the logits of an
    earlier forward of the same inputs (default: one run here)."""
    with torch.no_grad():
        if ref is None:
            ref = [t.clone() for t in m(d)["classified_edges"]]
        flags = m.graph_flags()
        for byte in POISON:
            poison_workspaces(m, byte)
            out = m(d)["classified_edges"]
            assert len(out) == len(ref)
            for i, (a, b) in enumerate(zip(out, ref)):
                assert torch.equal(a, b), (hex(byte), i, float((a - b).abs().max()))
            assert m.graph_flags() == flags, (hex(byte), m.graph_flags(), flags)
    return ref


def ring_graph(n_nodes, rng, node_in=2048, hops=(1, 5, 17)):
    """Sparse ring: node i -> i + h (mod N) for every hop h."""
    x = rng.standard_normal((n_nodes, node_in)).astype(np.float32)
    src = np.repeat(np.arange(n_nodes), len(hops))
    dst = (src + np.tile(list(hops), n_nodes)) % n_nodes
    ei = np.stack([src, dst]).astype(np.int64)
    ea = rng.random((ei.shape[1], 4)).astype(np.float32)
    return x, ei, ea


def to_device(x, ei, ea):
    return Data(torch.from_numpy(x).cuda(), torch.from_numpy(ei).cuda(), torch.from_numpy(ea).cuda())


def _params(**over):
    params, arch, _, _ = load_case(os.path.join(GOLDEN_DIR, "dense64.npz"))
    params = copy.deepcopy(params)
    params.update(over)
    return params, arch


def _model(params, arch, seed=0):
    from gnn_cca_amd import MOTMPNet
    torch.manual_seed(seed)
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    with torch.no_grad():   # node MLP scaled down: 'sum' over the ring's in-degree keeps activations O(1)
        for p in m.MPNet.node_model.node_mlp.parameters():
            p.mul_(1.0 / 3)
    return m.cuda().eval()


@pytest.mark.parametrize("n_nodes", [2, 64, 301, 1229, 2560, 3007, 4099, 6153, 8197, 51233])
def test_shipped_shape_poisoned_workspace(n_nodes):
    """The shipped encoder (2048 -> 128 -> 32) on every first-layer route its node count selects: f32 plan GEMM (2), fp16-split
    slices (64 ... 3007, wave-per-node or MFMA tail), 32-row fused (4099, 6153, 8197), 256-row un-split fused (51233)."""
    params, arch = _params()
    m = _model(params, arch, seed=n_nodes)
    d = to_device(*ring_graph(n_nodes, np.random.default_rng(n_nodes)))
    out = assert_poison_invariant(m, d)
    assert all(torch.isfinite(t).all() for t in out)


@pytest.mark.parametrize("option,n_nodes", [("bf16", 301), ("bf16", 8197), ("products3", 1229), ("products3", 6153),
                                            ("unsplit", 4099), ("unsplit", 8197), ("unsplit", 51233)])
def test_forward_options_poisoned_workspace(option, n_nodes):
    """`edge_state_dtype = 'bf16'`, `encoder_products = 3` (128-row / 256-row bf16 split-K GEMMs + tails) and `encoder_unsplit` at
    >= 4096 nodes (32-row and 256-row un-split kernels)."""
    params, arch = _params()
    m = _model(params, arch, seed=n_nodes)
    if option == "bf16":
        m.edge_state_dtype = "bf16"
    elif option == "products3":
        m.encoder_products = 3
    else:
        m.encoder_unsplit = True
    d = to_device(*ring_graph(n_nodes, np.random.default_rng(n_nodes)))
    assert_poison_invariant(m, d)


@pytest.mark.parametrize("route", ["steps_L0", "max_aggregation", "reattach_both", "generic_fused", "generic_op_by_op"])
@pytest.mark.parametrize("n_nodes", [64, 3007])
def test_other_forward_routes_poisoned_workspace(route, n_nodes):
    """L = 0 (no step kernel), the general step kernel (max aggregation; both reattach flags), the generic family's fused step
    (node latent 48) and its op-by-op form (node latent 160)."""
    params, arch = _params()
    if route == "steps_L0":
        params["num_enc_steps"], params["num_class_steps"] = 0, 1
    elif route == "max_aggregation":
        params["node_agg_fn"] = "max"
    elif route == "reattach_both":
        params["reattach_initial_nodes"] = params["reattach_initial_edges"] = True
    elif route == "generic_fused":
        params["encoder_feats_dict"]["nodes"][arch]["node_out_dim"] = 48
        params["node_model_feats_dict"]["fc_dims"] = [48]
    elif route == "generic_op_by_op":
        params["encoder_feats_dict"]["nodes"][arch]["node_out_dim"] = 160
        params["node_model_feats_dict"]["fc_dims"] = [160]
    m = _model(params, arch, seed=7)
    d = to_device(*ring_graph(n_nodes, np.random.default_rng(n_nodes + 1)))
    assert_poison_invariant(m, d)


@pytest.mark.parametrize("agg,edge_state", [("sum", "fp32"), ("mean", "fp32"), ("sum", "bf16")])
def test_padded_layout_poisoned_workspace(agg, edge_state):
    """The batch of test_padded_layout_ragged_batch_vs_oracle: 45 dense graphs of 120 ... 129 nodes, edge state in the padded layout
    (128 slots per node, every segment ends in padding slots)."""
    from test_gpu_parity import _default_model, _union
    from test_gpu_parity import build as build_golden
    params, arch, sd = _default_model(1.0 / 124, node_agg_fn=agg)
    rng = np.random.default_rng(5)
    x, ei, ea = _union([120 + (7 * g) % 10 for g in range(45)], rng)
    assert ei.shape[1] >= 1 << 19
    m = build_golden(params, arch, sd)
    m.edge_state_dtype = edge_state
    assert_poison_invariant(m, to_device(x, ei, ea))


def test_frame_pipeline_poisoned_workspace():
    """FramePipeline borrows the module's workspace (MOTMPNet._scratch) for the graph build, the forward and the pruning: one call
    after the workspace is poisoned gives every output of the call before it, bit for bit."""
    from gnn_cca_amd.pipeline import FramePipeline
    from test_gpu_pipeline import _frames, _model as pipeline_model
    m = pipeline_model()
    rng = np.random.default_rng(11)
    f = _frames(rng, 64)
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    pipe = FramePipeline(m)
    keys = ("probs", "preds", "pruned", "flow_out", "flow_in", "labels", "n_clusters", "triggers")

    def snapshot(r):
        got = {k: getattr(r, k).clone() for k in keys}
        got["logits"] = [t.clone() for t in r.outputs["classified_edges"]]
        got["edge_index"] = r.batch.edge_index.clone()
        got["edge_attr"] = r.batch.edge_attr.clone()
        return got

    ref = snapshot(pipe(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid))
    flags = m.graph_flags()
    for byte in POISON:
        poison_workspaces(m, byte)
        got = snapshot(pipe(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid))
        for k in keys + ("edge_index", "edge_attr"):
            assert torch.equal(got[k], ref[k]), (hex(byte), k)
        for a, b in zip(got["logits"], ref["logits"]):
            assert torch.equal(a, b), hex(byte)
        assert m.graph_flags() == flags
    pipe.close()
