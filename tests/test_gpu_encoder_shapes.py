"""Node-encoder shapes of the fast family (csrc/pack.cpp: kFamilyMfma32x6) beyond the shipped `in -> 128 -> 32`.

The family takes any node encoder of up to GNNCCA_MAX_LAYERS layers no wider than 1024 and any node_in_dim.  Which GEMM form its
first layer runs on, how many partial slabs that launch writes (summed by reduce_bias_act_kernel for encoders of three or more layers,
by the encoder tail otherwise), where the graph plan goes and which tail follows is decided by encoder_route() (csrc/enc_route.cpp)
from N, K, the first layer's width, the depth and the options; tests/test_encoder_route.py pins that table on the CPU.  Every case here builds a
model from torch.manual_seed and, on a sparse ring graph:

  * asserts from the packed header that the model really is on the fast family;
  * judges the encoder output (trace['h_enc']) against an fp64 evaluation, within 4x the fp32 oracle's own error;
  * judges the UNTRACED logits (the production route: the traced forward skips the padded layout and the register-resident tail)
    against the fp32 oracle;
  * poisons the workspace (test_gpu_workspace_poison.py) and requires bit-for-bit the same logits;
  * checks the device-packed weight blob against the host packer's byte for byte (pack kinds 2 and 4, the split weight images of the
    first layer, included).

The forms (csrc/internal.h: EncForm) as the docstrings below name them:
  PLAN    kEncPlanGemm: the f32 plan GEMM in Workspace::ksplit slabs, and every GEMM layer behind the first;
  SLICES  kEncSlices: fp16-split slices, nks <= Workspace::ksplit slabs;
  D128    kEncD128: the 128-row split-bf16 GEMM;
  R32     kEncR32F16 (kEncR32Bf16 under encoder_unsplit): 32-row un-split GEMM with the fused epilogue, no tail launch;
  LDS256  kEncLdsF16 / kEncLdsBf16: the 256-row GEMM, split-K + a tail / reduce, or un-split with the fused epilogue;
and the tails (EncTail): MFMA (kTailMfma), fast (kTailFast) or wave-per-node through LDS (kTailLds)."""
import copy
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle.mpn_oracle import NumpyOracle, load_case
from test_gpu_workspace_poison import assert_poison_invariant, ring_graph, to_device

pytestmark = pytest.mark.gpu

TOL_TIGHT = 5e-6
FAMILY_MFMA32X6 = 1   # csrc/internal.h: kFamilyMfma32x6


def _model(node_in, fc, seed, reattach=False):
    from gnn_cca_amd import MOTMPNet
    params, arch, _, _ = load_case(os.path.join(GOLDEN_DIR, "dense64.npz"))
    params = copy.deepcopy(params)
    params["encoder_feats_dict"]["nodes"][arch]["node_in_dim"] = node_in
    params["encoder_feats_dict"]["nodes"][arch]["node_fc_dims"] = list(fc)
    params["reattach_initial_nodes"] = reattach
    torch.manual_seed(seed)
    ref_m = MOTMPNet(copy.deepcopy(params), None, arch)
    sd = {k: v.detach().clone().numpy() for k, v in ref_m.state_dict().items()}
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return params, arch, sd, m.cuda().eval()


def _check(node_in, fc, n_nodes, reattach=False, products=6, unsplit=False):
    params, arch, sd, m = _model(node_in, fc, seed=node_in + n_nodes + len(fc), reattach=reattach)
    m.encoder_products = products
    m.encoder_unsplit = unsplit
    host_blob = m.pack_weights_host()
    family, = struct.unpack("<I", host_blob[8:12].numpy().tobytes())
    assert family == FAMILY_MFMA32X6, (node_in, fc, family)
    dev_blob = m._pack_weights_device(torch.device("cuda", torch.cuda.current_device()))
    assert dev_blob is not None
    torch.cuda.synchronize()
    assert torch.equal(dev_blob.cpu(), host_blob), (node_in, fc)

    rng = np.random.default_rng(n_nodes + node_in)
    x, ei, ea = ring_graph(n_nodes, rng, node_in=node_in)
    orc = NumpyOracle(params, arch, sd, np.float32)
    tr = {}
    ref = orc.forward(x, ei, ea, tr)
    d = to_device(x, ei, ea)
    trace = {}
    with torch.no_grad():
        for byte in (0x7F, 0x41):   # whatever a previous forward left in the workspace must not matter; here: a fresh one
            m(d)
            for ws in m._workspaces.values():
                ws.fill_(byte)
        m(d, trace=trace)
        out = [t.clone() for t in m(d)["classified_edges"]]
    h64 = NumpyOracle(params, arch, sd, np.float64)._mlp("encoder.node_mlp", x.astype(np.float64))
    err_gpu = float(np.abs(trace["h_enc"].cpu().numpy() - h64).max())
    err_ref = float(np.abs(tr["h_enc"] - h64).max())
    scale_h = max(1.0, float(np.abs(h64).max()))
    if products == 6:
        assert err_gpu <= max(4 * err_ref, 2e-7 * scale_h), (err_gpu, err_ref)
    else:   # three of the six split products (GNNCCA_OPT_ENC_SPLIT3): ~2^-17 relative on the first layer
        assert err_gpu <= 4e-5 * scale_h, err_gpu
    for i, (o, r) in enumerate(zip(out, ref)):
        scale = max(1.0, float(np.abs(r).max()))
        err = float(np.abs(o.cpu().numpy() - r).max())
        assert err <= TOL_TIGHT * 2 * scale, (i, err, scale)
    assert_poison_invariant(m, d, out)


# The deep encoders of the slab-count fix: the first layer writes EncGemmRoute::slabs slabs (SLICES: nks, D128 / LDS256: the split its
# form picked) and reduce_bias_act_kernel must sum exactly those, not ws.ksplit.  With 2048 -> 128 -> 64 -> 32:
#   64, 301 nodes    SLICES, 16 slabs written of ws.ksplit = 32
#   1229             SLICES, 8 of 16
#   3007             SLICES, 8 of 8
#   4099             D128, 8 of 8
#   8197             LDS256 split-K (not fusable: three layers), 4 of 8
#   51233            LDS256, 1 slab of ws.ksplit = 2
@pytest.mark.parametrize("n_nodes", [64, 301, 1229, 3007, 4099, 8197, 51233])
def test_three_layer_encoder_2048_128_64(n_nodes):
    """node_fc_dims [128, 64], node_in 2048: SLICES (<= 3007), D128 (4099), LDS256 split-K (8197) and un-split (51233), each
    followed by ENC_REDUCE, the 128 -> 64 plan GEMM and the wave-per-node tail."""
    _check(2048, [128, 64], n_nodes)


@pytest.mark.parametrize("n_nodes", [64, 301, 1229, 3007, 51233])
def test_four_layer_encoder_2048_128_128_64(n_nodes):
    """node_fc_dims [128, 128, 64]: the SLICES / LDS256 first layer, then two reduces (the second behind a one-slab plan GEMM)
    through the ping-pong activation buffer."""
    _check(2048, [128, 128, 64], n_nodes)


@pytest.mark.parametrize("node_in,n_nodes", [(512, 301), (512, 1229), (512, 6153), (1536, 301), (1536, 1229), (1000, 1229), (40, 301)])
def test_three_layer_encoder_other_inputs(node_in, n_nodes):
    """node_fc_dims [128, 64] on other inputs: node_in 512 SLICES (8 of 8 slabs at 301, 4 of 8 at 1229) and LDS256 split-K (6153);
    1536 (a multiple of 32, not a power of two: no SLICES) PLAN at 301 and D128 at 1229; 1000 (K % 32 != 0: no split weights)
    and 40 (below 64) PLAN."""
    _check(node_in, [128, 64], n_nodes)


@pytest.mark.parametrize("option,n_nodes", [("products3", 6153), ("products3", 8197), ("unsplit", 6153), ("unsplit", 8197)])
def test_three_layer_encoder_under_options(option, n_nodes):
    """[128, 64] at 6153 / 8197 nodes under `encoder_products = 3` (bf16 LDS256, three products) and `encoder_unsplit` (bf16
    LDS256, six products): both change the first layer's split from the default's, on the reduce's input.  The 32-row un-split
    kernel needs the two-layer encoder, so `encoder_unsplit` still splits K here (include/gnncca_mpn.h)."""
    _check(2048, [128, 64], n_nodes, products=3 if option == "products3" else 6, unsplit=option == "unsplit")


@pytest.mark.parametrize("node_in,n_nodes", [(2048, 64), (2048, 3007), (40, 301), (1000, 6153)])
def test_one_layer_encoder(node_in, n_nodes):
    """node_fc_dims []: in -> 32 in ONE layer -- PLAN (no split weights), the tail with has_last = 0 sums the slabs."""
    _check(node_in, [], n_nodes)


@pytest.mark.parametrize("node_in,fc,n_nodes", [(2048, [64], 301), (2048, [64], 3007), (512, [64], 6153),
                                                (2048, [256], 64), (2048, [256], 3007), (512, [256], 8197),
                                                (2048, [100], 301), (2048, [100], 1229), (1000, [100], 4099)])
def test_two_layer_encoder_other_widths(node_in, fc, n_nodes):
    """First layer 64, 256 or 100 wide: no split weights (those need 128), so PLAN at every N and the wave-per-node tail; 100 is
    not a multiple of 4, so the tail's vectorised slab reduction is off."""
    _check(node_in, fc, n_nodes)


@pytest.mark.parametrize("reattach,node_in,n_nodes", [(False, 512, 64), (False, 2048, 1229), (True, 512, 301), (True, 2048, 3007)])
def test_widest_hidden_layer(reattach, node_in, n_nodes):
    """node_fc_dims [1024] (the family's widest layer): PLAN and the wave-per-node tail with a 1024 x 32 last layer in LDS; with
    reattach_initial_nodes the tail's LDS request is exactly the 160 KB it may take (mpn_forward.hip: hin * kProjOut + F * kH +
    4 F + 1024 floats)."""
    _check(node_in, [1024], n_nodes, reattach=reattach)


@pytest.mark.parametrize("node_in,n_nodes", [(1536, 301), (1536, 2000), (1536, 3007), (1536, 6153), (1536, 9000), (1000, 1229),
                                             (1000, 3007), (40, 64), (40, 2560), (512, 2560)])
def test_shipped_widths_other_inputs(node_in, n_nodes):
    """node_fc_dims [128] (the shipped widths) on inputs the goldens never use: 1536 PLAN (301), D128 + wave-per-node tail (2000),
    D128 + MFMA tail (3007), R32 (6153), LDS256 split-K + MFMA tail (9000); 1000 and 40 (no split weights) PLAN + wave-per-node tail
    below 2560 nodes and + MFMA tail from there; 512 SLICES + MFMA tail (2560)."""
    _check(node_in, [128], n_nodes)


@pytest.mark.parametrize("fc,n_nodes,want", [([128, 64], 301, ["enc_gemm", "enc_reduce", "enc_gemm", "enc_tail"]),
                                             ([128, 64], 51233, ["enc_gemm", "plan", "enc_reduce", "enc_gemm", "enc_tail"]),
                                             ([128], 9000, ["enc_gemm", "plan", "enc_tail"]),
                                             ([128], 6153, ["plan", "enc_gemm"]),
                                             ([128], 51233, ["plan", "enc_gemm"])])
def test_profiled_kernel_sequence(fc, n_nodes, want):
    """The launches of the encoder, as forward_profiled() reports them: SLICES with the plan riding (301), LDS256 split-K with a
    plan launch of its own (51233 deep, 9000), each followed by a reduce between the GEMMs of a deep encoder and by a tail; the fused
    routes (R32 at 6153, LDS256 un-split at 51233) have the plan first and no tail launch."""
    _, _, _, m = _model(2048, fc, seed=1)
    d = to_device(*ring_graph(n_nodes, np.random.default_rng(3)))
    with torch.no_grad():
        _, times = m.forward_profiled(d)
    kinds = [k for k, _ in times if not k.startswith("step")]
    assert kinds == want, kinds


_G, _P, _R, _T = "enc_gemm", "plan", "enc_reduce", "enc_tail"


@pytest.mark.parametrize("node_in,fc,n_nodes,unsplit,want", [
    (2048, [128], 64, False, [_G, _T]),                       # SLICES, the plan riding; fast tail
    (2048, [128], 2560, False, [_G, _T]),                     # SLICES; MFMA tail
    (2048, [128], 4096, False, [_P, _G]),                     # R32_F16: the plan first, no tail
    (2048, [128], 8192, False, [_P, _G]),
    (2048, [128], 8193, False, [_G, _P, _T]),                 # LDS256_F16 split-K 4: the plan behind the GEMM, MFMA tail
    (2048, [128], 4099, True, [_P, _G]),                      # encoder_unsplit: R32_BF16
    (1536, [128], 301, False, [_G, _T]),                      # PLAN form (K not a power of two, below 384 nodes)
    (1536, [128], 1229, False, [_G, _T]),                     # D128, the plan riding
    (2048, [], 64, False, [_G, _T]),                          # one layer: PLAN form, the tail without a last layer
    (2048, [128, 64], 4099, False, [_G, _R, _G, _T]),         # D128, reduce, 128 -> 64 PLAN form, LDS tail
    (2048, [128, 64], 8197, False, [_G, _P, _R, _G, _T]),     # LDS256_F16 split-K (three layers: not fusable)
    (2048, [128, 128, 64], 3007, False, [_G, _R, _G, _R, _G, _T])])
def test_profiled_kinds_follow_the_route_table(node_in, fc, n_nodes, unsplit, want):
    """The whole kind sequence of forward_profiled() -- encoder launches, then `step` for every message step but the last and `step_last` --
    is the one encoder_route() implies (tests/test_encoder_route.py pins the routes themselves on the CPU): a riding plan has no launch
    of its own, a fused GEMM has the plan in front and no tail, the other big-batch forms have the plan behind the GEMM, and every
    GEMM but the last is followed by a reduce."""
    _, _, _, m = _model(node_in, fc, seed=1)
    m.encoder_unsplit = unsplit
    d = to_device(*ring_graph(n_nodes, np.random.default_rng(3), node_in=node_in))
    with torch.no_grad():
        _, times = m.forward_profiled(d)
    kinds = [k for k, _ in times]
    enc = [k for k in kinds if not k.startswith("step")]
    steps = kinds[len(enc):]
    assert enc == want and kinds[:len(enc)] == enc, kinds
    L = m.native_dims().num_enc_steps
    assert L >= 1 and steps == ["step"] * (L - 1) + ["step_last"], kinds


@pytest.mark.parametrize("cls,family", [([8], FAMILY_MFMA32X6), ([], FAMILY_MFMA32X6), ([1], 2)])
@pytest.mark.parametrize("n_nodes", [64, 3007])
def test_classifier_shapes(cls, family, n_nodes):
    """classifier edge_fc_dims other than the shipped [4]: a hidden layer of 8 (the widest the fast family keeps in registers) and
    none stay on the fast family; a hidden layer of width 1 has no ReLU (models/mlp.py) where the family's classifier kernels apply
    one, so it runs on the generic family (csrc/pack.cpp: classify).  Logits against the fp32 oracle, poisoned workspace."""
    from gnn_cca_amd import MOTMPNet
    params, arch, _, _ = load_case(os.path.join(GOLDEN_DIR, "dense64.npz"))
    params = copy.deepcopy(params)
    params["classifier_feats_dict"]["edge_fc_dims"] = list(cls)
    torch.manual_seed(n_nodes + len(cls))
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    with torch.no_grad():
        for p in m.MPNet.node_model.node_mlp.parameters():
            p.mul_(1.0 / 3)
        for mod in m.modules():   # BatchNorm running statistics other than (0, 1): the fold is exercised
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.5, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
    sd = {k: v.detach().clone().numpy() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    got, = struct.unpack("<I", m.pack_weights_host()[8:12].numpy().tobytes())
    assert got == family, (cls, got)
    x, ei, ea = ring_graph(n_nodes, np.random.default_rng(n_nodes), node_in=2048)
    ref = NumpyOracle(params, arch, sd, np.float32).forward(x, ei, ea)
    d = to_device(x, ei, ea)
    with torch.no_grad():
        out = [t.clone() for t in m(d)["classified_edges"]]
    for i, (o, r) in enumerate(zip(out, ref)):
        scale = max(1.0, float(np.abs(r).max()))
        err = float(np.abs(o.cpu().numpy() - r).max())
        assert err <= TOL_TIGHT * 2 * scale, (i, err, scale)
    assert_poison_invariant(m, d, out)
