"""Synthetic configurations of the tuned family that between them take every branch of the weight-pack program (csrc/pack.cpp:
pack_program): BatchNorm in every MLP with running statistics that are not 0 / 1, node encoders of 1, 2 and 3 layers, a first layer with
and without the bf16 / fp16 piece images, edge_in 2 / 4 / 16, the four reattach combinations, the three classifier shapes, and first-layer
weights beyond fp16's range and inside its subnormal range.  Parameters come from numpy's default_rng(seed), not from torch's
initialisers.  tests/test_gpu_parity.py packs them on the device against the host; tools/pack_blob_diff.py packs them with two builds
of the library."""
import numpy as np
import torch

ARCH = "resnet50"

#        name             node_in node_fc      edge_in  bn     reattach (n, e)  cls_fc  planted first-layer weights
CONFIGS = [
    ("bn_everywhere",     2048,   (128,),      4,       True,  (False, False),  (4,),   ()),
    ("enc3_bn",           256,    (128, 64),   4,       True,  (False, False),  (4,),   ()),
    ("enc1_edge2",        96,     (),          2,       False, (False, False),  (),     ()),
    ("enc1_edge2_bn",     96,     (),          2,       True,  (True, False),   (8,),   ()),
    ("first_not_128",     2048,   (96,),       4,       False, (False, False),  (4,),   ()),
    ("first_in_odd",      100,    (128,),      4,       True,  (False, True),   (8,),   ()),
    ("reattach_both_e16", 64,     (128,),      16,      True,  (True, True),    (8,),   ()),
    ("reattach_nodes",    64,     (128,),      16,      False, (True, False),   (4,),   ()),
    ("reattach_edges",    64,     (128,),      4,       False, (False, True),   (),     ()),
    ("f16_overflow",      64,     (128,),      4,       False, (False, False),  (4,),   (65520.0, -7.0e4, 65519.0)),
    ("f16_subnormal",     64,     (128,),      4,       False, (False, False),  (4,),   (6.0e-8, -3.0e-6, 5.9e-5, 2.0e-8)),
    ("f16_extremes_bn",   2048,   (128,),      4,       True,  (False, False),  (4,),   (1.0e6, 6.0e-8, -3.0e-6)),
]
NAMES = [c[0] for c in CONFIGS]


def model_params(name):
    _, node_in, node_fc, edge_in, bn, (re_n, re_e), cls_fc, _ = CONFIGS[NAMES.index(name)]
    return {
        "node_agg_fn": "sum", "num_enc_steps": 2, "num_class_steps": 1,
        "reattach_initial_nodes": re_n, "reattach_initial_edges": re_e,
        "encoder_feats_dict": {
            "edges": {"edge_in_dim": edge_in, "edge_fc_dims": [], "edge_out_dim": 6},
            "nodes": {ARCH: {"node_in_dim": node_in, "node_fc_dims": list(node_fc), "node_out_dim": 32, "dropout_p": 0, "use_batchnorm": bn}},
        },
        "edge_model_feats_dict": {"fc_dims": [6], "dropout_p": 0, "use_batchnorm": bn},
        "node_model_feats_dict": {"fc_dims": [32], "dropout_p": 0, "use_batchnorm": bn},
        "classifier_feats_dict": {"edge_in_dim": 6, "edge_fc_dims": list(cls_fc), "edge_out_dim": 1, "dropout_p": 0, "use_batchnorm": bn},
    }


def state_dict(model, name):
    """Every tensor of `model` from default_rng(seed of the configuration); the planted weights go to scattered elements of the first
    encoder weight (different rows, k-chunks and 256-element pack blocks)."""
    rng = np.random.default_rng(1000 + NAMES.index(name))
    sd = {}
    for key, t in model.state_dict().items():
        if not t.dtype.is_floating_point:       # num_batches_tracked
            sd[key] = t.clone()
        elif key.endswith("running_var"):
            sd[key] = torch.from_numpy(rng.uniform(0.3, 3.0, tuple(t.shape)).astype(np.float32))
        else:                                   # weights, biases, BatchNorm gamma / beta / running_mean
            sd[key] = torch.from_numpy(rng.normal(0.0, 0.5, tuple(t.shape)).astype(np.float32))
    first = next(k for k in sd if k.startswith("encoder.node_mlp") and sd[k].dim() == 2)
    w = sd[first].view(-1)
    for i, v in enumerate(CONFIGS[NAMES.index(name)][7]):
        w[(i * 2087 + 300) % w.numel()] = v
    return sd


def build(name):
    from gnn_cca_amd import MOTMPNet
    m = MOTMPNet(model_params(name), None, ARCH)
    m.load_state_dict(state_dict(m, name), strict=True)
    return m.eval()
