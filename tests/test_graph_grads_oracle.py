"""Backward of row N1 (graph build): the numpy restatement of the two backwards (tests/helpers/graph_grad_oracle.py -- the kernel's own
algebra: per frame C r + diag(alpha) r + 1e-6 beta, edge slots derived from the plan) against torch autograd through the reference's own
statements (tests/golden/graph_grads/*.npz, make_golden_graph_grads.py).  CPU only.  Home of what test_gpu_graph_grads.py shares with it.

Criterion (the project's, test_input_grads_oracle.py): e(t) = max|t - t64| / max|t64|; e_ref = e(reference fp32 run).  The fp64
restatement must sit within 1e-12 of the fixture's fp64 gradients, the fp32 restatement within 4 e_ref + 2^-23.
"""
import glob
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT
from test_input_grads_oracle import EPS, rel_err

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import graph_grad_oracle as ggo  # noqa: E402

GRADS_DIR = os.path.join(GOLDEN_DIR, "graph_grads")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GRADS_DIR, "*.npz")))


def load_grads(name):
    z = np.load(os.path.join(GRADS_DIR, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def e_ref_max():
    """Largest e_ref over the fixtures, per gradient: the yardstick for shapes without a fixture."""
    best = {"d_node": 0.0, "d_reid": 0.0}
    for name in CASES:
        a = load_grads(name)
        for k in best:
            best[k] = max(best[k], rel_err(a[k + "32"], a[k + "64"]))
    return best


def test_the_eight_cases_are_there_and_small():
    assert set(CASES) == {"one_frame", "batch3", "interleaved", "frame70", "camera_only", "only_appearance", "only_dist", "terrace32"}
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
    for name in CASES:
        assert os.path.getsize(os.path.join(GRADS_DIR, name + ".npz")) <= largest
    a = load_grads("only_dist")
    assert not a["d_reid64"].any() and a["d_node64"].any()
    assert "g_reid" in load_grads("terrace32")


def test_plan_restatement_gives_the_reference_edge_order():
    for name in CASES:
        a = load_grads(name)
        r = ggo.normalize(a["reid_embeds_raw"], np.float64)
        ei, _, _ = ggo.forward_attrs(r, a["id_cam"], a["graph_sizes"], np.float64)
        assert np.array_equal(ei, a["edge_index"]), name


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_autograd(name):
    a = load_grads(name)
    dn64, dr64 = ggo.graph_build_backward(a, np.float64)
    dn32, dr32 = ggo.graph_build_backward(a, np.float32)
    for key, g64, g32 in (("d_node", dn64, dn32), ("d_reid", dr64, dr32)):
        e64, e32, e_ref = rel_err(g64, a[key + "64"]), rel_err(g32, a[key + "64"]), rel_err(a[key + "32"], a[key + "64"])
        print(f"{name}: {key} e_oracle64 {e64:.3e}  e_oracle32 {e32:.3e}  e_ref {e_ref:.3e}")
        assert g64.shape == a[key + "64"].shape
        assert e64 <= 1e-12, (name, key, e64)
        assert e32 <= 4 * e_ref + EPS, (name, key, e32, e_ref)
    if name == "only_dist":
        assert not dr64.any()
    if name == "camera_only":   # no cross-camera partner: the gradient of the NORMALISED table is a zero row there
        r = ggo.normalize(a["reid_embeds_raw"], np.float64)
        _, emb, cos = ggo.forward_attrs(r, a["id_cam"], a["graph_sizes"], np.float64)
        d_r = ggo.edges_backward(r, emb, cos, a["g_edge_attr"][:, 2], a["g_edge_attr"][:, 3], a["id_cam"], a["graph_sizes"], np.float64)
        assert not d_r[-4:].any() and d_r[:-4].any()
