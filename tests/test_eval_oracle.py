"""The host restatement of the per-frame metrics (tests/helpers/eval_oracle.py) against the reference's own scoring (goldens of
tests/golden/make_golden_eval.py) and live scikit-learn where it is installed; the C ABI of gnncca_eval_frames refuses bad arguments before
any launch (no device needed); the column order of gnn_cca_amd.evaluation.METRICS."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import eval_oracle as eo  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = {"mutual_index": 1e-8, "homogeneity": 1e-12, "completeness": 1e-12, "v_measure": 1e-12}


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def check_row(got, want, where):
    for q, name in enumerate(eo.COLUMNS[:len(want)]):
        if name in TOL:
            assert abs(got[q] - want[q]) <= TOL[name], (where, name, got[q], want[q])
        else:
            assert got[q] == want[q], (where, name, got[q], want[q])


def frames_of(name):
    z = np.load(os.path.join(GOLDEN, name))
    nptr, eptr = z["node_ptr"].astype(np.int64), z["edge_ptr"].astype(np.int64)
    for g in range(len(nptr) - 1):
        v0, v1, k0, k1 = nptr[g], nptr[g + 1], eptr[g], eptr[g + 1]
        yield g, dict(n=int(v1 - v0), src=z["src"][k0:k1].astype(np.int64), dst=z["dst"][k0:k1].astype(np.int64),
                      lab=z["edge_labels"][k0:k1].astype(np.float32), pred=z["predictions"][k0:k1].astype(np.int64),
                      id_gt=z["id_gt"][v0:v1].astype(np.int64), id_pred=z["id_pred"][v0:v1].astype(np.int64), metrics=z["metrics"][g])


@pytest.mark.parametrize("fixture", ["post2_eval_frames.npz", "post2_eval_partitions.npz"])
def test_restatement_equals_the_reference_goldens(fixture):
    count = 0
    for g, f in frames_of(fixture):
        row, gt = eo.eval_frame(f["src"], f["dst"], f["lab"], f["pred"], f["id_pred"], f["n"])
        check_row(row, f["metrics"], (fixture, g))
        assert same_partition(gt, f["id_gt"]), (fixture, g)
        assert row[14] == len(set(f["id_gt"].tolist())) and row[15] == len(set(f["id_pred"].tolist()))
        count += 1
    assert count >= 13


def test_restatement_equals_live_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for n, k, kp in ((3, 2, 2), (20, 6, 7), (64, 10, 3), (300, 40, 55), (777, 5, 200), (50, 1, 4), (50, 4, 1), (40, 40, 40)):
        t, p = rng.integers(0, k, size=n), rng.integers(0, kp, size=n)
        ari, ami, h, c, v = eo.cluster_scores(t, p)
        assert ari == metrics.adjusted_rand_score(t, p)
        assert abs(ami - metrics.adjusted_mutual_info_score(t, p)) <= 1e-10
        for got, want in zip((h, c, v), metrics.homogeneity_completeness_v_measure(t, p)):
            assert abs(got - want) <= 1e-12


def test_metrics_columns():
    from gnn_cca_amd.evaluation import METRICS
    assert METRICS == ("P", "R", "F", "TP", "FP", "FN", "TN", "rand_index", "mutual_index", "homogeneity", "completeness", "v_measure",
                       "precision0", "precision1", "n_clusters_gt", "n_clusters_pred") == eo.COLUMNS
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    cols = " ".join(re.findall(r'"([^"]*)"', header[header.index("#define GNNCCA_EVAL_COLUMNS"):].split("\nGNNCCA_API")[0])).split()
    assert tuple(cols) == METRICS
    assert "#define GNNCCA_EVAL_MAX_FRAME_NODES 4096" in header


def test_aggregate_matches_main_py():
    rows = np.random.default_rng(0).random((9, 16))
    rows[:, 3:7] = np.round(rows[:, 3:7] * 100)
    agg = eo.aggregate(rows)
    assert agg["TP"] == int(rows[:, 3].sum()) and agg["P"] == float(np.mean(rows[:, 0])) and agg["prec1"] == float(np.mean(rows[:, 13]))
    assert sorted(agg) == sorted(["P", "R", "F", "TP", "FP", "FN", "TN", "RI", "MI", "hom", "com", "v", "prec0", "prec1"])


def test_eval_frames_refuses_bad_arguments_before_any_launch():
    """Argument checks come first: the pointers are never followed and no device is needed."""
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    n, e, g = 40, 100, 3
    fake = 0x10000
    need = lib.gnncca_eval_workspace_bytes(n, e, g)
    assert need >= 8 * (n + g) and lib.gnncca_eval_workspace_bytes(-1, e, g) == 0

    def call(**kw):
        a = dict(ei=fake, el=fake, pr=fake, lb=fake, n=n, e=e, nptr=fake, eptr=fake, g=g, maxn=20, gt=None, out=fake, ws=fake, wsb=need)
        a.update(kw)
        return lib.gnncca_eval_frames(a["ei"], a["el"], a["pr"], a["lb"], a["n"], a["e"], a["nptr"], a["eptr"], a["g"], a["maxn"], a["gt"],
                                      a["out"], a["ws"], a["wsb"], None)

    for k in ("ei", "el", "pr", "lb", "nptr", "eptr", "out", "ws"):
        assert call(**{k: None}) == nat.ERR_INVALID_ARG, k
    assert call(maxn=4097, n=5000) == nat.ERR_INVALID_ARG
    assert call(maxn=-1) == nat.ERR_INVALID_ARG
    assert call(n=-1) == nat.ERR_INVALID_ARG and call(g=-1) == nat.ERR_INVALID_ARG
    assert call(wsb=need - 1) == nat.ERR_WORKSPACE and call(wsb=0) == nat.ERR_WORKSPACE
    assert call(g=0) == nat.OK          # nothing to score: nothing launched


def test_evaluate_frames_refuses_a_frame_above_the_cap_before_launch():
    import torch
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.sharding import GraphBatch
    b = GraphBatch(None, torch.zeros((2, 0), dtype=torch.int64), None, [0, 0], [0, 4097])
    b.edge_labels = torch.zeros(0)
    with pytest.raises(ValueError, match="at most 4096"):
        evaluate_frames(b, torch.zeros(0, dtype=torch.int64), torch.zeros(4097, dtype=torch.int32))
