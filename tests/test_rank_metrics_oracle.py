"""gnn_cca_amd.ranking, the parts that need no GPU: the numpy oracle of the ranking rule (tests/rank_metrics_oracle.py) against
scikit-learn and against hand cases with known answers; the pooled oracle against the reference's own sweep
(tests/golden/calibration/reid_sweep.npz, main.py:141-175); the host reduction of a pooled curve against the oracle; the entry points
declared, bound and refusing before any launch; and every ValueError of the module before a device is touched (host tensors stand in for
the batch: a check that came too late would raise the module's "MI355X only" RuntimeError instead)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import rank_metrics_oracle as ro  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "calibration", "reid_sweep.npz")


def _draw(rng, e, how):
    labels = (rng.random(e) < rng.uniform(0.05, 0.6)).astype(np.float32)
    if labels.min() == labels.max():
        labels[0], labels[-1] = 0.0, 1.0
    if how == "continuous":
        s = rng.standard_normal(e) + 0.7 * labels
    elif how == "seven values":
        s = rng.choice(np.array([-2.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.0]), size=e) + 0.0
    else:   # barely separated: neighbouring float32 values around 1
        s = np.float32(1.0) + rng.integers(0, 40, size=e).astype(np.float32) * np.float32(2.0 ** -23)
    return s.astype(np.float32), labels


def test_oracle_agrees_with_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    sizes = [2, 3, 17, 64, 255, 256, 257, 1000, 4097, 16380]
    worst = {"AUROC": 0.0, "AP": 0.0}
    for how in ("continuous", "seven values", "barely separated"):
        for e in sizes + [int(x) for x in rng.integers(2, 3000, size=12)]:
            s, labels = _draw(rng, e, how)
            for low in (False, True):
                row = ro.rank_row(s, labels, low)
                sk = (-s if low else s).astype(np.float64)
                want_auc, want_ap = metrics.roc_auc_score(labels, sk), metrics.average_precision_score(labels, sk)
                # each side adds at most E <= 16384 terms <= 1 with one rounding each: 2 * 16384 * 2^-52 = 7.3e-12
                assert abs(row[4] - want_auc) <= 1e-11, (how, e, low, row[4], want_auc)
                assert abs(row[5] - want_ap) <= 1e-11, (how, e, low, row[5], want_ap)
                worst["AUROC"] = max(worst["AUROC"], abs(row[4] - want_auc))
                worst["AP"] = max(worst["AP"], abs(row[5] - want_ap))
                assert row[0] == labels.sum() and row[1] == e - labels.sum() and row[3] == 0
                assert row[2] == len(np.unique(np.where(s == 0, np.float32(0), s)))
                if e > 1000:
                    continue
                # best_F: brute force over the distinct cuts
                cuts = np.unique(s)
                f = []
                for c in cuts:
                    pred = s <= c if low else s >= c
                    tp, fp, fn = (pred & (labels == 1)).sum(), (pred & (labels == 0)).sum(), (~pred & (labels == 1)).sum()
                    P = tp / (tp + fp) if (tp + fp) != 0 else 0
                    R = tp / (tp + fn) if (tp + fn) != 0 else 0
                    f.append(2 * (P * R) / (P + R) if (P + R) != 0 else 0)
                f = np.array(f)
                assert row[6] == f.max(), (how, e, low)
                first = cuts[f == f.max()].min() if low else cuts[f == f.max()].max()      # the most positive of the best cuts
                assert row[7] == np.float64(first), (how, e, low, row[7], first)
    print("largest |oracle - sklearn|:", worst)


def _row(s, labels, low=False):
    return ro.rank_row(np.array(s, dtype=np.float32), np.array(labels, dtype=np.float32), low)


def test_hand_cases():
    nan = float("nan")
    assert _row([0.9, 0.8, 0.2, 0.1], [1, 1, 0, 0]).tolist() == [2, 2, 4, 0, 1.0, 1.0, 1.0, np.float64(np.float32(0.8))]      # perfect
    rev = _row([0.9, 0.8, 0.2, 0.1], [0, 0, 1, 1])
    assert rev[4] == 0.0 and rev[5] == (0.5 * (1 / 3)) + (0.5 * (2 / 4)) and rev[6] == 2 * (0.5 * 1.0) / 1.5                 # reversed
    assert rev[7] == np.float64(np.float32(0.1))
    low = _row([0.9, 0.8, 0.2, 0.1], [0, 0, 1, 1], low=True)                                                                  # ... as distances
    assert low.tolist() == [2, 2, 4, 0, 1.0, 1.0, 1.0, np.float64(np.float32(0.2))]
    tied = _row([0.5] * 10, [1, 0, 0, 1, 0, 0, 0, 1, 0, 0])                                                                   # all tied
    assert tied.tolist() == [3, 7, 1, 0, 0.5, 0.3, 2 * (0.3 * 1.0) / 1.3, 0.5]
    zeros = _row([0.0, -0.0], [1, 0])                                                                                          # +0 and -0 tie
    assert zeros[2] == 1 and zeros[4] == 0.5 and zeros[5] == 0.5 and zeros[7] == 0.0 and not np.signbit(zeros[7])
    assert not np.signbit(_row([0.0, -0.0], [1, 0], low=True)[7])
    only_pos = _row([0.3, 0.1, 0.2], [1, 1, 1])
    assert only_pos[:4].tolist() == [3, 0, 3, 0] and np.isnan(only_pos[4]) and abs(only_pos[5] - 1.0) < 1e-15 and only_pos[6] == 1.0
    assert only_pos[7] == np.float64(np.float32(0.1))
    only_neg = _row([0.3, 0.1, 0.1], [0, 0, 0])
    assert only_neg[:4].tolist() == [0, 3, 2, 0] and np.isnan(only_neg[4:]).all()
    empty = _row([], [])
    assert empty[:4].tolist() == [0, 0, 0, 0] and np.isnan(empty[4:]).all()
    one_nan = _row([0.3, nan, 0.1, 0.1], [1, 1, 0, 0])
    assert one_nan[:4].tolist() == [2, 2, 2, 1] and np.isnan(one_nan[4:]).all()
    inf = _row([np.inf, 1.0, -np.inf, -1.0], [1, 0, 0, 1])                                                                     # +-inf: ordinary values
    assert inf[:4].tolist() == [2, 2, 4, 0] and inf[4] == 0.75 and inf[6] == 2 * ((2 / 3) * 1.0) / ((2 / 3) + 1.0) and inf[7] == -1.0
    assert _row([0.3, 0.2, 0.1], [1, 2, 0])[:4].tolist() == [1, 1, 2, 0]                                                       # a label of 2: no sample
    # the lanes of AP's order: 300 perfectly ranked positives in front of 300 negatives, one term per position
    s = np.arange(600, 0, -1, dtype=np.float32)
    lab = (np.arange(600) < 300).astype(np.float32)
    assert _row(s, lab)[5] == ro.ap_sum(np.concatenate([np.full(300, 1.0 / 300.0), np.zeros(300)])) and abs(_row(s, lab)[5] - 1.0) < 1e-13


def test_pooled_oracle_reproduces_the_reference_sweep_and_the_host_reduction_is_the_oracle():
    from gnn_cca_amd.ranking import curve_from_histograms
    z = np.load(GOLDEN)
    hist, nans = ro.pooled_histograms(z["scores"], z["edge_labels"], z["thresholds"], "le")
    assert nans == (0, 0) and hist.sum() == len(z["scores"])
    got = ro.pooled_rows(hist, "le")
    for name in ("TP", "FP", "FN", "TN"):
        assert np.array_equal(got[name], z[name]), name
    for name in ("P", "R", "F"):
        assert got[name].tobytes() == np.asarray(z[name], dtype=np.float64).tobytes(), name        # bit for bit
    rng = np.random.default_rng(8)
    s = rng.standard_normal(5000).astype(np.float32)
    s[::50] = 0.25                                                                                 # scores ON a threshold
    lab = (rng.random(5000) < 0.3).astype(np.float32)
    th = np.sort(np.unique(np.concatenate([rng.standard_normal(40), [0.25]])))
    for keep in ("le", "ge"):
        hist, _ = ro.pooled_histograms(s, lab, th, keep)
        want, got = ro.pooled_rows(hist, keep), curve_from_histograms(hist, keep)
        for t, v in enumerate(th):                                                                 # the histograms ARE the comparisons
            pred = s.astype(np.float64) <= v if keep == "le" else s.astype(np.float64) >= v
            assert want["TP"][t] == (pred & (lab == 1)).sum() and want["FP"][t] == (pred & (lab == 0)).sum(), (keep, t)
        for name in ("TP", "FP", "FN", "TN", "P", "R", "F"):
            assert got[name].tobytes() == want[name].tobytes() and got[name].dtype == want[name].dtype, (keep, name)
        assert got["AUROC"] == want["AUROC"] and got["AP"] == want["AP"] and 0.3 < got["AUROC"] < 0.7
        # the quantised score's AUROC / AP are those of the bucket index as a score
        b = np.searchsorted(th, s.astype(np.float64), side="left" if keep == "le" else "right")
        row = ro.rank_row(b.astype(np.float32), lab, low=keep == "le")
        assert row[4] == want["AUROC"] and abs(row[5] - want["AP"]) <= 1e-12


class _Batch:
    """What rank_metrics and PooledCurve.add read of a GraphBatch, on the host."""

    def __init__(self, frame_edges=(4, 4)):
        self.edge_ptr = np.concatenate([[0], np.cumsum(frame_edges)]).tolist()
        e = self.edge_ptr[-1]
        self.node_ptr = list(range(len(frame_edges) + 1))
        self.edge_index = torch.zeros((2, e), dtype=torch.int64)
        self.edge_labels = torch.zeros(e)
        self.edge_ptr_dev = torch.tensor(self.edge_ptr, dtype=torch.int32)


def test_every_value_error_comes_before_the_gpu_is_touched():
    from gnn_cca_amd.ranking import MAX_POOL_THRESHOLDS, MAX_RANK_FRAME_EDGES, RANK_COLUMNS, PooledCurve, RankMeter, rank_metrics
    assert RANK_COLUMNS == ro.COLUMNS and MAX_RANK_FRAME_EDGES == 16384 and MAX_POOL_THRESHOLDS == 65536
    b, s = _Batch(), torch.zeros(8)
    for bad in ("up", None, 0, ["high", "low"], [], ["high", "down"]):
        with pytest.raises(ValueError, match="positive"):
            rank_metrics(b, s, bad)
    with pytest.raises(ValueError, match="positive"):
        rank_metrics(b, [s, s], ["high"])
    with pytest.raises(ValueError, match="1 to 4"):
        rank_metrics(b, [s] * 5)
    with pytest.raises(ValueError, match="1 to 4"):
        rank_metrics(b, [])
    for wrong in (torch.zeros(7), torch.zeros(8, 2), [s, torch.zeros(9)], [s, np.zeros(8)]):
        with pytest.raises(ValueError, match="does not match"):
            rank_metrics(b, wrong)
    short = _Batch()
    short.edge_labels = torch.zeros(5)
    with pytest.raises(ValueError, match="do not match"):
        rank_metrics(short, s)
    big = _Batch(frame_edges=(3, 16385))
    with pytest.raises(ValueError, match="at most 16384"):
        rank_metrics(big, torch.zeros(16388))
    # what is left is a well-formed call on host tensors: the module's usual refusal
    ok = _Batch(frame_edges=(16384, 4))
    for scores, positive in ((s, "high"), (s.view(-1, 1), "low"), ([s, s, s, s], ["high", "low", "low", "high"])):
        with pytest.raises(RuntimeError, match="MI355X only"):
            rank_metrics(b, scores, positive)
    with pytest.raises(RuntimeError, match="MI355X only"):
        rank_metrics(ok, torch.zeros(16388))
    for bad in ([], [[0.1, 0.2]], 0.5, None, ["a"], [0.1, float("nan")], [0.1, float("inf")], [0.2, 0.1], [0.1, 0.1], [0.1, 0.3, 0.2],
                np.arange(MAX_POOL_THRESHOLDS + 1)):
        with pytest.raises(ValueError, match="thresholds"):
            PooledCurve(bad)
    for keep in ("lt", "gt", None, 0):
        with pytest.raises(ValueError, match="keep"):
            PooledCurve([0.5], keep=keep)
    curve = PooledCurve(np.arange(MAX_POOL_THRESHOLDS), keep="ge")
    assert curve.thresholds.dtype == np.float64 and PooledCurve([0.5]).keep == "le"
    with pytest.raises(ValueError, match="do not match"):
        curve.add(b, torch.zeros(7))
    with pytest.raises(ValueError, match="do not match"):
        curve.add_raw(torch.zeros(7), torch.zeros(8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        curve.add(b, s)
    with pytest.raises(ValueError, match="nothing was added"):
        curve.result()
    meter = RankMeter()
    for bad in (torch.zeros((1, 2, 8)), torch.zeros((2, 8), dtype=torch.float64), torch.zeros((5, 2, 8), dtype=torch.float64),
                torch.zeros((1, 2, 16), dtype=torch.float64), None):
        with pytest.raises(ValueError, match="RankMeter.add"):
            meter.add(bad)
    with pytest.raises(RuntimeError, match="MI355X only"):
        meter.add(torch.zeros((1, 2, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="no rows"):
        meter.result()
    from gnn_cca_amd.pipeline import FrameResult
    assert callable(FrameResult.rank_metrics) and "rank_metrics" not in FrameResult.__slots__


def _declaration(header, name, result="int"):
    m = re.search(r"GNNCCA_API\s+" + result + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_they_refuse_before_any_launch():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    lib = nat.lib()
    for name, result, res, count in (("gnncca_rank_metrics_lds_bytes", "size_t", C.c_size_t, 1), ("gnncca_rank_metrics", "int", C.c_int, 11),
                                     ("gnncca_rank_rows_accumulate", "int", C.c_int, 6), ("gnncca_rank_pool_add", "int", C.c_int, 10)):
        args = _declaration(header, name, result)
        got_res, argtypes = nat._SIGNATURES[name]
        assert len(args) == count == len(argtypes) and got_res is res, name
        assert name in nat.exported_symbols() and hasattr(lib, name)
    assert "#define GNNCCA_RANK_MAX_FRAME_EDGES 16384" in header and nat.RANK_MAX_FRAME_EDGES == 16384
    assert "#define GNNCCA_RANK_MAX_SCORES 4" in header and nat.RANK_MAX_SCORES == 4
    assert "#define GNNCCA_RANK_POOL_MAX_THRESHOLDS 65536" in header and nat.RANK_POOL_MAX_THRESHOLDS == 65536
    assert '"' + ",".join(ro.COLUMNS) + '"' in header
    for word in ("-0 is taken as +0", "ONE tie group", "neg_ranked_below", "never fused", "o = 32, 16, 8, 4, 2, 1", "FIRST cut", "n_nan"):
        assert word in header, word                                                    # the rule is in the header in full
    # LDS by the largest frame: three capacities' worth of sizes
    assert [lib.gnncca_rank_metrics_lds_bytes(n) for n in (0, 64, 65, 768, 1024, 1025, 4096, 4097, 16384)] == \
        [512, 512, 1024, 8192, 8192, 16384, 32768, 65536, 131072]
    assert lib.gnncca_rank_metrics_lds_bytes(16385) == 0 and lib.gnncca_rank_metrics_lds_bytes(-1) == 0
    fake = 0x10000

    def call(k=2, e=100, g=3, max_e=40, el=fake, eptr=fake, rows=fake, ptrs=(fake, fake), strides=(1, 4), low=(0, 1)):
        return lib.gnncca_rank_metrics(el, (C.c_void_p * 4)(*ptrs), (C.c_int64 * 4)(*strides), (C.c_int32 * 4)(*low), k, e, eptr, g, max_e, rows, None)

    for k in (0, -1, 5):
        assert call(k=k) == nat.ERR_INVALID_ARG, k
    assert call(max_e=16385) == nat.ERR_INVALID_ARG and call(max_e=-1) == nat.ERR_INVALID_ARG and call(max_e=101) == nat.ERR_INVALID_ARG
    assert call(strides=(1, 0)) == nat.ERR_INVALID_ARG and call(low=(0, 2)) == nat.ERR_INVALID_ARG and call(ptrs=(fake, None)) == nat.ERR_INVALID_ARG
    for name in ("el", "eptr", "rows"):
        assert call(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert call(e=-1) == nat.ERR_INVALID_ARG and call(g=-1) == nat.ERR_INVALID_ARG
    assert call(g=0, eptr=None, rows=None) == nat.OK                                               # nothing to rank: nothing launched
    assert lib.gnncca_rank_rows_accumulate(fake, 0, 3, fake, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_rank_rows_accumulate(fake, 5, 3, fake, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_rank_rows_accumulate(None, 2, 3, fake, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_rank_rows_accumulate(fake, 2, 3, None, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_rank_rows_accumulate(None, 2, 0, fake, fake, None) == nat.OK

    def pool(sc=fake, stride=1, lab=fake, n=50, th=fake, t=100, hist=fake, nans=fake):
        return lib.gnncca_rank_pool_add(sc, stride, lab, n, th, t, 1, hist, nans, None)

    for t in (0, -1, 65537):
        assert pool(t=t) == nat.ERR_INVALID_ARG, t
    for name in ("sc", "lab", "th", "hist", "nans"):
        assert pool(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert pool(stride=0) == nat.ERR_INVALID_ARG and pool(n=-1) == nat.ERR_INVALID_ARG
    assert pool(n=0, sc=None, lab=None) == nat.OK
