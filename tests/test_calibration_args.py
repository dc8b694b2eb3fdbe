"""gnn_cca_amd.calibration, the parts that need no GPU: every refusal comes before a device is touched (host tensors stand in for the
batch: a check that came too late would raise the module's "MI355X only" RuntimeError instead), the three new entry points are
exported, declared in the header and bound with matching argument counts, their own refusals come before any launch (the pointers are
never followed), SweepAccumulator.best returns every tied threshold, and the reference's sweep (tests/golden/calibration/reid_sweep.npz, made by
tests/golden/make_golden_sweep.py from main.py:141-175) is reproduced by compute_P_R_F's expressions on the stored counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "calibration", "reid_sweep.npz")


class _Batch:
    """What sweep_thresholds reads of a GraphBatch, on the host."""

    def __init__(self, sizes=(3, 2), e=8):
        self.node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        self.edge_ptr = [0, e // 2, e][:len(sizes) + 1]
        self.edge_index = torch.zeros((2, e), dtype=torch.int64)
        self.edge_labels = torch.zeros(e)
        self.node_ptr_dev = torch.tensor(self.node_ptr, dtype=torch.int32)
        self.edge_ptr_dev = torch.tensor(self.edge_ptr, dtype=torch.int32)


def test_every_value_error_comes_before_the_gpu_is_touched():
    from gnn_cca_amd.calibration import MAX_THRESHOLDS, SweepAccumulator, sweep_thresholds
    b, s = _Batch(), torch.zeros(8)
    assert MAX_THRESHOLDS == 1024
    for bad in ([], (), np.zeros(0), [[0.1, 0.2]], 0.5, None, ["a"], [0.1, float("nan")], [float("inf")], [-float("inf"), 0.2],
                np.linspace(0, 1, MAX_THRESHOLDS + 1)):
        with pytest.raises(ValueError):
            sweep_thresholds(b, s, bad)
        with pytest.raises(ValueError):
            SweepAccumulator(bad)
    for keep in ("gt", "lt", None, 0, "GE"):
        with pytest.raises(ValueError, match="keep"):
            sweep_thresholds(b, s, [0.5], keep=keep)
    with pytest.raises(ValueError, match="do not match"):
        sweep_thresholds(b, torch.zeros(7), [0.5])
    short = _Batch()
    short.edge_labels = torch.zeros(5)
    with pytest.raises(ValueError, match="do not match"):
        sweep_thresholds(short, s, [0.5])
    with pytest.raises(ValueError, match="at most 4096"):
        sweep_thresholds(_Batch(sizes=(4097, 2)), s, [0.5])
    # what is left is a well-formed call on host tensors: the module's usual refusal, for [E] and [E, 1] alike, in any order of thresholds
    for scores, ths, keep in ((s, [0.5], "ge"), (s.view(-1, 1), [0.9, 0.1, 0.9], "le"), (s, np.linspace(0, 1, MAX_THRESHOLDS), "ge")):
        with pytest.raises(RuntimeError, match="MI355X only"):
            sweep_thresholds(b, scores, ths, keep=keep)


def test_threshold_switch_is_validated_in_the_constructor_and_the_function():
    from gnn_cca_amd.pipeline import FramePipeline, FrameResult
    from gnn_cca_amd.postprocess import threshold

    class StandIn:
        """A model object the constructor only stores."""

    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), "0.3", None, True, [0.3]):
        with pytest.raises(ValueError):
            FramePipeline(StandIn(), threshold=bad)
        with pytest.raises(ValueError):
            threshold(torch.zeros(4), at=bad)
    assert FramePipeline(StandIn()).threshold == 0.5
    p = FramePipeline(StandIn(), threshold=np.float32(0.25))
    assert p.threshold == 0.25 and type(p.threshold) is float
    with pytest.raises(RuntimeError, match="MI355X only"):
        threshold(torch.zeros(4), at=0.3)
    assert callable(FrameResult.sweep) and "sweep" not in FrameResult.__slots__


def _declaration(header, name, result="int"):
    m = re.search(r"GNNCCA_API\s+" + result + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_binding_mirrors_them():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    lib = nat.lib()
    for name, result, res, count in (("gnncca_eval_sweep_workspace_bytes", "size_t", C.c_size_t, 4), ("gnncca_eval_sweep", "int", C.c_int, 17),
                                     ("gnncca_post_threshold_at", "int", C.c_int, 6)):
        args = _declaration(header, name, result)
        got_res, argtypes = nat._SIGNATURES[name]
        assert len(args) == count == len(argtypes) and got_res is res, name
        assert name in nat.exported_symbols() and hasattr(lib, name)
    args = _declaration(header, "gnncca_eval_sweep")
    assert [a.split()[-1].lstrip("*") for a in args[9:14]] == ["thresholds_dev", "n_thresholds", "keep_le", "rows_out", "labels_out"]
    assert nat._SIGNATURES["gnncca_post_threshold_at"][1][2] is C.c_double
    assert "#define GNNCCA_EVAL_SWEEP_MAX_THRESHOLDS 1024" in header and nat.SWEEP_MAX_THRESHOLDS == 1024
    assert "#define GNNCCA_ABI_VERSION 2" in header and nat.ABI_VERSION == 2
    # the rule is in the header in full
    for word in ("activity", "pruning", "partition", "widened fp32 score", "NaN score is never active", "duplicate ordered pairs"):
        assert word in header, word


def test_entry_points_refuse_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000
    n, e, g = 10, 24, 2
    ws = lib.gnncca_eval_sweep_workspace_bytes(n, e, g, 5)
    assert ws > 0 and ws % 256 == 0
    assert lib.gnncca_eval_sweep_workspace_bytes(n, e, g, 1000) == ws          # O(E + N): the thresholds cost no workspace
    assert lib.gnncca_eval_sweep_workspace_bytes(-1, e, g, 5) == 0

    def call(t=5, max_n=6, ei=fake, el=fake, sc=fake, nptr=fake, eptr=fake, th=fake, rows=fake, work=fake, nbytes=ws, nn=n, ee=e, gg=g):
        return lib.gnncca_eval_sweep(ei, el, sc, nn, ee, nptr, eptr, gg, max_n, th, t, 0, rows, None, work, nbytes, None)

    for t in (0, -1, 1025, 1 << 20):
        assert call(t=t) == nat.ERR_INVALID_ARG, t
    assert call(max_n=4097) == nat.ERR_INVALID_ARG and call(max_n=-1) == nat.ERR_INVALID_ARG
    for name in ("ei", "el", "sc", "nptr", "eptr", "th", "rows", "work"):
        assert call(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert call(nn=-1) == nat.ERR_INVALID_ARG and call(ee=-1) == nat.ERR_INVALID_ARG and call(gg=-1) == nat.ERR_INVALID_ARG
    assert call(nbytes=ws - 1) == nat.ERR_WORKSPACE
    assert call(gg=0, nptr=None, eptr=None, rows=None, work=None, nbytes=0) == nat.OK                  # nothing to score: nothing launched
    assert lib.gnncca_post_threshold_at(None, 4, 0.3, fake, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_post_threshold_at(fake, 4, 0.3, None, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_post_threshold_at(fake, -1, 0.3, fake, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_post_threshold_at(fake, 4, float("nan"), fake, fake, None) == nat.ERR_INVALID_ARG
    assert lib.gnncca_post_threshold_at(None, 0, 0.3, None, None, None) == nat.OK


def _rows_from_counts(tp, fp, fn, tn):
    """float64 [T, 1, 16] host rows carrying the counts (the other columns zero): what SweepAccumulator reads of a sweep."""
    rows = torch.zeros((len(tp), 1, 16), dtype=torch.float64)
    for col, v in ((3, tp), (4, fp), (5, fn), (6, tn)):
        rows[:, 0, col] = torch.from_numpy(np.asarray(v, dtype=np.float64))
    return rows


def test_best_returns_every_tied_threshold():
    from gnn_cca_amd.calibration import SweepAccumulator
    ths = [0.2, 0.4, 0.4, 0.6, 0.8]
    acc = SweepAccumulator(ths)
    # two batches, their counts summed; index 3 has nothing predicted (P = R = F = 0)
    acc.add(_rows_from_counts([1, 2, 3, 0, 4], [3, 0, 1, 0, 2], [3, 1, 1, 4, 0], [5, 5, 5, 5, 5]))
    acc.add(_rows_from_counts([1, 2, 1, 0, 0], [0, 1, 0, 0, 0], [2, 1, 0, 4, 0], [1, 1, 1, 1, 1]))
    assert len(acc) == 2
    res = acc.result()
    assert res is acc.result()
    assert res["TP"].tolist() == [2, 4, 4, 0, 4] and res["FP"].tolist() == [3, 1, 1, 0, 2] and res["FN"].tolist() == [5, 2, 1, 8, 0]
    assert res["TN"].tolist() == [6] * 5 and res["TP"].dtype == np.int64
    assert res["F_micro"][3] == 0.0 and res["P_micro"][3] == 0.0 and res["R_micro"][3] == 0.0
    assert res["F_micro"][1] == 2 * ((4 / 5) * (4 / 6)) / ((4 / 5) + (4 / 6))
    assert acc.best().tolist() == np.where(res["F_micro"] == res["F_micro"].max())[0].tolist() and 2 in acc.best().tolist()
    assert acc.best("R_micro").tolist() == [4] and acc.best("TN").tolist() == [0, 1, 2, 3, 4] and acc.best("FN").tolist() == [3]
    assert [a["TP"] for a in res["aggregates"]] == res["TP"].tolist() and sorted(res["aggregates"][0]) == sorted(
        ["P", "R", "F", "TP", "FP", "FN", "TN", "RI", "MI", "hom", "com", "v", "prec0", "prec1"])
    assert np.array_equal(acc.thresholds[acc.best("TN")], np.asarray(ths))
    with pytest.raises(ValueError):
        acc.best("accuracy")
    with pytest.raises(ValueError):
        acc.add(torch.zeros((4, 1, 16), dtype=torch.float64))      # another number of thresholds
    with pytest.raises(ValueError):
        acc.add(torch.zeros((5, 16), dtype=torch.float64))
    with pytest.raises(ValueError):
        acc.add(torch.zeros((5, 1, 16)))
    with pytest.raises(ValueError):
        SweepAccumulator(ths).result()
    # exact ties: equal counts at two thresholds give equal bits
    tie = SweepAccumulator([0.1, 0.2, 0.3]).add(_rows_from_counts([3, 1, 3], [1, 1, 1], [2, 4, 2], [0, 0, 0]))
    assert tie.best().tolist() == [0, 2]


def test_golden_counts_reproduce_the_reference_p_r_f_bit_for_bit():
    from gnn_cca_amd.calibration import SweepAccumulator
    z = np.load(GOLDEN)
    ths, f = z["thresholds"], z["F"]
    assert ths.shape == (100,) and ths.dtype == np.float64 and np.array_equal(ths, np.arange(0.01, 1.01, 0.01))
    e = z["edge_index"].shape[1]
    assert z["scores"].dtype == np.float32 and z["scores"].shape == (e,) and 200 <= e <= 1000
    assert np.all(z["TP"] + z["FP"] + z["FN"] + z["TN"] == e)
    # the condition the golden was made under: the float32 and the float64 comparison agree at every threshold
    for k, t in enumerate(ths):
        lo, hi = z["scores"] <= np.float32(t), z["scores"].astype(np.float64) <= t
        assert np.array_equal(lo, hi), t
        lab = z["edge_labels"]
        assert (int((hi & (lab == 1)).sum()), int((hi & (lab == 0)).sum())) == (int(z["TP"][k]), int(z["FP"][k])), t
    # both directions of a pair carry one distance: pruning single-direction edges changes nothing at any threshold
    where = {(int(a), int(b)): k for k, (a, b) in enumerate(z["edge_index"].T)}
    back = np.array([where[(int(b), int(a))] for a, b in z["edge_index"].T])
    assert np.array_equal(z["scores"][back], z["scores"]) and np.array_equal(z["edge_labels"][back], z["edge_labels"])
    acc = SweepAccumulator(ths).add(_rows_from_counts(z["TP"], z["FP"], z["FN"], z["TN"]))
    res = acc.result()
    for name, key in (("P", "P_micro"), ("R", "R_micro"), ("F", "F_micro")):
        assert np.array_equal(res[key], z[name]), name      # bit for bit
    assert np.array_equal(acc.best(), np.where(f == np.max(f))[0])
    assert 0 < f.max() < 1 and 0 < int(np.argmax(f)) < 99       # the optimum is inside the swept range
