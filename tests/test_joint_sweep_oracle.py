"""The joint sweep (gnn_cca_amd.calibration.sweep_joint / sweep_grid / JointSweepAccumulator, gnn_cca_amd.baselines,
gnncca_eval_sweep_joint, gnncca_eval_rows_accumulate), the parts that need no GPU: the numpy restatement of the rule
(tests/joint_sweep_oracle.py) against the reference's own statements (tests/golden/calibration/geom_appearance.npz, made by
tests/golden/make_golden_geom.py from inference.py:896, :722-724, :899-908, :935-939); every host-side refusal before a device is touched
(host tensors stand in for the batch: a check that came too late would raise the module's "MI355X only" RuntimeError instead); header,
binding and library agree on the two entries; and the entries' own refusals come before any launch (the pointers are never followed)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_sweep_oracle as jo  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "calibration", "geom_appearance.npz")
TOL = {8: 1e-8, 9: 1e-12, 10: 1e-12, 11: 1e-12}      # tests/test_eval_oracle.py's: mutual_index, homogeneity, completeness, v_measure


def _same_partition(a, b):
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len(set(np.asarray(a).tolist())) == len(set(np.asarray(b).tolist()))


def test_oracle_equals_the_reference_statements():
    z = np.load(GOLDEN)
    ei, n = z["edge_index"], int(z["n_nodes"])
    e = ei.shape[1]
    assert n == 20 and e == 300 and z["geom"].dtype == np.float32 and z["reid"].dtype == np.float32
    geom_th, max_dist, reid_th = float(z["geom_th"]), float(z["max_dist"]), float(z["reid_th"])
    # the conditions the golden was made under: one value per unordered pair; float32 and float64 comparisons agree at both thresholds
    where = {(int(a), int(b)): k for k, (a, b) in enumerate(ei.T)}
    back = np.array([where[(int(b), int(a))] for a, b in ei.T])
    assert np.array_equal(z["geom"][back], z["geom"]) and np.array_equal(z["reid"][back], z["reid"])
    assert np.array_equal(z["geom"] < np.float32(geom_th / max_dist), z["geom"].astype(np.float64) < geom_th / max_dist)
    assert np.array_equal(z["reid"] < np.float32(reid_th), z["reid"].astype(np.float64) < reid_th)
    for scores, points, keep, div, name in (([z["geom"], z["reid"]], [[geom_th, reid_th]], ["lt", "lt"], [[max_dist], [1.0]], "joint"),
                                            ([z["geom"]], [[geom_th]], ["lt"], [[max_dist]], "geom")):
        rows, labels, kept = jo.sweep_joint(ei, z["edge_labels"], [0, n], [0, e], scores, points, keep, frame_div=div)
        assert np.array_equal(kept[0], z[f"pred_{name}"]), name                       # predictions: exact (pruning changes nothing here)
        assert _same_partition(labels[0], z[f"id_pred_{name}"]), name
        want = z[f"scores_{name}"]
        assert rows[0, 0, 7] == want[0], (name, rows[0, 0, 7], want[0])              # ARI: exact
        for q in (8, 9, 10, 11):
            assert abs(rows[0, 0, q] - want[q - 7]) <= TOL[q], (name, q, rows[0, 0, q], want[q - 7])
        assert rows[0, 0, 14] == len(set(z["id_gt"].tolist())) and rows[0, 0, 15] == len(set(z[f"id_pred_{name}"].tolist()))
        lab = z["edge_labels"]
        assert rows[0, 0, 3] == ((kept[0] == 1) & (lab == 1)).sum() and rows[0, 0, 4] == ((kept[0] == 1) & (lab == 0)).sum()
    # the oracle's comparators at a threshold equal to a score, NaN under all four, and the accumulation order
    s = np.array([0.25, 0.5, np.nan], dtype=np.float32)
    assert [jo.active_edges([s], [c], [0.5]).tolist() for c in ("ge", "gt", "le", "lt")] == [
        [False, True, False], [False, False, False], [True, True, False], [True, False, False]]
    r = np.random.default_rng(0).random((3, 5, 16)) * 1e3
    want = np.zeros((3, 16))
    for g in range(5):
        want = want + r[:, g]
    assert np.array_equal(jo.accumulate(np.zeros((3, 16)), r), want)


class _Batch:
    """What sweep_joint reads of a GraphBatch, on the host."""

    def __init__(self, sizes=(3, 2), e=8, attr_cols=4):
        self.node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        self.edge_ptr = [0, e // 2, e][:len(sizes) + 1]
        self.edge_index = torch.zeros((2, e), dtype=torch.int64)
        self.edge_labels = torch.zeros(e)
        self.edge_attr = torch.zeros((e, attr_cols))
        self.node_ptr_dev = torch.tensor(self.node_ptr, dtype=torch.int32)
        self.edge_ptr_dev = torch.tensor(self.edge_ptr, dtype=torch.int32)


def test_every_value_error_comes_before_the_gpu_is_touched():
    from gnn_cca_amd.baselines import geometry_baseline
    from gnn_cca_amd.calibration import MAX_POINTS, JointSweepAccumulator, grid_points, sweep_grid, sweep_joint
    assert MAX_POINTS == 16384
    b, s = _Batch(), torch.zeros(8)
    two = [s, s.view(-1, 1)]
    # scores
    for bad in ([], [s] * 5, [torch.zeros(7)], [s, None], [torch.zeros((4, 2))], torch.zeros(8), torch.zeros((5, 8)), torch.zeros((2, 7)), None, 3):
        with pytest.raises(ValueError):
            sweep_joint(b, bad, [[0.5]], ["ge"])
    # points
    for bad in ([], [0.5, 0.5], [[0.5]], [[0.5, 0.5, 0.5]], [[0.5, float("nan")]], [[float("inf"), 0.5]], None, [["a", "b"]], np.zeros((0, 2)),
                np.zeros((MAX_POINTS + 1, 2)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match="points"):
            sweep_joint(b, two, bad, ["lt", "lt"])
    # keep
    for bad in ("lt", None, ["lt"], ["lt", "lt", "lt"], ["lt", "eq"], ["lt", None], ["LT", "lt"], [0, 1], 7):
        with pytest.raises(ValueError, match="keep"):
            sweep_joint(b, two, [[0.5, 0.5]], bad)
    # frame_div: [K, G], finite, > 0; [G] only for K = 1
    for bad in ([1.0, 2.0], [[1.0, 2.0]], [[1.0], [2.0]], [[1.0, 2.0, 3.0]] * 2, [[1.0, 0.0], [1.0, 1.0]], [[1.0, -2.0], [1.0, 1.0]],
                [[1.0, float("nan")], [1.0, 1.0]], [[float("inf"), 1.0], [1.0, 1.0]], "x", [["a", "b"], ["c", "d"]]):
        with pytest.raises(ValueError, match="frame_div"):
            sweep_joint(b, two, [[0.5, 0.5]], ["lt", "lt"], frame_div=bad)
    with pytest.raises(ValueError, match="frame_div"):
        sweep_joint(b, [s], [[0.5]], ["lt"], frame_div=[1.0, 2.0, 3.0])
    # the batch
    short = _Batch()
    short.edge_labels = torch.zeros(5)
    with pytest.raises(ValueError, match="do not match"):
        sweep_joint(short, two, [[0.5, 0.5]], ["lt", "lt"])
    with pytest.raises(ValueError, match="at most 4096"):
        sweep_joint(_Batch(sizes=(4097, 2)), two, [[0.5, 0.5]], ["lt", "lt"])
    # what is left is a well-formed call on host tensors: the module's usual refusal
    for scores, pts, keep, div in ((two, [[0.5, 0.5]], ["lt", "ge"], None), ([s], [[0.5]], ["gt"], [2.0, 3.0]), (torch.zeros((3, 8)), np.zeros((4, 3)),
                                   ("le", "lt", "ge"), np.ones((3, 2))), ([b.edge_attr[:, 0], b.edge_attr[:, 2:3]], np.zeros((MAX_POINTS, 2)), ["lt", "lt"], None)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            sweep_joint(b, scores, pts, keep, frame_div=div)
    # sweep_grid: the product in C order, at most 16384 points
    pts, shape = grid_points([[0.1, 0.2], [1.0, 2.0, 3.0]])
    assert shape == (2, 3) and pts.tolist() == [[0.1, 1.0], [0.1, 2.0], [0.1, 3.0], [0.2, 1.0], [0.2, 2.0], [0.2, 3.0]]
    for bad in ([], [[0.1], []], [[[0.1]]], [np.zeros(129), np.zeros(128)], [[0.1]] * 5, None, [["a"]]):
        with pytest.raises(ValueError):
            sweep_grid(b, two, bad, ["lt", "lt"])
    with pytest.raises(ValueError, match="points"):
        sweep_grid(b, two, [[0.1, float("nan")], [0.2]], ["lt", "lt"])
    with pytest.raises(ValueError):
        sweep_grid(b, two, [[0.1, 0.2]], ["lt", "lt"])                      # one axis for two scores
    with pytest.raises(RuntimeError, match="MI355X only"):
        sweep_grid(b, two, [np.zeros(128), np.zeros(128)], ["lt", "lt"])     # 16384 points: the limit itself
    # JointSweepAccumulator
    for bad in ([], [0.5], [[]], [[0.1] * 5], [[float("nan")]], None, np.zeros((MAX_POINTS + 1, 1)), [["a"]]):
        with pytest.raises(ValueError):
            JointSweepAccumulator(bad)
    acc = JointSweepAccumulator([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    for bad in (torch.zeros((2, 4, 16), dtype=torch.float64), torch.zeros((3, 16), dtype=torch.float64), torch.zeros((3, 4, 16)),
                torch.zeros((3, 4, 15), dtype=torch.float64)):
        with pytest.raises(ValueError):
            acc.add(bad)
    with pytest.raises(RuntimeError, match="MI355X only"):
        acc.add(torch.zeros((3, 4, 16), dtype=torch.float64))
    with pytest.raises(ValueError, match="no rows"):
        acc.result()
    # geometry_baseline
    for batch, args, kw in ((_Batch(attr_cols=2), (1.0, [10.0, 10.0]), {}), (types_without_attr(), (1.0, [10.0, 10.0]), {}), (b, (1.0, [10.0]), {}),
                            (b, (1.0, [10.0, 0.0]), {}), (b, (1.0, [10.0, float("nan")]), {}), (b, (float("nan"), [10.0, 10.0]), {}),
                            (b, ("x", [10.0, 10.0]), {}), (b, (1.0, [10.0, 10.0]), {"reid_th": float("inf")}),
                            (b, (1.0, [10.0, 10.0]), {"reid_th": 0.5, "max_dist_l2": 0.0}), (b, (1.0, 10.0), {})):
        with pytest.raises(ValueError):
            geometry_baseline(batch, *args, **kw)
    for kw in ({}, {"reid_th": 0.4}, {"reid_th": 0.4, "max_dist_l2": 31.5}):
        with pytest.raises(RuntimeError, match="MI355X only"):
            geometry_baseline(b, 1.5, [20.0, 30.0], **kw)


def types_without_attr():
    b = _Batch()
    del b.edge_attr
    return b


def _declaration(header, name, result="int"):
    m = re.search(r"GNNCCA_API\s+" + result + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_binding_mirrors_them():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    lib = nat.lib()
    for name, result, res, count in (("gnncca_eval_sweep_joint_workspace_bytes", "size_t", C.c_size_t, 3),
                                     ("gnncca_eval_sweep_joint", "int", C.c_int, 20), ("gnncca_eval_rows_accumulate", "int", C.c_int, 6)):
        args = _declaration(header, name, result)
        got_res, argtypes = nat._SIGNATURES[name]
        assert len(args) == count == len(argtypes) and got_res is res, name
        assert name in nat.exported_symbols() and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(argtypes)
    names = [a.split()[-1].lstrip("*") for a in _declaration(header, "gnncca_eval_sweep_joint")]
    assert names == ["edge_index", "edge_labels", "scores", "score_strides", "comparators", "n_scores", "n_nodes", "n_edges", "node_ptr_dev",
                     "edge_ptr_dev", "n_frames", "max_frame_nodes", "points_dev", "n_points", "frame_div_dev", "rows_out", "labels_out",
                     "workspace", "workspace_bytes", "stream"]
    sig = nat._SIGNATURES["gnncca_eval_sweep_joint"][1]
    assert sig[3]._type_ is C.c_int64 and sig[4]._type_ is C.c_int32 and sig[5] is C.c_int32 and sig[13] is C.c_int32 and sig[18] is C.c_size_t
    assert [a.split()[-1].lstrip("*") for a in _declaration(header, "gnncca_eval_rows_accumulate")] == [
        "rows", "n_points", "n_frames", "sums", "frames", "stream"]
    assert "#define GNNCCA_EVAL_JOINT_MAX_SCORES 4" in header and nat.JOINT_MAX_SCORES == 4
    assert "#define GNNCCA_EVAL_JOINT_MAX_POINTS 16384" in header and nat.JOINT_MAX_POINTS == 16384
    codes = {k: int(v) for k, v in re.findall(r"#define GNNCCA_CMP_(\w+) (\d+)", header)}
    assert codes == {"GE": nat.CMP["ge"], "GT": nat.CMP["gt"], "LE": nat.CMP["le"], "LT": nat.CMP["lt"]} and len(set(codes.values())) == 4
    section = header[header.index("Joint sweep: every operating point"):header.index("gnncca_eval_sweep_joint_workspace_bytes(int64_t")]
    for word in ("threshold", "activity", "one IEEE fp64 division", "widened", "never active under any comparator", "strongly connected components",
                 "max_dist[0]", "ascending g", "no atomics"):
        assert word in section, word


def test_entry_points_refuse_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000
    n, e, g = 10, 24, 2
    ws = lib.gnncca_eval_sweep_joint_workspace_bytes(n, e, g)
    assert ws > 0 and ws % 256 == 0 and ws == lib.gnncca_eval_sweep_workspace_bytes(n, e, g, 1)     # O(E + N), no term in T or K
    for bad in ((-1, e, g), (n, -1, g), (n, e, -1)):
        assert lib.gnncca_eval_sweep_joint_workspace_bytes(*bad) == 0

    def call(k=2, t=5, max_n=6, ei=fake, el=fake, sc=(fake, fake, fake, fake), strides=(1, 4, 1, 1), cmps=(3, 3, 0, 2), nptr=fake, eptr=fake,
             pts=fake, div=None, rows=fake, work=fake, nbytes=ws, nn=n, ee=e, gg=g):
        ptrs = (C.c_void_p * 4)(*sc) if sc is not None else None
        st = (C.c_int64 * 4)(*strides) if strides is not None else None
        cm = (C.c_int32 * 4)(*cmps) if cmps is not None else None
        return lib.gnncca_eval_sweep_joint(ei, el, ptrs, st, cm, k, nn, ee, nptr, eptr, gg, max_n, pts, t, div, rows, None, work, nbytes, None)

    for k in (0, -1, 5, 1 << 20):
        assert call(k=k) == nat.ERR_INVALID_ARG, k
    for t in (0, -1, 16385, 1 << 30):
        assert call(t=t) == nat.ERR_INVALID_ARG, t
    for cmps in ((4, 0, 0, 0), (0, -1, 0, 0), (0, 99, 0, 0)):
        assert call(cmps=cmps) == nat.ERR_INVALID_ARG, cmps
    assert call(k=1, cmps=(3, 99, 0, 0), nbytes=ws - 1) == nat.ERR_WORKSPACE           # only the first K codes are read
    for strides in ((0, 1, 1, 1), (1, -4, 1, 1), (1, 0, 1, 1)):
        assert call(strides=strides) == nat.ERR_INVALID_ARG, strides
    assert call(sc=(fake, None, fake, fake)) == nat.ERR_INVALID_ARG and call(sc=(None, fake, fake, fake)) == nat.ERR_INVALID_ARG
    assert call(max_n=4097) == nat.ERR_INVALID_ARG and call(max_n=-1) == nat.ERR_INVALID_ARG
    for name in ("ei", "el", "sc", "strides", "cmps", "nptr", "eptr", "pts", "rows", "work"):
        assert call(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert call(nn=-1) == nat.ERR_INVALID_ARG and call(ee=-1) == nat.ERR_INVALID_ARG and call(gg=-1) == nat.ERR_INVALID_ARG
    assert call(nbytes=ws - 1) == nat.ERR_WORKSPACE and call(nbytes=0) == nat.ERR_WORKSPACE
    assert call(k=4, t=16384, div=fake, nbytes=ws - 1) == nat.ERR_WORKSPACE            # the limits themselves pass the argument checks
    assert call(gg=0, nptr=None, eptr=None, rows=None, work=None, nbytes=0) == nat.OK  # nothing to score: nothing launched
    assert call(gg=0, k=5) == nat.ERR_INVALID_ARG                                      # ... but the arguments are still judged

    acc = lib.gnncca_eval_rows_accumulate
    assert acc(fake, 0, 3, fake, fake, None) == nat.ERR_INVALID_ARG and acc(fake, 16385, 3, fake, fake, None) == nat.ERR_INVALID_ARG
    assert acc(fake, 4, -1, fake, fake, None) == nat.ERR_INVALID_ARG and acc(fake, 4, 3, None, fake, None) == nat.ERR_INVALID_ARG
    assert acc(None, 4, 3, fake, fake, None) == nat.ERR_INVALID_ARG
    assert acc(None, 4, 0, fake, None, None) == nat.OK                                 # no frame: nothing launched
