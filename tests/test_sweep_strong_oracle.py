"""The sweep over the strongly connected clusters (calibration.sweep_thresholds / sweep_joint / sweep_grid with partition='strong',
baselines.geometry_baseline(partition='strong'), gnncca_eval_sweep_strong), the parts that need no GPU:

  * the numpy restatement of the rule (tests/sweep_strong_oracle.py) against the reference's own partitions at threshold 0.5
    (tests/golden/post_unpruned.npz: id_unpruned / pred_unpruned);
  * the input condition of the GPU tests: on the golden frames the strong partition is NOT the mutual-pair components at the swept thresholds;
  * header, binding and library agree on the two new symbols;
  * every ValueError before a device is touched (host tensors stand in for the batch: a check that came too late would raise the module's
    "MI355X only" RuntimeError instead);
  * the entry's refusals before any launch (the pointers are never followed)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import sweep_strong_oracle as so  # noqa: E402
from oracle import post_oracle as po  # noqa: E402


def test_restatement_equals_the_reference_partitions_at_one_half():
    frames = so.golden_frames()
    assert len(frames) == 26
    b = so.golden_batch(frames)
    rows, labels, preds = so.sweep_strong(b["edge_index"], b["edge_labels"], b["node_ptr"], b["edge_ptr"], [b["probs"]], [[0.5]], ["ge"])
    for g, (name, n, ei, probs, get) in enumerate(frames):
        v0, k0, k1 = b["node_ptr"][g], b["edge_ptr"][g], b["edge_ptr"][g + 1]
        assert np.array_equal(preds[0, k0:k1], get("pred_unpruned")), name                 # nothing is pruned
        lab = labels[0, v0:v0 + n] - v0
        assert po.same_partition(lab, get("id_unpruned")), name
        assert all(lab[v] == min(u for u in range(n) if lab[u] == lab[v]) for v in range(n)), name   # the label convention
        assert rows[0, g, 15] == len(set(get("id_unpruned").tolist())), name
        assert rows[0, g, 3] + rows[0, g, 4] == get("pred_unpruned").sum(), name           # TP + FP = the predicted edges
    # one frame alone gives the frame's row of the batch (frames are independent)
    one = so.golden_batch(frames[3:4], seed=0)
    r1, l1, _ = so.sweep_strong(one["edge_index"], one["edge_labels"], one["node_ptr"], one["edge_ptr"], [one["probs"]], [[0.5]], ["ge"])
    assert po.same_partition(l1[0], frames[3][4]("id_unpruned"))
    # 'le' on 1 - p is not 'ge' on p bit for bit in float32, but the comparators themselves are exact in float64
    s = np.array([0.25, 0.5, np.nan, -0.0], dtype=np.float32)
    ei = np.array([[0, 1, 2, 0], [1, 2, 0, 2]])
    for keep, th, want in (("ge", 0.5, [0, 1, 0, 0]), ("gt", 0.5, [0, 0, 0, 0]), ("le", 0.5, [1, 1, 0, 1]), ("lt", 0.5, [1, 0, 0, 1]),
                           ("ge", 0.0, [1, 1, 0, 1]), ("gt", 0.0, [1, 1, 0, 0]), ("le", 0.0, [0, 0, 0, 1]), ("lt", 0.0, [0, 0, 0, 0])):
        _, _, p = so.sweep_strong(ei, np.zeros(4, np.float32), [0, 3], [0, 4], [s], [[th]], [keep])
        assert p[0].tolist() == want, (keep, th)
    # a 3-cycle: one cluster; frame_div divides the point
    cyc = np.array([[0, 1, 2], [1, 2, 0]])
    sc = np.array([0.9, 0.8, 0.7], dtype=np.float32)
    rows, labels, p = so.sweep_strong(cyc, np.ones(3, np.float32), [0, 3], [0, 3], [sc], [[1.2], [1.5]], ["ge"], frame_div=[[2.0]])
    assert labels.tolist() == [[0, 0, 0], [0, 1, 2]] and p.tolist() == [[1, 1, 1], [1, 1, 0]]


@pytest.mark.parametrize("th", [0.35, 0.5, 0.65, 0.8])
def test_input_condition_strong_differs_from_mutual_pairs_on_the_golden(th):
    """Measured when the sweep was written: 19 / 21 / 20 / 20 of the 26 frames differ at 0.35 / 0.5 / 0.65 / 0.8."""
    differ = 0
    for name, n, ei, probs, _ in so.golden_frames():
        pred = (probs.astype(np.float64) >= th).astype(np.int64)
        _, lab, _ = so.sweep_strong(ei, np.zeros(ei.shape[1], np.float32), [0, n], [0, ei.shape[1]], [probs], [[th]], ["ge"])
        mutual = po.clusters(ei, po.prune(ei, pred), n)[0] if ei.size else np.arange(n)
        differ += not po.same_partition(lab[0], mutual)
    print(f"threshold {th}: the strong partition differs from the mutual-pair components on {differ} of 26 frames")
    assert differ >= 15, (th, differ)


# ---- header, binding, export ----------------------------------------------------------------------------------------------------------
def _declaration(header, name, result="int"):
    m = re.search(r"GNNCCA_API\s+" + result + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_binding_mirrors_them():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    lib = nat.lib()
    for name, result, res, count in (("gnncca_eval_sweep_strong_workspace_bytes", "size_t", C.c_size_t, 3),
                                     ("gnncca_eval_sweep_strong", "int", C.c_int, 20)):
        args = _declaration(header, name, result)
        got_res, argtypes = nat._SIGNATURES[name]
        assert len(args) == count == len(argtypes) and got_res is res, name
        assert name in nat.exported_symbols() and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(argtypes)
    # gnncca_eval_sweep_joint's argument list, name for name and type for type
    strip = lambda decl: [a.split()[-1].lstrip("*") for a in decl]   # noqa: E731
    assert strip(_declaration(header, "gnncca_eval_sweep_strong")) == strip(_declaration(header, "gnncca_eval_sweep_joint"))
    assert list(nat._SIGNATURES["gnncca_eval_sweep_strong"][1]) == list(nat._SIGNATURES["gnncca_eval_sweep_joint"][1])
    assert [a.split()[0] for a in _declaration(header, "gnncca_eval_sweep_strong_workspace_bytes", "size_t")] == ["int64_t", "int64_t", "int32_t"]
    assert nat._SIGNATURES["gnncca_eval_sweep_strong_workspace_bytes"][1] == [C.c_int64, C.c_int64, C.c_int32]
    section = header[header.index("Sweep over the STRONGLY CONNECTED clusters"):header.index("gnncca_eval_sweep_strong_workspace_bytes(int64_t")]
    for word in ("threshold", "active edges", "predictions", "labels", "row", "one IEEE", "widened", "NaN", "No reverse edge is consulted",
                 "UNPRUNED", "smallest batch-global id", "leaves its frame sets no bit", "elf loops and duplicates are harmless", "any order",
                 "bit for bit", "TWO launches", "ceil(log2(n_pad)) + 1", "GNNCCA_STRONG_MAX_FRAME_NODES"):
        assert re.sub(r"\s*\n \*\s*", " ", section).count(word), word
    from gnn_cca_amd import calibration
    assert calibration.SWEEP_PARTITIONS == ("components", "exclusive", "strong") and calibration.JOINT_PARTITIONS == ("components", "strong")


# ---- every host-side refusal, no device touched ---------------------------------------------------------------------------------------
class _Batch:
    """What the sweeps read of a GraphBatch, on the host."""

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
    from gnn_cca_amd.calibration import sweep_grid, sweep_joint, sweep_thresholds
    b, s = _Batch(), torch.zeros(8)
    two = [s, s.view(-1, 1)]
    # an unknown partition, everywhere the keyword exists
    for bad in ("scc", "Strong", None, 3, ("strong",)):
        with pytest.raises(ValueError, match="partition"):
            sweep_thresholds(b, s, [0.5], partition=bad)
        with pytest.raises(ValueError, match="partition"):
            sweep_joint(b, two, [[0.5, 0.5]], ["lt", "lt"], partition=bad)
        with pytest.raises(ValueError, match="partition"):
            sweep_grid(b, two, [[0.5], [0.5]], ["lt", "lt"], partition=bad)
        with pytest.raises(ValueError, match="partition"):
            geometry_baseline(b, 1.5, [20.0, 30.0], partition=bad)
    # the camera-exclusive partition is not swept jointly
    for call in (lambda: sweep_joint(b, two, [[0.5, 0.5]], ["lt", "lt"], partition="exclusive"),
                 lambda: sweep_grid(b, two, [[0.5], [0.5]], ["lt", "lt"], partition="exclusive"),
                 lambda: geometry_baseline(b, 1.5, [20.0, 30.0], partition="exclusive")):
        with pytest.raises(ValueError, match="exclusive"):
            call()
    # a 1025-node frame: the limit is named; 1024 passes the host checks
    wide, fits = _Batch(sizes=(1025, 2)), _Batch(sizes=(1024, 2))
    with pytest.raises(ValueError, match="at most 1024"):
        sweep_thresholds(wide, s, [0.5], partition="strong")
    with pytest.raises(ValueError, match="at most 1024"):
        sweep_joint(wide, two, [[0.5, 0.5]], ["lt", "lt"], partition="strong")
    with pytest.raises(ValueError, match="at most 1024"):
        geometry_baseline(wide, 1.5, [20.0, 30.0], partition="strong")
    with pytest.raises(RuntimeError, match="MI355X only"):
        sweep_thresholds(fits, s, [0.5], partition="strong")
    with pytest.raises(RuntimeError, match="MI355X only"):                  # ... and the components keep their own limit
        sweep_joint(wide, two, [[0.5, 0.5]], ["lt", "lt"])
    # lengths that disagree
    short = _Batch()
    short.edge_labels = torch.zeros(5)
    for call in (lambda: sweep_thresholds(b, torch.zeros(7), [0.5], partition="strong"),
                 lambda: sweep_thresholds(short, s, [0.5], partition="strong"),
                 lambda: sweep_joint(short, two, [[0.5, 0.5]], ["lt", "lt"], partition="strong"),
                 lambda: sweep_joint(b, [s, torch.zeros(7)], [[0.5, 0.5]], ["lt", "lt"], partition="strong")):
        with pytest.raises(ValueError, match="match"):
            call()
    # sweep_thresholds' own argument checks hold under the new partition
    with pytest.raises(ValueError, match="keep"):
        sweep_thresholds(b, s, [0.5], keep="lt", partition="strong")
    for bad in ([], [float("nan")], [[0.5]], np.zeros(1025)):
        with pytest.raises(ValueError, match="thresholds"):
            sweep_thresholds(b, s, bad, partition="strong")
    with pytest.raises(ValueError, match="points"):
        sweep_joint(b, two, [[0.5]], ["lt", "lt"], partition="strong")
    with pytest.raises(ValueError, match="frame_div"):
        sweep_joint(b, two, [[0.5, 0.5]], ["lt", "lt"], frame_div=[[1.0, 0.0], [1.0, 1.0]], partition="strong")
    # what is left is a well-formed call on host tensors: the module's usual refusal (any finite threshold, both keeps, cam ignored)
    for keep, ths in (("ge", [0.5]), ("le", [-3.0, 0.0, 1.0, 7.5]), ("ge", np.linspace(0, 1, 1024))):
        with pytest.raises(RuntimeError, match="MI355X only"):
            sweep_thresholds(b, s, ths, keep=keep, partition="strong", cam="ignored")
    with pytest.raises(RuntimeError, match="MI355X only"):
        sweep_joint(b, two, [[0.5, 0.5]], ["lt", "ge"], frame_div=np.ones((2, 2)), partition="strong", return_labels=True)
    with pytest.raises(RuntimeError, match="MI355X only"):
        sweep_grid(b, two, [np.zeros(128), np.zeros(128)], ["lt", "lt"], partition="strong")
    for kw in ({}, {"reid_th": 0.4}):
        with pytest.raises(RuntimeError, match="MI355X only"):
            geometry_baseline(b, 1.5, [20.0, 30.0], partition="strong", **kw)


# ---- the C entry's refusals ------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000
    n, e, g = 10, 24, 2
    ws = lib.gnncca_eval_sweep_strong_workspace_bytes(n, e, g)
    assert ws == lib.gnncca_eval_workspace_bytes(n, e, g) and ws % 256 == 0                # the lgamma tables only
    assert ws < lib.gnncca_eval_sweep_joint_workspace_bytes(n, e, g)                       # no plan, no reverse edges
    assert lib.gnncca_eval_sweep_strong_workspace_bytes(1000, 10 ** 6, 10) == lib.gnncca_eval_sweep_strong_workspace_bytes(1000, 0, 10)
    for bad in ((-1, e, g), (n, -1, g), (n, e, -1)):
        assert lib.gnncca_eval_sweep_strong_workspace_bytes(*bad) == 0

    def call(k=2, t=5, max_n=6, ei=fake, el=fake, sc=(fake, fake, fake, fake), strides=(1, 4, 1, 1), cmps=(3, 3, 0, 2), nptr=fake, eptr=fake,
             pts=fake, div=None, rows=fake, work=fake, nbytes=ws, nn=n, ee=e, gg=g):
        ptrs = (C.c_void_p * 4)(*sc) if sc is not None else None
        st = (C.c_int64 * 4)(*strides) if strides is not None else None
        cm = (C.c_int32 * 4)(*cmps) if cmps is not None else None
        return lib.gnncca_eval_sweep_strong(ei, el, ptrs, st, cm, k, nn, ee, nptr, eptr, gg, max_n, pts, t, div, rows, None, work, nbytes, None)

    for k in (0, -1, 5, 1 << 20):
        assert call(k=k) == nat.ERR_INVALID_ARG, k
    for t in (-1, 16385, 1 << 30):
        assert call(t=t) == nat.ERR_INVALID_ARG, t
    for cmps in ((4, 0, 0, 0), (0, -1, 0, 0), (0, 99, 0, 0)):
        assert call(cmps=cmps) == nat.ERR_INVALID_ARG, cmps
    assert call(k=1, cmps=(3, 99, 0, 0), nbytes=ws - 1) == nat.ERR_WORKSPACE           # only the first K codes are read
    for strides in ((0, 1, 1, 1), (1, -4, 1, 1), (1, 0, 1, 1)):
        assert call(strides=strides) == nat.ERR_INVALID_ARG, strides
    assert call(sc=(fake, None, fake, fake)) == nat.ERR_INVALID_ARG and call(sc=(None, fake, fake, fake)) == nat.ERR_INVALID_ARG
    assert call(max_n=-1) == nat.ERR_INVALID_ARG and call(max_n=n + 1) == nat.ERR_INVALID_ARG
    assert call(max_n=1025, nn=2000) == nat.ERR_INVALID_ARG                            # GNNCCA_STRONG_MAX_FRAME_NODES, not the scorer's 4096
    assert call(max_n=1024, nn=2000, nbytes=0) == nat.ERR_WORKSPACE                    # the limit itself passes the argument checks
    for name in ("ei", "el", "sc", "strides", "cmps", "nptr", "eptr", "pts", "rows", "work"):
        assert call(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert call(nn=-1) == nat.ERR_INVALID_ARG and call(ee=-1) == nat.ERR_INVALID_ARG and call(gg=-1) == nat.ERR_INVALID_ARG
    assert call(nbytes=ws - 1) == nat.ERR_WORKSPACE and call(nbytes=0) == nat.ERR_WORKSPACE
    assert call(k=4, t=16384, div=fake, nbytes=ws - 1) == nat.ERR_WORKSPACE            # the limits themselves pass the argument checks
    # nothing to score: nothing launched, whichever count is zero
    assert call(gg=0, nptr=None, eptr=None, rows=None, work=None, nbytes=0) == nat.OK
    assert call(t=0, pts=None, rows=None, work=None, nbytes=0) == nat.OK
    assert call(gg=0, k=5) == nat.ERR_INVALID_ARG and call(t=0, cmps=(7, 0, 0, 0)) == nat.ERR_INVALID_ARG   # ... the arguments are still judged
