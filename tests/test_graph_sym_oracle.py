"""Symmetric capped graphs (build_graph_batch(top_k=k, symmetric='union' | 'mutual')) and scoring against the dense truth
(evaluate_frames(against='dense')): the numpy restatements (tests/helpers/graph_sym_oracle.py) on the golden graph cases, and the argument
refusals of the public functions, which are raised before the GPU is touched.  CPU only.  Home of what test_gpu_graph_sym.py and
test_gpu_eval_dense.py share with it: the case list, the cached oracle cases, the stated tie sets and the check that no case holds a near
tie at the tested k."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_graph_topk_oracle import GOLDEN_CASES, KS, RANKS, SYNTHETIC, load

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import eval_oracle as eo  # noqa: E402
import graph_sym_oracle as gso  # noqa: E402
import graph_topk_oracle as gto  # noqa: E402

CASES = GOLDEN_CASES + SYNTHETIC + ["ties"]
MODES = gso.MODES
EVAL_CASES = ["batch3", "frame70"]
EVAL_KS = [1, 3]

_oracle = {}


def case(name):
    """The oracle's dense build and keys of a case, computed once and left unchanged."""
    if name not in _oracle:
        _oracle[name] = gso.Case(load(name))
    return _oracle[name]


# ties_case with k = 1, by destination list of every source (0 and 7 on camera 0 at the origin with the same reid row; 1 .. 4 on camera 1
# at distance exactly 1 with identical reid rows; 5, 6 on camera 2, farther away in both keys).  D: 0 -> 1 and 7 -> 1 (ties to the smaller
# id), 1 .. 4 -> 0 (0 and 7 tie), and 5, 6 -> 2 by 'ground' ((0, 1) is the nearest to both), -> 0 by 'reid' (0 and 7 tie there too).
TIES_K1 = {
    "ground": {"mutual": {0: [1], 1: [0]},
               "union": {0: [1, 2, 3, 4], 1: [0, 7], 2: [0, 5, 6], 3: [0], 4: [0], 5: [2], 6: [2], 7: [1]}},
    "reid": {"mutual": {0: [1], 1: [0]},
             "union": {0: [1, 2, 3, 4, 5, 6], 1: [0, 7], 2: [0], 3: [0], 4: [0], 5: [0], 6: [0], 7: [1]}},
}


def by_source(ei):
    out = {}
    for s, d in ei.T.tolist():
        out.setdefault(s, []).append(d)
    return out


@pytest.mark.parametrize("name", CASES)
def test_oracle_properties(name):
    c = case(name)
    deg = gto.degrees(c.a)
    rev = gso.reverse_index(c.ei)
    assert np.array_equal(c.ei[:, rev], c.ei[::-1]) and np.array_equal(rev[rev], np.arange(rev.size))
    for rank_by in RANKS:
        for k in KS:
            d = c.keep(k, rank_by, None)
            u, m = c.keep(k, rank_by, "union"), c.keep(k, rank_by, "mutual")
            assert np.array_equal(u, u[rev]) and np.array_equal(m, m[rev])          # closed under reversal
            assert not (m & ~d).any() and not (d & ~u).any()                        # mutual <= D <= union
            assert np.array_equal(u | m, u) and np.array_equal(u & ~m, d ^ d[rev])  # they differ exactly by the one-way edges
            for mode, keep in (("union", u), ("mutual", m)):
                ei_k, attr_k, lab_k, keep2 = c.build(k, rank_by, mode)
                assert np.array_equal(keep, keep2) and np.array_equal(ei_k, c.ei[:, keep]) and np.array_equal(attr_k, c.attr[keep])
                assert int(c.edge_ptr(keep)[-1]) == int(keep.sum())
        for k in (int(max(deg.max(), 1)), 10 ** 6):                                 # k >= max deg: the dense list
            for mode in MODES:
                assert c.keep(k, rank_by, mode).all()


def test_one_way_edges_exist_on_the_cases():
    """The closure is not vacuous: at k = 3 a good share of the directed list has no reverse (64 % reciprocated on frame70 by ground
    distance: 138 of the 162 same-identity dense edges kept by the cap, 120 in both directions)."""
    c = case("frame70")
    d, m = c.keep(3, "ground", None), c.keep(3, "ground", "mutual")
    assert round(100 * m.sum() / d.sum()) == 64
    assert (int((c.lab == 1).sum()), int((d & (c.lab == 1)).sum()), int((m & (c.lab == 1)).sum())) == (162, 138, 120)


def test_a_single_camera_frame_has_no_edge():
    a = gto.degree_steps_case()
    only = {k: (v[6:8] if np.ndim(v) and len(v) == len(a["id_cam"]) else v) for k, v in a.items()}
    only["graph_sizes"], only["max_dist"] = np.array([2], np.int64), a["max_dist"][1:2]
    c = gso.Case(only)
    assert c.ei.shape == (2, 0)
    for mode in MODES:
        assert c.keep(1, "ground", mode).size == 0 and c.edge_ptr(c.keep(1, "ground", mode)).tolist() == [0, 0]
    # and inside a batch: frame 1 of degree_steps owns no edge in either mode
    c = case("degree_steps")
    for mode in MODES:
        ptr = c.edge_ptr(c.keep(2, "reid", mode))
        assert ptr[1] == ptr[2] and ptr[1] > 0 and ptr[3] > ptr[2]


def test_stated_tie_sets():
    c = case("ties")
    for rank_by in RANKS:
        assert by_source(c.build(1, rank_by, None)[0]) == {0: [1], 1: [0], 2: [0], 3: [0], 4: [0], 7: [1],
                                                           5: [2] if rank_by == "ground" else [0], 6: [2] if rank_by == "ground" else [0]}
        for mode in MODES:
            assert by_source(c.build(1, rank_by, mode)[0]) == TIES_K1[rank_by][mode], (rank_by, mode)


@pytest.mark.parametrize("name", CASES)
def test_no_case_holds_a_near_tie(name):
    """test_gpu_graph_sym.py compares selections exactly: it may skip a source whose k-th and (k+1)-th keys are within 1e-6 relative, and
    asserts that it skipped none.  `ties` holds exact ties only (equal bits on both sides: no evaluation order can flip them), which
    near_ties reports too: there the check is that every reported pair of keys is EQUAL."""
    c = case(name)
    for rank_by in RANKS:
        for k in KS:
            near = gto.near_ties(c.ei, c.key[rank_by], k)
            if name != "ties":
                assert near == [], (name, rank_by, k)
                continue
            for s0, s1 in gto.segments(c.ei):
                if int(c.ei[0, s0]) in near:
                    ks = np.sort(c.key[rank_by][s0:s1])
                    assert ks[k - 1] == ks[k], (rank_by, k, int(c.ei[0, s0]))


@pytest.mark.parametrize("mode", [None, "union"])
@pytest.mark.parametrize("k", EVAL_KS)
@pytest.mark.parametrize("name", EVAL_CASES)
def test_scoring_against_the_dense_truth(name, k, mode):
    """Scattering the capped predictions into the dense list and scoring that (the oracle of against='dense') feeds the formulas exactly
    what the definition says: TP / FP of the kept edges, FN / TN raised by the dropped pairs of each class counted from the person ids and
    cameras, ID_GT from the identities seen on two cameras."""
    c = case(name)
    keep = c.keep(k, "ground", mode)
    pred, labels = gso.random_outcome(c, keep, seed=7)
    rows, gt = gso.score_against_dense(c, keep, pred, labels)
    counts, gt_def = gso.dense_truth_by_definition(c, keep, pred)
    assert np.array_equal(rows[:, [3, 4, 5, 6]], counts.astype(np.float64)) and np.array_equal(gt, gt_def)
    kept_rows, kept_gt = gso.score_kept(c, keep, pred, labels)
    assert np.array_equal(rows[:, [3, 4]], kept_rows[:, [3, 4]])                       # TP and FP as today
    assert np.all(rows[:, 5] >= kept_rows[:, 5]) and np.all(rows[:, 6] >= kept_rows[:, 6])
    assert not keep.all() and rows[:, 5:7].sum() - kept_rows[:, 5:7].sum() == keep.size - keep.sum()   # every dropped edge is a negative
    assert rows[:, 14].sum() <= kept_rows[:, 14].sum()                                 # a true identity no longer falls apart
    if (name, k) == ("frame70", 3) and mode is None:
        assert rows[:, 5].sum() - kept_rows[:, 5].sum() == 162 - 138                   # the true pairs the directed cap dropped
    # a dense "capped" batch scores as itself
    everything = np.ones(keep.size, bool)
    pred_all, _ = gso.random_outcome(c, everything, seed=8)
    a, b = gso.score_against_dense(c, everything, pred_all, labels), gso.score_kept(c, everything, pred_all, labels)
    assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
    assert len(eo.COLUMNS) == rows.shape[1]


class _NoGpu:
    """An embedding stand-in that fails the test if the GPU path is entered: the refusals come first."""
    shape = (4, 8)

    @property
    def is_cuda(self):
        raise AssertionError("the argument check must come before the device check")


def test_argument_refusals_come_before_the_gpu():
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    a = load("one_frame")
    args = (a["xw"], a["yw"], a["id"], a["id_cam"], a["graph_sizes"], a["max_dist"], _NoGpu(), _NoGpu())
    for kw in (dict(symmetric="union"), dict(symmetric="mutual"), dict(top_k=2, symmetric="both"), dict(top_k=2, symmetric=True),
               dict(top_k=2, symmetric=1), dict(top_k=2, symmetric=""), dict(top_k=0, symmetric="union"),
               dict(top_k=2, rank_by="cosine", symmetric="union")):
        with pytest.raises(ValueError):
            build_graph_batch(*args, **kw)
        with pytest.raises(ValueError):
            FramePipeline(None, **kw)
    with pytest.raises(AssertionError):
        build_graph_batch(*args, top_k=2, symmetric="union")      # (a legal request does reach the device check)
    pipe = FramePipeline(None, top_k=2, symmetric="mutual")
    assert (pipe.top_k, pipe.symmetric) == (2, "mutual") and FramePipeline(None, top_k=2).symmetric is None
    for bad in ("full", None, 1, "Dense"):
        with pytest.raises(ValueError):
            evaluate_frames(None, None, None, against=bad)
    with pytest.raises(ValueError):      # against='dense' needs the person ids and cameras of the batch
        evaluate_frames(object(), None, None, against="dense")
