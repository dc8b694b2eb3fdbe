"""FrameLinker(matching='optimal') on its restatement (tests/tracking_assign_oracle.py, which the GPU tests compare the kernel with): the
augmenting-path loops against a brute-force optimum and against scipy, matching='mutual' through the new walk against
tracking_gap_oracle.link_gap, a hand-written 2 x 2 case where the two rules differ, that cutting a sequence into batches changes nothing;
and what the Python front end and the ctypes binding declare and refuse, which needs no GPU."""
import math

import numpy as np
import pytest

import tracking_assign_oracle as ta
import tracking_gap_oracle as tg
from test_tracking_gap_oracle import _line


def test_the_loops_find_the_brute_force_optimum():
    rng = np.random.default_rng(5)
    worst, busiest = 0.0, 0
    for case in range(400):
        n, m = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        w = rng.uniform(-1.0, 0.3, size=(n, m))   # (some pairs dearer than staying unlinked)
        ok = rng.random((n, m)) < 0.6
        col, steps = ta.assign(w, ok)
        taken = [j for j in col if j >= 0]
        assert len(set(taken)) == len(taken) and all(ok[i, j] for i, j in enumerate(col) if j >= 0)
        assert all(w[i, j] <= 0 for i, j in enumerate(col) if j >= 0)   # a pair dearer than the miss cost is never taken
        worst = max(worst, abs(ta.total(w, col) - ta.brute_force(w, ok)))
        busiest = max(busiest, steps)
    print("largest difference to the brute-force total:", worst, "most tree steps of a row:", busiest)
    assert worst < 1e-12 and busiest > 2
    assert ta.assign(np.zeros((0, 3)), np.zeros((0, 3), bool))[0].tolist() == []
    assert ta.assign(np.zeros((2, 0)), np.zeros((2, 0), bool))[0].tolist() == [-1, -1]
    assert ta.assign(np.full((2, 2), -1.0), np.zeros((2, 2), bool))[0].tolist() == [-1, -1]


def test_the_loops_equal_scipy_on_integer_costs():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(6)
    for case in range(50):
        n, m = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        w = rng.integers(-20, 5, size=(n, m)).astype(np.float64)   # integers: every total is exact
        ok = rng.random((n, m)) < 0.6
        col, _ = ta.assign(w, ok)
        # the same problem as a square-free padded matrix: column m + i is row i's unlinked column, a non-edge is dearer than any set
        big = 1e6
        padded = np.full((n, m + n), big)
        padded[:, :m] = np.where(ok, w, big)
        padded[np.arange(n), m + np.arange(n)] = 0.0
        rr, cc = linear_sum_assignment(padded)
        assert ta.total(w, col) == float(padded[rr, cc].sum()), case


CASES = [(12, 25, 21, 1.0, None, 2), (9, 70, 3, 0.0, None, 1), (9, 70, 4, 0.5, 0.05, 0), (12, 40, 8, 0.0, 1.0, 3)]


@pytest.mark.parametrize("g,persons,seed,lam,max_cos,m", CASES)
def test_mutual_through_the_new_walk_is_the_gap_oracle(g, persons, seed, lam, max_cos, m):
    summ = tg.hide_sequence(np.random.default_rng(seed), g, persons, 8, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=8.0, empty=(7,))
    want, wstate = tg.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, m)
    got, state = ta.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, m, matching="mutual")
    for k in ("cluster_track", "node_track", "matched_prev", "matched_gap"):
        assert np.array_equal(got[k], want[k]), k
    assert got["next_id"] == want["next_id"] == state["next_id"] == wstate["next_id"]
    for a, b in zip(state["frames"], wstate["frames"]):
        assert all(np.array_equal(a[k], b[k]) for k in ("pos", "emb", "track", "succ"))


def test_two_by_two_by_hand():
    #           b0    b1       a0    a1
    s = _line([[0.0, 0.7], [0.3, -0.6]])
    mutual, _ = ta.link_gap(s, s["node_ptr"], max_step=0.8, lam=0.0, matching="mutual")
    # a0 is 0.3 from b0 and 0.4 from b1, a1 is 0.6 from b0 and 1.3 (outside the gate) from b1.  b0's best is a0 and a0's best is b0: they
    # link; a1's only admissible partner is taken, b1's best a0 prefers b0: a1 starts a new track and b1's track ends.
    assert mutual["matched_prev"].tolist() == [-1, -1, 0, -1] and mutual["cluster_track"].tolist() == [0, 1, 0, 2] and mutual["next_id"] == 3
    # miss cost 1 (lam = 0): linking nobody is worth 0, a0-b0 alone 0.375 - 1, a0-b1 with a1-b0 (0.5 - 1) + (0.75 - 1) = -0.75: the least
    opt, state = ta.link_gap(s, s["node_ptr"], max_step=0.8, lam=0.0, matching="optimal")
    assert opt["matched_prev"].tolist() == [-1, -1, 1, 0] and opt["cluster_track"].tolist() == [0, 1, 1, 0] and opt["next_id"] == 2
    assert opt["matched_gap"].tolist() == [-1, -1, 0, 0] and state["frames"][-1]["track"].tolist() == [1, 0]
    assert ta.default_miss_cost(0.0, None) == 1.0 and ta.default_miss_cost(0.5, None) == 2.0 and ta.default_miss_cost(2.0, 0.25) == 1.5
    # a miss cost of 0.7 makes a1-b0 (0.75) dearer than staying unlinked: then a0-b0 alone, which is what mutual best found
    cheap, _ = ta.link_gap(s, s["node_ptr"], max_step=0.8, lam=0.0, matching="optimal", miss_cost=0.7)
    assert cheap["matched_prev"].tolist() == [-1, -1, 0, -1]
    # a NaN position is outside every gate; a NaN embedding makes the cost NaN, which is not admissible in this mode
    s2 = _line([[0.0, 0.7], [0.3, float("nan")]])
    assert ta.link_gap(s2, s2["node_ptr"], 0.8, 0.0, matching="optimal")[0]["matched_prev"].tolist() == [-1, -1, 0, -1]
    s3 = dict(_line([[0.0, 0.7], [0.3, -0.6]]), emb=np.array([[1, 0], [0, 1], [1, 0], [math.nan, 0]], np.float32))
    assert ta.link_gap(s3, s3["node_ptr"], 0.8, 1.0, matching="optimal")[0]["matched_prev"].tolist() == [-1, -1, 0, -1]


@pytest.mark.parametrize("m", [0, 1, 2])
@pytest.mark.parametrize("cuts", [((0, 5), (5, 6), (6, 12)), ((0, 5), (5, 6), (6, 6), (6, 7), (7, 12)), ((0, 1), (1, 1), (1, 12))])
def test_cutting_a_sequence_into_batches_changes_nothing(m, cuts):
    summ = tg.hide_sequence(np.random.default_rng(40 + m), 12, 30, 8, noise=0.3, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=5.0, empty=(7,))
    whole, wstate = ta.link_gap(summ, summ["node_ptr"], 0.8, 0.0, None, m, matching="optimal")
    mutual, _ = ta.link_gap(summ, summ["node_ptr"], 0.8, 0.0, None, m, matching="mutual")
    assert not np.array_equal(whole["cluster_track"], mutual["cluster_track"])   # crowded enough for the two rules to differ
    assert all((whole["matched_gap"] == k).any() for k in range(m + 1))
    state, parts = None, []
    for lo, hi in cuts:
        part = tg.frames_of(summ, lo, hi)
        out, state = ta.link_gap(part, part["node_ptr"], 0.8, 0.0, None, m, state, matching="optimal")
        parts.append(out)
    for k in ("cluster_track", "node_track", "matched_prev", "matched_gap"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    assert parts[-1]["next_id"] == whole["next_id"] == state["next_id"]
    for a, b in zip(state["frames"], wstate["frames"]):
        assert a["count"] == b["count"] and all(np.array_equal(a[k], b[k]) for k in ("pos", "emb", "track", "succ"))


def test_the_linker_validates_matching_and_miss_cost_before_the_gpu():
    from gnn_cca_amd import tracking
    from gnn_cca_amd.tracking import FrameLinker
    assert tracking.MAX_OPTIMAL_FRAME_NODES == ta.MAX_OPTIMAL_FRAME_NODES == 128 and "MAX_OPTIMAL_FRAME_NODES" in tracking.__all__
    for bad in ("best", "Optimal", None, 1, True, b"optimal"):
        with pytest.raises(ValueError):
            FrameLinker(1.0, matching=bad)
        with pytest.raises(ValueError):
            ta.link_gap(_line([[0.0]]), [0, 1], 1.0, 0.0, matching=bad)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError):
            FrameLinker(1.0, matching="optimal", miss_cost=bad)
    with pytest.raises(ValueError):
        FrameLinker(1.0, miss_cost=1.0)   # the mutual-best rule has no price for staying unlinked
    with pytest.raises(ValueError):
        FrameLinker(1.0, matching="mutual", miss_cost=3.0)
    link = FrameLinker(1.0)
    assert link.matching == "mutual" and link.max_gap == 0
    assert FrameLinker(0.8, 0.0, None, 0, "optimal").miss_cost == ta.default_miss_cost(0.0, None) == 1.0
    assert FrameLinker(0.8, lam=0.5, matching="optimal").miss_cost == 2.0
    assert FrameLinker(0.8, lam=2.0, max_cos=0.25, matching="optimal").miss_cost == ta.default_miss_cost(2.0, 0.25) == 1.5
    assert FrameLinker(0.8, matching="optimal", miss_cost=np.float64(0.5)).miss_cost == 0.5


def test_the_binding_declares_the_ex_entry():
    import os
    import re
    from conftest import ROOT
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    assert "gnncca_link_frames_gap_ex" in nat.exported_symbols()
    decl = re.search(r"GNNCCA_API\s+int\s+gnncca_link_frames_gap_ex\s*\(([^;]*)\)\s*;", header).group(1)
    args = nat._SIGNATURES["gnncca_link_frames_gap_ex"][1]
    assert len(decl.split(",")) == len(args) == len(nat._SIGNATURES["gnncca_link_frames_gap"][1]) + 2   # matching, miss_cost
    assert re.search(r"int32_t\s+max_gap,\s*int32_t\s+matching,\s*double\s+miss_cost,", decl)
    assert int(re.search(r"#define GNNCCA_TRACK_MAX_OPTIMAL_FRAME_NODES (\d+)", header).group(1)) == nat.TRACK_MAX_OPTIMAL_FRAME_NODES == 128
    assert nat.MATCHING == {"mutual": 0, "optimal": 1}


def test_the_ex_entry_checks_its_arguments_before_any_launch():
    """No device needed: the argument checks come first and the (fake) device pointers are never followed."""
    import ctypes as C
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000

    def call(n=5, g=1, max_n=5, gap=2, matching=1, miss=1.0, rows_in=(10, 20), rows_out=(10, 20, 5), ws_bytes=1 << 20):
        c_in, c_out = (C.c_int32 * max(len(rows_in), 1))(*rows_in), (C.c_int32 * max(len(rows_out), 1))(*rows_out)
        return lib.gnncca_link_frames_gap_ex(fake, fake, fake, fake, None, 0, n, g, max_n, 1.0, 0.0, 0, 0.0, gap, matching, miss, fake, c_in,
                                             len(rows_in), fake, c_out, len(rows_out), fake, fake, fake, fake, fake, ws_bytes, None)

    assert call(g=0) == nat.OK and call(g=0, matching=0) == nat.OK            # no frames: nothing is launched, nothing written
    for bad in (dict(matching=2), dict(matching=-1), dict(miss=0.0), dict(miss=-1.0), dict(miss=float("inf")), dict(miss=float("nan")),
                dict(n=129, max_n=129, rows_out=(10, 20, 129)), dict(rows_in=(10, 129)), dict(gap=-1), dict(rows_out=(10, 20))):
        assert call(**bad) == nat.ERR_INVALID_ARG, bad
    # the limit is the optimal form's alone: mutual best takes the same frames through the same entry (and then misses its workspace)
    assert call(matching=0, n=129, max_n=129, rows_in=(10, 129), rows_out=(10, 129, 129), ws_bytes=16) == nat.ERR_WORKSPACE
    assert call(ws_bytes=16) == nat.ERR_WORKSPACE
