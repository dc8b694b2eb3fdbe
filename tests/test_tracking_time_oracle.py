"""Time stamps in gnn_cca_amd.tracking (FrameLinker(...)(x, times=...)) on their numpy restatement (tests/tracking_time_oracle.py, which
the GPU tests compare the kernels with): with times 0, 1, 2, ... it is each untimed oracle in every field, also across batches with the
state carried; a dropped frame is a gap, by hand; and what the Python front end and the ctypes binding declare and refuse, which needs no
GPU."""
import inspect

import numpy as np
import pytest

import tracking_assign_oracle as ta
import tracking_gap_oracle as tg
import tracking_motion_oracle as tm
import tracking_time_oracle as tt

FIELDS = ("cluster_track", "node_track", "matched_prev", "matched_gap")
CUTS = ((0, 5), (5, 6), (3, 3), (6, 12))   # (3, 3): a call without frames passes no time


def _points(frames):
    """frames: per frame a list of (x, y) -> the summaries of one-node clusters, without embeddings."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([p for f in frames for p in f], np.float64).reshape(n, 2)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, pos=pos, emb=np.zeros((n, 0), np.float32), node_ptr=node_ptr)


def _in_batches(summ, link):
    """link(part, lo, hi, state) -> (out, state) over CUTS -> (the outputs concatenated, the last next_id, the last state)."""
    state, parts = None, []
    for lo, hi in CUTS:
        out, state = link(tg.frames_of(summ, lo, hi), lo, hi, state)
        parts.append(out)
    whole = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "next_id"}
    return whole, parts[-1]["next_id"], state


def _same_states(a, b, keys):
    assert len(a["frames"]) == len(b["frames"]) and a["next_id"] == b["next_id"]
    for fa, fb in zip(a["frames"], b["frames"]):
        assert fa["count"] == fb["count"] and all(np.array_equal(fa[k], fb[k]) for k in keys)


# ---- the main consequence: times 0, 1, 2, ... give the untimed rule, in every field, in one call and across batches ---------------------
@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("lam,max_cos,empty,seed", [(1.0, None, (), 1), (0.5, 0.05, (5,), 2), (0.0, None, (4, 5), 3)])
def test_with_times_0_1_2_the_gap_rule(m, lam, max_cos, empty, seed):
    summ = tg.hide_sequence(np.random.default_rng(seed), 12, 40, 16, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=9.0, empty=empty)
    want, wstate = tg.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    got, state = tt.link_timed(summ, summ["node_ptr"], np.arange(12), 1.0, lam, max_cos, m)
    parts, next_id, pstate = _in_batches(summ, lambda p, lo, hi, st: tt.link_timed(p, p["node_ptr"], np.arange(lo, hi), 1.0, lam, max_cos, m, st))
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]) and np.array_equal(parts[k], want[k]), k
    assert got["next_id"] == want["next_id"] == next_id and not got["velocity"].any()
    _same_states(state, wstate, ("pos", "emb", "track", "succ"))
    _same_states(pstate, wstate, ("pos", "emb", "track", "succ"))
    assert [float(f["time"]) for f in state["frames"]] == list(range(12 - len(state["frames"]), 12))


@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("lam,seed,miss_cost", [(0.0, 1, None), (1.0, 4, None), (0.0, 7, 0.6)])
def test_with_times_0_1_2_the_optimal_rule(m, lam, seed, miss_cost):
    summ = tg.hide_sequence(np.random.default_rng(seed), 12, 40, 8, arena=6.0, max_hide=m + 1, noise=0.3, max_alive=70)
    want, wstate = ta.link_gap(summ, summ["node_ptr"], 0.8, lam, None, m, matching="optimal", miss_cost=miss_cost)
    base, _ = ta.link_gap(summ, summ["node_ptr"], 0.8, lam, None, m, matching="mutual")
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    assert lam != 0.0 or not np.array_equal(base["cluster_track"], want["cluster_track"])   # the assignment differs from mutual best here
    kw = dict(matching="optimal", miss_cost=miss_cost)
    got, state = tt.link_timed(summ, summ["node_ptr"], np.arange(12), 0.8, lam, None, m, **kw)
    parts, next_id, pstate = _in_batches(summ, lambda p, lo, hi, st: tt.link_timed(p, p["node_ptr"], np.arange(lo, hi), 0.8, lam, None, m, st, **kw))
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]) and np.array_equal(parts[k], want[k]), k
    assert got["next_id"] == want["next_id"] == next_id
    _same_states(state, wstate, ("pos", "emb", "track", "succ"))
    _same_states(pstate, wstate, ("pos", "emb", "track", "succ"))


@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("lam,seed", [(1.0, 30), (0.0, 31)])
def test_with_times_0_1_2_the_motion_rule(m, lam, seed):
    summ = tm.cross_sequence(np.random.default_rng(seed + m), 12, 25, 8, p_hide=0.12 if m else 0.0, max_hide=m + 1, arena=6.0)
    want, wstate = tm.link_motion(summ, summ["node_ptr"], 0.4, lam, None, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1)) and want["velocity"].any()
    got, state = tt.link_timed(summ, summ["node_ptr"], np.arange(12), 0.4, lam, None, m, motion=True)
    parts, next_id, pstate = _in_batches(summ, lambda p, lo, hi, st: tt.link_timed(p, p["node_ptr"], np.arange(lo, hi), 0.4, lam, None, m, st,
                                                                                    motion=True))
    for k in FIELDS + ("velocity",):
        assert np.array_equal(got[k], want[k]) and np.array_equal(parts[k], want[k]), k
    assert got["next_id"] == want["next_id"] == next_id
    _same_states(state, wstate, ("pos", "vel", "emb", "track", "succ"))
    _same_states(pstate, wstate, ("pos", "vel", "emb", "track", "succ"))


# ---- a dropped frame is a gap ----------------------------------------------------------------------------------------------------------
def walker(times, speed=0.5):
    return _points([[(speed * t, 0.0)] for t in times])


def _hole_walk(link):
    """One person walks 0.5 per period along x; the frame at time 2 is absent (times 0, 1, 3, 4); max_gap = 1, motion, max_step = 0.2.
    A track's FIRST link is made without a velocity, and 0.5 is outside 0.2: so the frames at times 0 and 1 are one call under
    max_step = 1.0, which gives the track its velocity (0.5, 0), and the frames at times 3 and 4 a second call under max_step = 0.2 on
    the carried state.  link(part, times, max_step, state) -> (out, state).  -> the two outputs."""
    a, state = link(walker([0, 1]), [0, 1], 1.0, None)
    b, _ = link(_points([[(1.5, 0.0)], [(2.0, 0.0)]]), [3, 4], 0.2, state)
    return a, b


def test_a_dropped_frame_by_hand():
    # untimed: after the hole the prediction 0.5 + 1 * 0.5 = 1.0 is 0.5 from 1.5, outside 0.2 (and 0.4 at level 1): a second id, then a third
    a, b = _hole_walk(lambda p, t, step, st: tm.link_motion(p, p["node_ptr"], step, 0.0, None, 1, st))
    assert a["cluster_track"].tolist() == [0, 0] and a["velocity"].tolist() == [[0.0, 0.0], [0.5, 0.0]]
    assert b["cluster_track"].tolist() == [1, 2] and not b["velocity"].any()
    # timed: dt = 2 at level 0, pred = 0.5 + 2 * 0.5 = 1.5 exactly, vel = 1.0 / 2; then dt = 1, pred = 1.5 + 0.5 = 2.0
    a, b = _hole_walk(lambda p, t, step, st: tt.link_timed(p, p["node_ptr"], t, step, 0.0, None, 1, st, motion=True))
    assert a["cluster_track"].tolist() == [0, 0] and b["cluster_track"].tolist() == [0, 0] and b["next_id"] == 1
    assert b["matched_gap"].tolist() == [0, 0] and a["velocity"].tolist()[1] == b["velocity"].tolist()[0] == b["velocity"].tolist()[1] == [0.5, 0.0]
    # the tables of the second call: (level 1, frame 0) has dt = 3 > max_dt = 2 and is skipped, and everybody is linked before (1, 1)
    _, state = tt.link_timed(walker([0, 1]), [0, 1, 2], [0, 1], 1.0, 0.0, None, 1, motion=True)
    tables = tt.level_tables(_points([[(1.5, 0.0)], [(2.0, 0.0)]]), [0, 1, 2], [3, 4], 0.2, 0.0, None, 1, state, motion=True)
    assert [(k, t, float(dt)) for k, t, *_, dt in tables] == [(0, 0, 2.0), (0, 1, 1.0)]
    assert [float(f["time"]) for f in state["frames"]] == [0.0, 1.0]
    # with max_gap = 0 the default max_dt is 1: the hole (dt = 2) ends the track
    a, b = _hole_walk(lambda p, t, step, st: tt.link_timed(p, p["node_ptr"], t, step, 0.0, None, 0, st, motion=True))
    assert a["cluster_track"].tolist() == [0, 0] and b["cluster_track"].tolist() == [1, 2] and not b["velocity"].any()
    # times 0, 1, 5 and a person walking 0.1 per period: the link over dt = 4 exists under the default max_dt = max_gap + 1 = 4, not under 3.5
    slow = walker([0, 1, 5], speed=0.1)
    assert tt.link_timed(slow, slow["node_ptr"], [0, 1, 5], 0.2, 0.0, None, 3)[0]["cluster_track"].tolist() == [0, 0, 0]
    assert tt.link_timed(slow, slow["node_ptr"], [0, 1, 5], 0.2, 0.0, None, 3, max_dt=3.5)[0]["cluster_track"].tolist() == [0, 0, 1]
    # the gate grows with the time, not with the level: 0.9 away after dt = 2.5 is inside 0.4 * 2.5 at level 0, outside 0.4 * 1
    far = _points([[(0.0, 0.0)], [(0.9, 0.0)]])
    assert tt.link_timed(far, far["node_ptr"], [0, 2.5], 0.4, 0.0, None, 2)[0]["cluster_track"].tolist() == [0, 0]
    assert tt.link_timed(far, far["node_ptr"], [0, 1], 0.4, 0.0, None, 2)[0]["cluster_track"].tolist() == [0, 1]


def test_the_oracle_refuses_bad_times():
    s = walker([0, 1, 2])
    for bad in ([0, 1], [0, 1, 2, 3], [0, 1, 1], [0, 2, 1], [0, 1, float("nan")], [0, 1, float("inf")], [0, 1, "2"], [0, 1, 2j], [0, True, 2]):
        with pytest.raises(ValueError):
            tt.link_timed(s, s["node_ptr"], bad, 1.0, 0.0)
    _, state = tt.link_timed(s, s["node_ptr"], [0, 1, 2], 1.0, 0.0)
    for bad in ([2, 3, 4], [1.5, 3, 4]):
        with pytest.raises(ValueError):
            tt.link_timed(s, s["node_ptr"], bad, 1.0, 0.0, state=state)
    for bad in (0, -1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            tt.link_timed(s, s["node_ptr"], [0, 1, 2], 1.0, 0.0, max_dt=bad)


# ---- the front end, without a GPU ------------------------------------------------------------------------------------------------------
def _cpu_summaries(frames):
    import torch
    from gnn_cca_amd.tracking import ClusterSummaries
    s = _points(frames)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n = len(s["rank"])
    ones = torch.ones(n, dtype=torch.int32)
    return ClusterSummaries(t(s["count"]), t(s["rank"]), ones, ones, t(s["pos"]), t(s["emb"]), s["node_ptr"].tolist(),
                            t(s["node_ptr"].astype(np.int32)))


def test_the_linker_takes_max_dt_and_times():
    from gnn_cca_amd import tracking
    from gnn_cca_amd.tracking import FrameLinker
    assert FrameLinker(1.0).max_dt == 1.0 and FrameLinker(1.0, max_gap=3).max_dt == 4.0 and FrameLinker(1.0, max_gap=3, max_dt=None).max_dt == 4.0
    assert FrameLinker(1.0, max_gap=1, max_dt=2.5).max_dt == 2.5 and FrameLinker(1.0, max_dt=7).max_dt == 7.0
    assert FrameLinker(1.0, max_gap=2, motion="velocity", max_dt=np.float64(3.5)).max_dt == 3.5
    assert FrameLinker(1.0, matching="optimal", max_dt=0.5).max_dt == 0.5
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "2", True, 1j, [2.0]):
        with pytest.raises(ValueError, match="max_dt"):
            FrameLinker(1.0, max_gap=1, max_dt=bad)
    call = inspect.signature(FrameLinker.__call__).parameters
    assert list(call) == ["self", "x", "times"] and call["times"].default is None
    assert inspect.signature(FrameLinker.__init__).parameters["max_dt"].default is None
    assert len(tracking.__all__) == 10


@pytest.mark.parametrize("kw", [dict(), dict(max_gap=2), dict(matching="optimal", max_gap=1), dict(motion="velocity", max_gap=2)])
def test_bad_times_are_refused_before_the_gpu(kw):
    """CPU tensors: a refusal that came after the GPU was touched would not be a ValueError."""
    from gnn_cca_amd.tracking import FrameLinker
    link = FrameLinker(1.0, lam=0.0, **kw)
    s = _cpu_summaries([[(0.0, 0.0)], [(0.1, 0.0)], [(0.2, 0.0)]])
    for bad in ([0, 1], [0, 1, 2, 3], [], 5.0, "012", [0, 1, 1], [0, 2, 1], [2, 1, 0], [0, 1, float("nan")], [0, float("inf"), 2],
                [0, 1, -float("inf")], [0, 1, "2"], [0, 1, 2j], [0, True, 2], [0, 1, None], np.array([0.0, 1.0, np.nan]),
                np.zeros((3, 1)), np.array([0, 1, 2], dtype=np.complex128)):
        with pytest.raises(ValueError):
            link(s, times=bad)
        assert link._state is None and link._frame_rows == [] and link._frame_times == [] and link._state_timed is None
    link.max_dt = float("nan")
    with pytest.raises(ValueError, match="max_dt"):
        link(s, times=[0, 1, 2])
    link.max_dt = 1.0
    # a state written without time stamps is not continued with them, nor the reverse; a time not after the previous call's last
    link._state, link._state_timed, link._state_motion, link._reid_dim = object(), False, link.motion, 0
    link._frame_rows = [] if not kw else [1]
    with pytest.raises(ValueError, match=r"reset\(\) it first"):
        link(s, times=[0, 1, 2])
    link._state_timed, link._frame_rows, link._frame_times = True, [1], [2.0]
    with pytest.raises(ValueError, match=r"reset\(\) it first"):
        link(s)
    for bad in ([2, 3, 4], [1.5, 3, 4], [-1, 0, 1]):
        with pytest.raises(ValueError, match="previous call"):
            link(s, times=bad)
    assert link._frame_times == [2.0] and link._frame_rows == [1] and link._state_timed is True
    link.reset()
    assert link._state is None and link._frame_times == [] and link._state_timed is None


def test_the_binding_declares_the_timed_entries():
    import os
    import re
    from conftest import ROOT
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    for name, base in (("gnncca_link_frames_gap_timed", "gnncca_link_frames_gap_ex"), ("gnncca_link_frames_motion_timed", "gnncca_link_frames_motion")):
        assert name in nat.exported_symbols()
        decl = re.search(r"GNNCCA_API\s+int\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        args = nat._SIGNATURES[name][1]
        assert len(decl.split(",")) == len(args) == len(nat._SIGNATURES[base][1]) + 2   # frame_time_dev, max_dt
        assert args[:-2] == nat._SIGNATURES[base][1] and decl.split(",")[-2].split()[-1] == "frame_time_dev" and decl.split(",")[-1].split() == ["double", "max_dt"]
    # the rule stands in the header, the module docstring and the oracle in the same words
    import gnn_cca_amd.tracking as tracking
    flat = lambda text: " ".join(text.replace("*", " ").split())
    for sentence in ("finite, strictly increasing, the first strictly greater than the last time of the previous call",
                     "the other frame is still s = t - 1 - k, counted in frames PRESENT",
                     "pred(b) = pos(b) + dt * vel(b) and vel(a) = (pos(a) - pos(b)) / dt",
                     "cost = d / gate + lam * dcos, ties, mutual best or the assignment with miss_cost, the numbering of fresh ids, and matched_gap (still the level k)"):
        for where in (header, tracking.__doc__, tt.__doc__, open(os.path.join(ROOT, "DESIGN.md")).read()):
            assert flat(sentence) in flat(where), sentence


def test_the_timed_entries_check_their_arguments_before_any_launch():
    """No device needed: the argument checks come first and the (fake) device pointers are never followed."""
    import ctypes as C
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000

    def gap(n=5, g=1, gap=2, matching=0, miss=1.0, times=fake, max_dt=3.0, rows_in=(10, 20), rows_out=(10, 20, 5), ws_bytes=1 << 20):
        c_in, c_out = (C.c_int32 * max(len(rows_in), 1))(*rows_in), (C.c_int32 * max(len(rows_out), 1))(*rows_out)
        return lib.gnncca_link_frames_gap_timed(fake, fake, fake, fake, None, 0, n, g, 5, 1.0, 0.0, 0, 0.0, gap, matching, miss, fake, c_in,
                                                len(rows_in), fake, c_out, len(rows_out), fake, fake, fake, fake, fake, ws_bytes, None, times, max_dt)

    def motion(n=5, g=1, gap=2, mot=1, times=fake, max_dt=3.0, rows_in=(10, 20), rows_out=(10, 20, 5), velocity=fake, ws_bytes=1 << 20):
        c_in, c_out = (C.c_int32 * max(len(rows_in), 1))(*rows_in), (C.c_int32 * max(len(rows_out), 1))(*rows_out)
        return lib.gnncca_link_frames_motion_timed(fake, fake, fake, fake, None, 0, n, g, 5, 1.0, 0.0, 0, 0.0, gap, mot, fake, c_in, len(rows_in),
                                                   fake, c_out, len(rows_out), fake, fake, fake, fake, velocity, fake, ws_bytes, None, times, max_dt)

    for call in (gap, motion):
        assert call(g=0) == nat.OK and call(g=0, times=None) == nat.OK   # no frames: nothing is launched, nothing written
        for bad in (dict(times=None), dict(max_dt=0.0), dict(max_dt=-1.0), dict(max_dt=float("nan")), dict(max_dt=float("inf")), dict(gap=-1),
                    dict(gap=nat.TRACK_MAX_GAP + 1), dict(rows_in=(10, 4097)), dict(rows_in=(1, 2, 3, 4)), dict(n=-1)):
            assert call(**bad) == nat.ERR_INVALID_ARG, (call.__name__, bad)
        assert call(ws_bytes=16) == nat.ERR_WORKSPACE
    assert gap(matching=2) == nat.ERR_INVALID_ARG and gap(miss=0.0) == nat.ERR_INVALID_ARG and gap(matching=1, rows_in=(10, 129)) == nat.ERR_INVALID_ARG
    assert motion(mot=0) == nat.ERR_INVALID_ARG and motion(velocity=None) == nat.ERR_INVALID_ARG
