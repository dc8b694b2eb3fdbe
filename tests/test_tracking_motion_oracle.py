"""The motion rule of gnn_cca_amd.tracking (FrameLinker(motion='velocity')) on its numpy restatement (tests/tracking_motion_oracle.py, which
the GPU tests compare the kernels with): without motion its frames-outside order is the gap rule, one hand-made crossing with every id
spelled out, zero velocities change nothing, cutting a sequence into batches changes nothing, a link at level k divides the displacement
by k + 1; and what the Python front end and the ctypes binding declare, which needs no GPU."""
import numpy as np
import pytest

import tracking_gap_oracle as tg
import tracking_motion_oracle as tm

FIELDS = ("cluster_track", "node_track", "matched_prev", "matched_gap")


def _points(frames):
    """frames: per frame a list of (x, y) -> the summaries of one-node clusters, without embeddings."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([p for f in frames for p in f], np.float64).reshape(n, 2)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, pos=pos, emb=np.zeros((n, 0), np.float32), node_ptr=node_ptr)


def crossing():
    """Two people walking through each other on parallel lines 0.25 apart, one unit per frame: (t, 0) and (5 - t, 0.25), t = 0 .. 5."""
    return _points([[(float(t), 0.0), (5.0 - t, 0.25)] for t in range(6)])


@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("lam,max_cos,empty,seed", [(1.0, None, (), 1), (0.5, 0.05, (5,), 2), (0.0, None, (4, 5), 3)])
def test_without_motion_the_frames_outside_order_is_the_gap_rule(m, lam, max_cos, empty, seed):
    summ = tg.hide_sequence(np.random.default_rng(seed), 12, 40, 16, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=9.0, empty=empty)
    want, wstate = tg.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    got, state = tm.link_motion(summ, summ["node_ptr"], 1.0, lam, max_cos, m, motion=False)
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), k
    assert got["next_id"] == want["next_id"] == state["next_id"]
    assert not got["velocity"].any()
    for a, b in zip(state["frames"], wstate["frames"]):
        assert all(np.array_equal(a[k], b[k]) for k in ("pos", "emb", "track", "succ"))


def test_two_people_crossing_by_hand():
    s = crossing()
    # without motion: from frame 2 to frame 3 each stands 0.25 from where the OTHER was and 1 from where it was itself
    none, _ = tm.link_motion(s, s["node_ptr"], max_step=1.5, lam=0.0, max_gap=0, motion=False)
    assert none["cluster_track"].tolist() == [0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0]
    gap, _ = tg.link_gap(s, s["node_ptr"], max_step=1.5, lam=0.0, max_gap=0)
    assert gap["cluster_track"].tolist() == none["cluster_track"].tolist()
    # with motion: each is looked for one unit further along its own line, where it is; the other is looked for 1.03 away
    out, state = tm.link_motion(s, s["node_ptr"], max_step=1.5, lam=0.0, max_gap=0)
    assert out["cluster_track"].tolist() == [0, 1] * 6 and out["next_id"] == 2
    assert out["matched_prev"].tolist() == [-1, -1] + [0, 1] * 5 and out["matched_gap"].tolist() == [-1, -1] + [0, 0] * 5
    assert out["velocity"].tolist() == [[0.0, 0.0]] * 2 + [[1.0, 0.0], [-1.0, 0.0]] * 5
    assert len(state["frames"]) == 1 and state["frames"][0]["vel"].tolist() == [[1.0, 0.0], [-1.0, 0.0]]
    assert tm.switches([0, 1] * 6, out["cluster_track"], s["node_ptr"]) == 0
    assert tm.switches([0, 1] * 6, none["cluster_track"], s["node_ptr"]) == 2
    # max_step bounds the deviation from the prediction: a sharp turn ends the track although the step itself is short
    turn = _points([[(0.0, 0.0)], [(1.0, 0.0)], [(1.0, 0.8)]])
    assert tm.link_motion(turn, turn["node_ptr"], 1.0, 0.0, None, 0)[0]["cluster_track"].tolist() == [0, 0, 1]   # (2, 0) to (1, 0.8): 1.28
    assert tm.link_motion(turn, turn["node_ptr"], 1.0, 0.0, None, 0, motion=False)[0]["cluster_track"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("m", [0, 2])
def test_people_who_stand_still_link_as_under_the_gap_rule(m):
    rng = np.random.default_rng(5)
    base = tg.hide_sequence(rng, 1, 30, 8, p_leave=0.0, p_enter=0.0, arena=6.0)
    c = int(base["count"][0])
    # every frame repeats the same positions (in another order, some rows missing): the displacement of every link is exactly zero
    frames = []
    for q in range(8):
        keep = rng.permutation(c)[:c - (q % 3)]
        frames.append((base["pos"][keep], base["emb"][keep]))
    counts = [len(p) for p, _ in frames]
    n = sum(counts)
    summ = dict(count=np.array(counts, np.int32), rank=np.concatenate([np.arange(k) for k in counts]).astype(np.int32),
                pos=np.concatenate([p for p, _ in frames]), emb=np.concatenate([e for _, e in frames]),
                node_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    got, _ = tm.link_motion(summ, summ["node_ptr"], 0.5, 1.0, None, m)
    want, _ = tg.link_gap(summ, summ["node_ptr"], 0.5, 1.0, None, m)
    assert (got["matched_gap"] >= 0).sum() > n // 2 and (m == 0 or (got["matched_gap"] >= 1).any())
    assert not got["velocity"].any()
    for k in FIELDS:
        assert np.array_equal(got[k], want[k]), k
    assert got["next_id"] == want["next_id"]


@pytest.mark.parametrize("m", [0, 2])
def test_cutting_a_sequence_into_batches_changes_nothing(m):
    summ = tm.cross_sequence(np.random.default_rng(30 + m), 12, 25, 8, p_hide=0.12 if m else 0.0, max_hide=m + 1, arena=6.0)
    whole, wstate = tm.link_motion(summ, summ["node_ptr"], 0.4, 1.0, None, m)
    assert all((whole["matched_gap"] == k).any() for k in range(m + 1)) and whole["velocity"].any()
    state, parts = None, []
    for lo, hi in ((0, 5), (5, 6), (3, 3), (6, 12)):   # (3, 3): a call without frames passes no time
        part = tg.frames_of(summ, lo, hi)
        out, state = tm.link_motion(part, part["node_ptr"], 0.4, 1.0, None, m, state)
        parts.append(out)
    for k in FIELDS + ("velocity",):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    assert parts[-1]["next_id"] == whole["next_id"] == state["next_id"]
    assert len(state["frames"]) == len(wstate["frames"]) == m + 1
    for a, b in zip(state["frames"], wstate["frames"]):
        assert a["count"] == b["count"] and all(np.array_equal(a[k], b[k]) for k in ("pos", "vel", "emb", "track", "succ"))


def test_a_link_over_a_gap_divides_the_displacement_by_the_frames_gone_by():
    # one person at x = 0, 1, (hidden, hidden), 4.5: found at level 2 under gate 3 at 4.5 - (1 + 3 * 1) = 0.5 from the prediction
    s = _points([[(0.0, 7.0)], [(1.0, 7.0)], [], [], [(4.5, 7.75)]])
    out, state = tm.link_motion(s, s["node_ptr"], max_step=1.0, lam=0.0, max_gap=2)
    assert out["cluster_track"].tolist() == [0, 0, 0] and out["matched_gap"].tolist() == [-1, 0, 2]
    assert out["velocity"].tolist() == [[0.0, 0.0], [1.0, 0.0], [3.5 / 3.0, 0.75 / 3.0]]
    assert out["velocity"][2, 0] == (np.float64(4.5) - np.float64(1.0)) / np.float64(3)
    # without the prediction the same person is 3.58 away: outside gate 3
    assert tm.link_motion(s, s["node_ptr"], 1.0, 0.0, None, 2, motion=False)[0]["cluster_track"].tolist() == [0, 0, 1]
    # the table of level k sees the prediction over k + 1 frames
    tables = tm.level_tables(s, s["node_ptr"], 1.0, 0.0, None, 2)
    assert [(k, t) for k, t, *_ in tables] == [(0, 1), (2, 4)] and tables[1][2].tolist() == [[np.sqrt(0.5 * 0.5 + 0.75 * 0.75)]]


def test_the_linker_validates_motion_before_the_gpu():
    from gnn_cca_amd import tracking
    from gnn_cca_amd.tracking import FrameLinker, Tracks
    for bad in ("Velocity", "kalman", "", None, 1, True, b"velocity"):
        with pytest.raises(ValueError):
            FrameLinker(1.0, motion=bad)
    with pytest.raises(ValueError):
        FrameLinker(1.0, matching="optimal", motion="velocity")
    assert FrameLinker(1.0).motion == "none" and FrameLinker(1.0, motion="none", matching="optimal").motion == "none"
    assert FrameLinker(1.0, max_gap=3, motion="velocity").motion == "velocity" and FrameLinker(1.0, motion="velocity").max_gap == 0
    assert "velocity" in Tracks.__slots__
    assert "MOTION" not in tracking.__all__ and len(tracking.__all__) == 10


def test_the_binding_declares_the_motion_entry():
    import os
    import re
    from conftest import ROOT
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    for name in ("gnncca_link_motion_state_bytes", "gnncca_link_motion_workspace_bytes", "gnncca_link_frames_motion"):
        assert name in nat.exported_symbols() and re.search(r"GNNCCA_API[^;(]*\b" + name + r"\s*\(", header), name
    assert nat.MOTION == {"none": 0, "velocity": 1}
    decl = re.search(r"GNNCCA_API\s+int\s+gnncca_link_frames_motion\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(nat._SIGNATURES["gnncca_link_frames_motion"][1])
    # the gap entry's arguments plus motion and velocity
    assert len(nat._SIGNATURES["gnncca_link_frames_motion"][1]) == len(nat._SIGNATURES["gnncca_link_frames_gap"][1]) + 2


def test_the_motion_entry_checks_its_arguments_before_any_launch():
    """No device needed: the argument checks come first and the (fake) device pointers are never followed."""
    import ctypes as C
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000

    def call(n=5, g=1, max_n=5, gap=2, motion=1, state_in=fake, rows_in=(10, 20), rows_out=(10, 20, 5), frames_out=None, velocity=fake,
             max_step=1.0, ws_bytes=1 << 20):
        c_in, c_out = (C.c_int32 * max(len(rows_in), 1))(*rows_in), (C.c_int32 * max(len(rows_out), 1))(*rows_out)
        return lib.gnncca_link_frames_motion(fake, fake, fake, fake, None, 0, n, g, max_n, max_step, 0.0, 0, 0.0, gap, motion, state_in, c_in,
                                             len(rows_in), fake, c_out, len(rows_out) if frames_out is None else frames_out, fake, fake, fake,
                                             fake, velocity, fake, ws_bytes, None)

    assert call(g=0) == nat.OK                                                     # no frames: nothing is launched, nothing written
    for bad in (dict(motion=0), dict(motion=2), dict(motion=-1), dict(gap=-1), dict(gap=nat.TRACK_MAX_GAP + 1), dict(max_n=4097),
                dict(rows_in=(10, 4097)), dict(rows_out=(10, 4097, 5)), dict(rows_in=(1, 2, 3, 4)), dict(frames_out=2), dict(velocity=None),
                dict(max_step=0.0), dict(max_step=float("inf")), dict(state_in=None, rows_in=(10, 20)), dict(n=-1)):
        assert call(**bad) == nat.ERR_INVALID_ARG, bad
    assert call(ws_bytes=16) == nat.ERR_WORKSPACE
    # the sizes: the velocities are 16 more bytes per row than the gap state, and the 8-byte arrays come first
    assert lib.gnncca_link_motion_state_bytes(100, 3, 16) >= lib.gnncca_link_gap_state_bytes(100, 3, 16) + 1600 - 256
    assert lib.gnncca_link_motion_state_bytes(100, 3, 16) >= 64 + 100 * (16 + 16 + 8 + 64 + 4)
    assert lib.gnncca_link_motion_state_bytes(-1, 3, 16) == 0 and lib.gnncca_link_motion_state_bytes(1, 10, 16) == 0
    assert lib.gnncca_link_motion_workspace_bytes(1000, 12, 500) >= 1500 * 4 and lib.gnncca_link_motion_workspace_bytes(-1, 1, 0) == 0
