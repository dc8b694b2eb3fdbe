"""The gap-tolerant linking rule of gnn_cca_amd.tracking (FrameLinker(max_gap=M)) on its numpy restatement (tests/tracking_gap_oracle.py,
which the GPU tests compare the kernels with): level 0 alone is tracking_oracle.link, cutting a sequence into batches changes nothing, one
hand-written case with every id spelled out; and what the Python front end and the ctypes binding declare, which needs no GPU."""
import numpy as np
import pytest

import tracking_gap_oracle as tg
import tracking_oracle as to

CASES = [  # g, persons, seed, lam, max_cos, empty: the shapes tests/test_gpu_tracking.py links
    (1, 70, 1, 1.0, None, ()), (2, 70, 2, 1.0, None, ()), (9, 70, 3, 1.0, None, (4,)), (9, 70, 4, 0.5, 0.05, ()),
    (9, 70, 3, 0.0, None, (4,)), (9, 20, 6, 0.0, 1.0, (0,)), (12, 25, 21, 1.0, None, (7,))]


@pytest.mark.parametrize("g,persons,seed,lam,max_cos,empty", CASES)
def test_without_a_gap_the_rule_is_the_adjacent_frame_rule(g, persons, seed, lam, max_cos, empty):
    summ = to.walk_sequence(np.random.default_rng(seed), g, persons, 16, noise=0.3, p_leave=0.04, p_enter=0.6, arena=12.0, empty=empty)
    want, wstate = to.link(summ, summ["node_ptr"], 1.0, lam, max_cos)
    got, state = tg.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, 0)
    for k in ("cluster_track", "node_track", "matched_prev"):
        assert np.array_equal(got[k], want[k]), k
    assert got["next_id"] == want["next_id"] == state["next_id"]
    assert np.array_equal(got["matched_gap"], np.where(want["matched_prev"] >= 0, 0, -1))
    assert len(state["frames"]) == 1 and np.array_equal(state["frames"][0]["track"], wstate["track"])
    # ... and through a carried state: the second half continues the first
    if g >= 2:
        h = g // 2
        a, b = tg.frames_of(summ, 0, h), tg.frames_of(summ, h, g)
        w1, ws = to.link(a, a["node_ptr"], 1.0, lam, max_cos)
        w2, _ = to.link(b, b["node_ptr"], 1.0, lam, max_cos, ws)
        g1, gs = tg.link_gap(a, a["node_ptr"], 1.0, lam, max_cos, 0)
        g2, _ = tg.link_gap(b, b["node_ptr"], 1.0, lam, max_cos, 0, gs)
        assert np.array_equal(np.concatenate([g1["cluster_track"], g2["cluster_track"]]), want["cluster_track"])
        assert np.array_equal(g2["cluster_track"], w2["cluster_track"]) and g2["next_id"] == w2["next_id"] == want["next_id"]


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("cuts", [((0, 5), (5, 6), (6, 12)), ((0, 5), (5, 6), (6, 7), (7, 12)), ((0, 1), (1, 1), (1, 12))])
def test_cutting_a_sequence_into_batches_changes_nothing(m, cuts):
    summ = tg.hide_sequence(np.random.default_rng(40 + m), 12, 25, 8, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=8.0, empty=(7,))
    whole, wstate = tg.link_gap(summ, summ["node_ptr"], 1.0, 1.0, None, m)
    assert all((whole["matched_gap"] == k).any() for k in range(m + 1))
    state, parts = None, []
    for lo, hi in cuts:
        part = tg.frames_of(summ, lo, hi)
        out, state = tg.link_gap(part, part["node_ptr"], 1.0, 1.0, None, m, state)
        parts.append(out)
    for k in ("cluster_track", "node_track", "matched_prev", "matched_gap"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    assert parts[-1]["next_id"] == whole["next_id"] == state["next_id"]
    assert len(state["frames"]) == len(wstate["frames"]) == m + 1
    for a, b in zip(state["frames"], wstate["frames"]):
        assert a["count"] == b["count"] and all(np.array_equal(a[k], b[k]) for k in ("pos", "emb", "track", "succ"))


def _line(frames):
    """frames: per frame a list of x -> the summaries of one-node clusters on the line y = 0, without embeddings."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([(x, 0.0) for f in frames for x in f], np.float64).reshape(n, 2)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, pos=pos, emb=np.zeros((n, 0), np.float32), node_ptr=node_ptr)


def test_four_frames_by_hand():
    #            P     Q      S     T            R (new: 1.5 from S)    P again, c, T        Q again, T
    s = _line([[0.0, 10.0, 21.5, 30.0], [20.0, 30.1], [0.5, 20.9, 30.2], [10.0, 30.3]])
    out, state = tg.link_gap(s, s["node_ptr"], max_step=1.0, lam=0.0, max_gap=1)
    # P is hidden in frame 1 and found again in frame 2 (0.5 <= gate_1 = 2).  Q is hidden in frames 1 and 2: with max_gap = 1 nobody
    # looks that far back, Q gets a new id.  c (20.9, frame 2) is 0.9 from R of frame 1 (cost 0.9 at level 0) and 0.6 from S of frame 0
    # (cost 0.3 at level 1): level 0 runs first, so c continues R at the higher cost and S's track ends.
    assert out["cluster_track"].tolist() == [0, 1, 2, 3, 4, 3, 0, 4, 3, 5, 3]
    assert out["matched_prev"].tolist() == [-1, -1, -1, -1, -1, 3, 0, 0, 1, -1, 2]
    assert out["matched_gap"].tolist() == [-1, -1, -1, -1, -1, 0, 1, 0, 0, -1, 0]
    assert out["node_track"].tolist() == out["cluster_track"].tolist() and out["next_id"] == 6
    assert [f["track"].tolist() for f in state["frames"]] == [[0, 4, 3], [5, 3]]
    assert [f["succ"].tolist() for f in state["frames"]] == [[False, False, True], [False, False]]
    # with max_gap = 2 Q is found again (level 2, gate 3), and nothing else changes
    out2, _ = tg.link_gap(s, s["node_ptr"], max_step=1.0, lam=0.0, max_gap=2)
    assert out2["cluster_track"].tolist() == [0, 1, 2, 3, 4, 3, 0, 4, 3, 1, 3] and out2["next_id"] == 5
    assert out2["matched_prev"].tolist()[-2:] == [1, 2] and out2["matched_gap"].tolist()[-2:] == [2, 0]
    # without a gap P and Q both come back as strangers
    out0, _ = tg.link_gap(s, s["node_ptr"], max_step=1.0, lam=0.0, max_gap=0)
    assert out0["cluster_track"].tolist() == [0, 1, 2, 3, 4, 3, 5, 4, 3, 6, 3] and out0["next_id"] == 7
    # a gate is d <= max_step * (k + 1) exactly: P found again at 2.0 is on it, at 2.0 + 1 ulp outside
    for x, tid in ((2.0, 0), (np.nextafter(2.0, 3.0), 5)):
        s3 = _line([[0.0, 30.0], [30.0], [x, 30.0]])
        o3, _ = tg.link_gap(s3, s3["node_ptr"], max_step=1.0, lam=0.0, max_gap=1)
        assert o3["cluster_track"].tolist() == [0, 1, 1, tid if tid == 0 else 2, 1]
    # an empty frame and a refused one (count -1) still count as frames
    s4 = _line([[0.0], [], [0.0]])
    assert tg.link_gap(s4, s4["node_ptr"], 1.0, 0.0, None, 1)[0]["cluster_track"].tolist() == [0, 0]
    s5 = _line([[0.0], [5.0], [0.0]])
    s5["count"][1] = -1
    o5, _ = tg.link_gap(s5, s5["node_ptr"], 1.0, 0.0, None, 1)
    assert o5["cluster_track"].tolist() == [0, -1, 0] and o5["matched_gap"].tolist() == [-1, -1, 1]
    s6 = _line([[0.0], [], [], [0.0]])
    assert tg.link_gap(s6, s6["node_ptr"], 1.0, 0.0, None, 1)[0]["cluster_track"].tolist() == [0, 1]


def test_the_linker_validates_max_gap_before_the_gpu():
    from gnn_cca_amd.tracking import MAX_GAP, FrameLinker, Tracks
    assert MAX_GAP == tg.MAX_GAP == 8
    for bad in (-1, 9, True, False, 1.0, 1.5, "1", None, float("nan")):
        with pytest.raises(ValueError):
            FrameLinker(1.0, max_gap=bad)
        with pytest.raises(ValueError):
            tg.link_gap(_line([[0.0]]), [0, 1], 1.0, 0.0, None, bad)
    assert FrameLinker(1.0).max_gap == 0 and FrameLinker(1.0, max_gap=0).max_gap == 0
    assert FrameLinker(1.0, 0.0, None, 8).max_gap == 8 and FrameLinker(1.0, max_gap=np.int64(3)).max_gap == 3
    assert isinstance(Tracks.matched_gap, property)


def test_the_binding_declares_the_gap_entry():
    import os
    import re
    from conftest import ROOT
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    for name in ("gnncca_link_gap_state_bytes", "gnncca_link_gap_workspace_bytes", "gnncca_link_frames_gap"):
        assert name in nat.exported_symbols() and re.search(r"GNNCCA_API[^;(]*\b" + name + r"\s*\(", header), name
    assert int(re.search(r"#define GNNCCA_TRACK_MAX_GAP (\d+)", header).group(1)) == nat.TRACK_MAX_GAP == 8
    # the ctypes argument list has one entry per parameter of the declaration
    decl = re.search(r"GNNCCA_API\s+int\s+gnncca_link_frames_gap\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(nat._SIGNATURES["gnncca_link_frames_gap"][1])
    # the old entry's arguments plus max_gap, two (host rows, frames) pairs in place of two capacities, and matched_gap
    assert len(nat._SIGNATURES["gnncca_link_frames_gap"][1]) == len(nat._SIGNATURES["gnncca_link_frames"][1]) + 4


def test_the_gap_entry_checks_its_arguments_before_any_launch():
    """No device needed: the argument checks come first and the (fake) device pointers are never followed."""
    import ctypes as C
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000

    def call(n=5, g=1, max_n=5, gap=2, state_in=fake, rows_in=(10, 20), frames_in=None, rows_out=(10, 20, 5), frames_out=None, ws_bytes=1 << 20):
        c_in, c_out = (C.c_int32 * max(len(rows_in), 1))(*rows_in), (C.c_int32 * max(len(rows_out), 1))(*rows_out)
        return lib.gnncca_link_frames_gap(fake, fake, fake, fake, None, 0, n, g, max_n, 1.0, 0.0, 0, 0.0, gap, state_in, c_in,
                                          len(rows_in) if frames_in is None else frames_in, fake, c_out,
                                          len(rows_out) if frames_out is None else frames_out, fake, fake, fake, fake, fake, ws_bytes, None)

    assert call(g=0) == nat.OK                                                     # no frames: nothing is launched, nothing written
    for bad in (dict(gap=-1), dict(gap=nat.TRACK_MAX_GAP + 1), dict(max_n=4097), dict(rows_in=(10, 4097)), dict(rows_out=(10, 4097, 5)),
                dict(rows_out=(10, 20)), dict(gap=1, rows_in=(1, 2, 3), rows_out=(3, 5)), dict(state_in=None), dict(frames_in=-1)):
        assert call(**bad) == nat.ERR_INVALID_ARG, bad
    assert call(ws_bytes=16) == nat.ERR_WORKSPACE
    assert lib.gnncca_link_gap_state_bytes(35, 3, 16) >= 64 + 35 * (16 + 8 + 4 * 16 + 4)
    assert lib.gnncca_link_gap_state_bytes(35, nat.TRACK_MAX_GAP + 2, 16) == 0 and lib.gnncca_link_gap_state_bytes(-1, 1, 0) == 0
    assert lib.gnncca_link_gap_workspace_bytes(5, 1, 30) >= (30 + 2 * 5 + 2 * 1 + 1) * 4
