"""tests/track_score_oracle.py pinned down without a GPU: a hand-worked sequence whose every output is written out here, IDTP against brute
force over permutations, the duplicate and out-of-range rules, cut invariance with a carried state, and what TrackScorer refuses before
it touches a device."""
import itertools
import math

import numpy as np
import pytest
import torch

import track_score_oracle as ts

# 11 detections in 4 frames (frame 2 is empty), max_ids = 4, max_cams = 2.            stream   scored?  prev -> track
HAND = [  # (person, cam, track)
    (0, 0, 10),    # 0  frame 0                                                        (0, 0)   yes      none -> 10: 0
    (0, 1, 10),    # 1                                                                 (0, 1)   yes      none -> 10: 0
    (1, 0, 11),    # 2                                                                 (1, 0)   yes      none -> 11: 0
    (0, 0, 10),    # 3  frame 1: loses its (id, cam) to detection 5                    (0, 0)   no
    (1, 0, 10),    # 4                                                                 (1, 0)   yes      11 -> 10: 1
    (0, 0, 12),    # 5                                                                 (0, 0)   yes      10 -> 12: 1
    (0, 1, 10),    # 6  frame 3: two frames after detection 1                          (0, 1)   yes      10 -> 10: 0
    (-1, 0, 5),    # 7  no ground truth                                                         no
    (1, 0, 11),    # 8                                                                 (1, 0)   yes      10 -> 11: 1
    (2, 1, -1),    # 9  a refused frame's track                                                 no
    (2, 0, 13)]    # 10                                                                (2, 0)   yes      none -> 13: 0
HAND_PTR = [0, 3, 6, 6, 11]


def _hand():
    a = np.array(HAND, np.int64)
    return a[:, 0], a[:, 1].astype(np.int32), a[:, 2]


def test_a_hand_worked_sequence():
    ids, cam, track = _hand()
    sw, counts, res = ts.score(ids, cam, track, HAND_PTR, 4, 2)
    assert sw.dtype == np.int32 and sw.tolist() == [0, 0, 0, -1, 1, 1, 0, -1, 1, -1, 0]
    assert counts == [8, 3, 3, 5]
    # n: person 0 {10: 3, 12: 1}, person 1 {10: 1, 11: 2}, person 2 {13: 1};  rows 4, 3, 1;  columns 10: 4, 11: 2, 12: 1, 13: 1
    want = {"detections": 8, "ignored": 3, "ids": 3, "tracks": 4, "pairs": 5, "IDSW": 3,
            "IDTP": 6,                                                    # 0 -> 10 (3), 1 -> 11 (2), 2 -> 13 (1)
            "IDF1": 6 / 8,
            "AssA": math.fsum([9 / 5, 1 / 4, 1 / 6, 4 / 3, 1 / 1]) / 8,   # n n / (row + col - n) in ascending (p, t)
            "purity": 7 / 8,                                              # 3 + 2 + 1 + 1
            "coverage": 6 / 8,                                            # 3 + 2 + 1
            "MT": 1, "PT": 2, "ML": 0,                                    # shares 3/4, 2/3, 1/1
            "tracks_per_id": 5 / 3}
    assert res == want and list(res) == list(want)
    assert abs(res["AssA"] - 0.56875) < 1e-15


def test_idtp_is_the_maximum_over_all_assignments():
    rng = np.random.default_rng(0)
    shapes = [(1, 1), (1, 6), (6, 1), (6, 6), (5, 6), (6, 4)] + [tuple(rng.integers(1, 7, size=2)) for _ in range(30)]
    ties = 0
    for r, c in shapes:
        table = rng.integers(0, 6, size=(r, c)) * (rng.random((r, c)) < 0.6)   # sparse, small values: many equal totals
        if not table.any():
            table[0, 0] = 1
        cells = [(p, 100 + t, int(table[p, t])) for p in range(r) for t in range(c) if table[p, t]]
        best = ts.idtp_brute(table)
        assert ts.idtp(cells) == best, table
        wide = table if r <= c else table.T   # how many assignments reach the maximum: it is unique even where they are not
        ties += int(sum(sum(int(wide[i, perm[i]]) for i in range(len(wide))) == best
                        for perm in itertools.permutations(range(wide.shape[1]), len(wide))) > 1)
    assert ties > 0
    assert ts.idtp_brute([[3, 1], [1, 2], [0, 5]]) == 8 and ts.idtp_brute(np.zeros((0, 3))) == 0


def test_duplicates_and_values_out_of_range_are_ignored():
    # one frame; max_ids = 3, max_cams = 2.  Only the LARGEST node id of a VALID duplicate group is scored.
    rows = [(1, 0, 7),        # 0  loses to 4
            (1, 0, 8),        # 1  loses to 4
            (3, 0, 7),        # 2  id == max_ids
            (0, 2, 7),        # 3  cam == max_cams
            (1, 0, 9),        # 4  scored
            (1, 0, -1),       # 5  same (id, cam) as 4 and a larger node id, but NOT valid: it does not take 4's place
            (2, 1, 2 ** 40),  # 6  track == 2**40
            (2, 1, 2 ** 40 - 1),   # 7  scored: the largest track there is
            (0, -1, 7),       # 8  negative cam
            (-5, 0, 7)]       # 9  negative id
    a = np.array(rows, np.int64)
    sw, counts, res = ts.score(a[:, 0], a[:, 1].astype(np.int32), a[:, 2], [0, len(rows)], 3, 2)
    assert sw.tolist() == [-1, -1, -1, -1, 0, -1, -1, 0, -1, -1]
    assert counts == [2, 8, 0, 2]
    assert res["detections"] == 2 and res["ignored"] == 8 and res["IDTP"] == 2 and res["IDF1"] == 1.0 and res["AssA"] == 1.0
    # the same detections in the next frame with other tracks: the two scored streams switch, nobody else is looked at
    st = ts.new_state()
    ts.add(st, a[:, 0], a[:, 1].astype(np.int32), a[:, 2], [0, len(rows)], 3, 2)
    sw2 = ts.add(st, a[:, 0], a[:, 1].astype(np.int32), np.where(a[:, 2] >= 0, a[:, 2] // 2, -1), [0, len(rows)], 3, 2)
    assert sw2.tolist() == [-1, -1, -1, -1, 1, -1, -1, 1, -1, -1] and ts.counts(st) == [4, 16, 2, 4]
    with pytest.raises(ValueError):
        ts.result(ts.new_state())


def test_the_scores_do_not_depend_on_the_cuts():
    rng = np.random.default_rng(5)
    g, per = 12, 30
    sizes = rng.integers(0, per, size=g)
    sizes[4] = 0
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(ptr[-1])
    ids, cam, track = rng.integers(-1, 9, size=n), rng.integers(0, 4, size=n).astype(np.int32), rng.integers(-1, 12, size=n)
    sw, counts, res = ts.score(ids, cam, track, ptr, 8, 3)
    assert counts[1] > 0 and counts[2] > 0 and (sw == 0).any()
    for cuts in (((0, 5), (5, 6), (6, 6), (6, 7), (7, 12)), tuple((q, q + 1) for q in range(g)), ((0, 0), (0, 12))):
        st, parts, reach = ts.new_state(), [], 0
        for lo, hi in cuts:
            sl = slice(int(ptr[lo]), int(ptr[hi]))
            alone = ts.add(ts.new_state(), ids[sl], cam[sl], track[sl], ptr[lo:hi + 1] - ptr[lo], 8, 3)
            parts.append(ts.add(st, ids[sl], cam[sl], track[sl], ptr[lo:hi + 1] - ptr[lo], 8, 3))
            reach += int(((parts[-1] == 1) & (alone == 0)).sum())   # switches whose `prev` lies in an earlier call
        assert len(cuts) == 2 or reach > 0
        assert np.array_equal(np.concatenate(parts), sw) and ts.counts(st) == counts and ts.result(st) == res


def test_what_the_scorer_refuses_without_a_gpu():
    from gnn_cca_amd import tracking
    from gnn_cca_amd.tracking import TrackScorer
    assert "TrackScorer" in tracking.__all__
    for bad in (dict(max_ids=0), dict(max_ids=65537), dict(max_ids=2.0), dict(max_ids=True), dict(max_cams=0), dict(max_cams=65),
                dict(max_cams="4"), dict(max_ids=65536, max_cams=17), dict(max_ids=32768, max_cams=64)):
        with pytest.raises(ValueError):
            TrackScorer(**bad)
    assert TrackScorer(65536, 16).n_streams == 2 ** 20 and TrackScorer(16384, 64).n_streams == 2 ** 20
    s = TrackScorer()
    assert (s.max_ids, s.max_cams, s.cap) == (1024, 8, 0) and s.counts.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        s.result()
    i64, i32 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    for args in ((i32, i32, i64, [0, 4]),            # ids of the wrong dtype
                 (i64, i64, i64, [0, 4]),            # cam of the wrong dtype
                 (i64, i32, i32, [0, 4]),            # node_track of the wrong dtype
                 (i64, i32[:3], i64, [0, 4]),        # lengths
                 (i64, i32, i64, [0, 3]),            # node_ptr does not end at N
                 (i64, i32, i64, [1, 4]),            # ... or start at 0
                 (i64, i32, i64, [0, 5, 4]),         # ... or goes backwards
                 (i64, i32, i64, [])):
        with pytest.raises(ValueError):
            s.add_raw(*args)
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        s.add_raw(i64, i32, i64, [0, 4])
    with pytest.raises(ValueError):
        s.add(object(), None)
    assert s.cap == 0
