"""TrackScorer on the GPU against tests/track_score_oracle.py: `switched` and `counts` by torch.equal, result() by == -- over single-camera
sequences with occlusions, a multi-camera batch with duplicates and ids out of range, a sequence cut into calls, a pair table that is
rehashed while it fills, the edges of the index space (streams that are no multiple of a wave, a batch cut into several native calls, a
frame of 5000 detections, empty frames, no detections) and through FramePipeline results.  Every case first asserts, on the ORACLE's
numbers, that it exercises what it is about."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import track_score_oracle as ts
import tracking_gap_oracle as tg
import tracking_oracle as to

pytestmark = pytest.mark.gpu


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


def _add(score, ids, cam, track, ptr, lo=0, hi=None):
    """Frames lo .. hi of a host sequence through add_raw -> the device `switched` of those frames."""
    ptr = np.asarray(ptr, np.int64)
    hi = len(ptr) - 1 if hi is None else hi
    v0, v1 = int(ptr[lo]), int(ptr[hi])
    return score.add_raw(_dev(ids[v0:v1], np.int64), _dev(cam[v0:v1], np.int32), _dev(track[v0:v1], np.int64), (ptr[lo:hi + 1] - v0).tolist()).switched


def _same(score, switched, want):
    """`want`: the oracle's (switched, counts, result) for everything the scorer has seen."""
    sw, counts, res = want
    torch.cuda.synchronize()
    assert switched.dtype == torch.int32 and torch.equal(switched.cpu(), torch.from_numpy(sw))
    assert score.counts.dtype == torch.int64 and score.counts.is_cuda and torch.equal(score.counts.cpu(), torch.tensor(counts))
    got = score.result()
    assert got == res and list(got) == list(res), (got, res)


# ---- 1. single-camera hide sequences ----------------------------------------------------------------------------------------------------
HIDE = {1: dict(want={0: (56, 144, 140), 1: (32, 120, 105)}), 4: dict(want={0: (31, 68, 66), 2: (10, 47, 37)})}   # gap: IDSW, pairs, tracks


@pytest.mark.parametrize("seed,gap", [(1, 0), (1, 1), (4, 0), (4, 2)])
def test_hide_sequences(seed, gap):
    from test_gpu_tracking_gap import HIDE_CASES
    from gnn_cca_amd.tracking import TrackScorer
    persons, arena, lam, max_cos, m, empty, _ = [c for c in HIDE_CASES if c[-1] == seed][0]
    summ = tg.hide_sequence(np.random.default_rng(seed), 12, persons, 16, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=arena, empty=empty)
    assert gap in (0, m)
    track = tg.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, gap)[0]["node_track"]
    ids, cam = summ["person"], np.zeros(len(summ["person"]), np.int32)
    want = ts.score(ids, cam, track, summ["node_ptr"], 1024, 8)
    res = want[2]
    print(res)
    assert (res["IDSW"], res["pairs"], res["tracks"]) == HIDE[seed]["want"][gap]
    assert res["IDSW"] > 0 and res["pairs"] > res["tracks"] and res["tracks_per_id"] > 1 and res["pairs"] > res["ids"]
    by_person = {}
    for p, t in zip(ids.tolist(), track.tolist()):
        by_person.setdefault(p, set()).add(t)
    assert max(len(v) for v in by_person.values()) >= 2    # some person has two tracks
    score = TrackScorer()
    _same(score, _add(score, ids, cam, track, summ["node_ptr"]), want)


# ---- 2. multi-camera --------------------------------------------------------------------------------------------------------------------
def multi_camera():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import time_tracking
    b = time_tracking.make_batch(12, 3, 5, 8, seed=3, hide=0.2)
    ids = np.tile(np.tile(np.arange(5), 3), 12).astype(np.int64)
    summ = to.summaries(b["labels"], b["node_ptr"], b["xw"], b["yw"], b["cam"], b["emb"])
    tracks = {m: tg.link_gap(summ, b["node_ptr"], 0.8, max_gap=m)[0]["node_track"] for m in (0, 1, 2)}
    return ids, b["cam"].astype(np.int32), tracks, b["node_ptr"]


def test_multi_camera_batch():
    from gnn_cca_amd.tracking import TrackScorer
    ids, cam, tracks, ptr = multi_camera()
    idf1 = {}
    for m in (0, 1, 2):
        want = ts.score(ids, cam, tracks[m], ptr, 1024, 8)
        idf1[m] = round(want[2]["IDF1"], 3)
        assert want[1][:3] == [180, 0, 57]
        score = TrackScorer()
        _same(score, _add(score, ids, cam, tracks[m], ptr), want)
    assert idf1 == {0: 0.533, 1: 0.733, 2: 0.817}
    # no ground truth, an id out of range, and a duplicate (id, cam) that the larger node id wins
    ids, cam = ids.copy(), cam.copy()
    ids[7], ids[20], ids[16], cam[16] = -1, 5000, ids[15], cam[15]
    want = ts.score(ids, cam, tracks[1], ptr, 1024, 8)
    assert want[1] == [177, 3, 58, 42] and want[2]["tracks"] == 41 and want[0][[7, 15, 16, 20]].tolist() == [-1, -1, 1, -1]
    score = TrackScorer()
    _same(score, _add(score, ids, cam, tracks[1], ptr), want)


# ---- 3. cuts ----------------------------------------------------------------------------------------------------------------------------
def test_the_scores_do_not_depend_on_the_cuts():
    from gnn_cca_amd.tracking import TrackScorer
    ids, cam, tracks, ptr = multi_camera()
    track = tracks[1]
    want = ts.score(ids, cam, track, ptr, 1024, 8)
    cuts = ((0, 5), (5, 6), (6, 7), (7, 12))
    reach = 0
    st = ts.new_state()
    for lo, hi in cuts:   # a switch whose `prev` lies in an earlier call: scored alone, the same detection is no switch
        sl = slice(int(ptr[lo]), int(ptr[hi]))
        alone = ts.add(ts.new_state(), ids[sl], cam[sl], track[sl], ptr[lo:hi + 1] - ptr[lo], 1024, 8)
        reach += int(((ts.add(st, ids[sl], cam[sl], track[sl], ptr[lo:hi + 1] - ptr[lo], 1024, 8) == 1) & (alone == 0)).sum())
    print("switches whose prev lies in an earlier call:", reach)
    assert reach > 0
    whole = TrackScorer()
    sw_whole = _add(whole, ids, cam, track, ptr)
    _same(whole, sw_whole, want)
    score, parts = TrackScorer(), []
    for lo, hi in cuts:
        parts.append(_add(score, ids, cam, track, ptr, lo, hi))
        if hi == 6:   # an empty call in between changes nothing
            before = score.counts.clone()
            none = _add(score, ids, cam, track, ptr, 3, 3)
            assert none.numel() == 0 and none.dtype == torch.int32 and torch.equal(score.counts, before)
    _same(score, torch.cat(parts), want)
    assert torch.equal(torch.cat(parts), sw_whole) and score.result() == whole.result()
    score.reset()   # after reset() the first frames score as a sequence of their own
    assert score.cap == 0
    _same(score, _add(score, ids, cam, track, ptr, 0, 5), ts.score(ids[:ptr[5]], cam[:ptr[5]], track[:ptr[5]], ptr[:6], 1024, 8))


# ---- 4. table growth --------------------------------------------------------------------------------------------------------------------
def test_the_pair_table_is_rehashed_as_it_fills():
    from gnn_cca_amd.tracking import TrackScorer
    rng = np.random.default_rng(9)
    calls, frames, per = 7, 4, 100
    n = calls * frames * per
    ptr = np.arange(calls * frames + 1) * per
    ids, cam = rng.integers(0, 300, size=n), rng.integers(0, 4, size=n).astype(np.int32)
    track = rng.integers(0, 400, size=n) + np.where(rng.random(n) < 0.3, 2 ** 40 - 400, 0)   # both ends of the track range
    want = ts.score(ids, cam, track, ptr, 300, 4)
    print(want[1], want[2])
    assert want[1][3] >= 600 and want[1][1] > 0 and want[1][2] > 0     # >= 600 distinct pairs: probes collide in 1024 .. 8192 cells
    score, parts, caps, seen = TrackScorer(300, 4), [], [], []
    for c in range(calls):
        parts.append(_add(score, ids, cam, track, ptr, c * frames, (c + 1) * frames))
        caps.append(score.cap)
        seen.append((c + 1) * frames * per)
    assert seen[0] < 512 and seen[-1] > 2048
    assert caps == [1024, 2048, 4096, 4096, 4096, 8192, 8192]          # >= 2 x the detections seen: rehashed three times
    _same(score, torch.cat(parts), want)


# ---- 5. edges of the index space ----------------------------------------------------------------------------------------------------------
def _random_case(rng, sizes, max_ids, max_cams, n_tracks):
    """Ids and cams over the whole range and one past it on either side, tracks with -1 among them."""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(ptr[-1])
    ids = rng.integers(max(max_ids - 40, -1), max_ids + 1, size=n) if max_ids > 2000 else rng.integers(-1, max_ids + 1, size=n)
    cam = rng.integers(-1, max_cams + 1, size=n).astype(np.int32)
    return ids.astype(np.int64), cam, rng.integers(-1, n_tracks, size=n).astype(np.int64), ptr


def test_streams_that_are_no_multiple_of_a_wave_and_empty_frames():
    from gnn_cca_amd.tracking import TrackScorer
    ids, cam, track, ptr = _random_case(np.random.default_rng(2), [40, 0, 0, 55, 1, 0, 70, 0], 37, 3, 9)
    want = ts.score(ids, cam, track, ptr, 37, 3)
    scored = want[0] >= 0
    assert (ids[scored] == 36).any() and (cam[scored] == 2).any() and (ids[scored] == 0).any() and (cam[scored] == 0).any()
    assert (ids == 37).any() and (cam == 3).any() and want[1][1] > 0 and want[1][2] > 0
    score = TrackScorer(37, 3)
    _same(score, _add(score, ids, cam, track, ptr), want)


def test_a_batch_that_is_cut_into_three_native_calls():
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.tracking import TrackScorer
    ids, cam, track, ptr = _random_case(np.random.default_rng(3), [30, 25, 0, 30, 28, 31, 0, 0, 29, 30, 27, 33], 65536, 16, 6)
    want = ts.score(ids, cam, track, ptr, 65536, 16)
    scored = want[0] >= 0
    assert (ids[scored] == 65535).any() and (cam[scored] == 15).any() and (ids == 65536).any() and want[1][2] > 0
    score = TrackScorer(65536, 16)
    assert nat.SCORE_MAX_SLOTS // score.n_streams == 4 and len(ptr) - 1 == 12   # runs of 4 frames: three native calls
    frame_of = np.repeat(np.arange(12), np.diff(ptr))
    assert all((want[0][(frame_of >= lo) & (frame_of < lo + 4)] == 1).any() for lo in (4, 8))   # switches in the later runs: `last` carried
    _same(score, _add(score, ids, cam, track, ptr), want)


def test_a_frame_of_5000_detections():
    from gnn_cca_amd.tracking import TrackScorer
    ids, cam, track, ptr = _random_case(np.random.default_rng(4), [5000, 300], 1024, 8, 50)
    want = ts.score(ids, cam, track, ptr, 1024, 8)
    assert want[1][0] > 2000 and want[1][1] > 1000 and want[1][2] > 0   # thousands scored, duplicates ignored, switches in frame 1
    score = TrackScorer()
    _same(score, _add(score, ids, cam, track, ptr), want)


def test_no_detections():
    from gnn_cca_amd.tracking import TrackScorer
    score = TrackScorer()
    e64, e32 = torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
    for ptr in ([0], [0, 0, 0]):   # no frames; two empty frames
        s = score.add_raw(e64, e32, e64, ptr)
        assert s.switched.numel() == 0 and s.switched.dtype == torch.int32 and s.switched.is_cuda
    torch.cuda.synchronize()
    assert score.counts.cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        score.result()
    ids, cam, track = np.array([3, 3]), np.array([1, 1], np.int32), np.array([5, 6])   # ... and then a sequence starts as usual
    _add(score, ids, cam, track, [0, 1, 2])
    assert score.result() == ts.score(ids, cam, track, [0, 1, 2], 1024, 8)[2] and score.result()["IDSW"] == 1


# ---- 6. through the pipeline --------------------------------------------------------------------------------------------------------------
def test_through_the_pipeline():
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.tracking import FrameLinker, TrackScorer
    # the blanked-frame construction of test_gpu_tracking_gap.test_a_blanked_frame_of_a_pipeline_result_is_bridged
    rng = np.random.default_rng(33)
    k, cams = 14, 4
    one = dict(id_cam=rng.integers(0, cams, size=k), ids=rng.integers(0, 6, size=k), xw=rng.uniform(-10, 10, k), yw=rng.uniform(-10, 10, k),
               node=rng.standard_normal((k, 2048)).astype(np.float32), reid=rng.standard_normal((k, 256)).astype(np.float32))
    f = {q: np.concatenate([one[q], one[q]]) for q in one}
    f["xw"][k:] += rng.normal(0, 0.05, k)
    f["yw"][k:] += rng.normal(0, 0.05, k)
    sizes, max_dist = np.array([k, 0, k]), np.array([50.0, 50.0, 50.0])
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    pipe = FramePipeline(m)
    args = (f["xw"], f["yw"], f["ids"], f["id_cam"], sizes, max_dist, node, reid)
    r = pipe(*args)
    with torch.no_grad():
        sd = m.state_dict()
        key = [q for q in sd if q.startswith("classifier.") and q.endswith(".bias")][-1]
        sd[key] -= r.outputs["classified_edges"][-1].median()
        m.load_state_dict(sd)
    r = pipe(*args)
    t1, t0 = FrameLinker(3.0, max_gap=1)(r), FrameLinker(3.0)(r)
    score = TrackScorer()
    s = score.add(r, t1)
    ids_h, ptr = r.batch.y.cpu().numpy(), np.asarray(r.batch.node_ptr, np.int64)
    assert np.array_equal(ids_h, f["ids"]) and ptr.tolist() == [0, k, k, 2 * k]
    cam_h = r.batch.cam_dev.cpu().numpy()
    assert cam_h.dtype == np.int32 and np.array_equal(cam_h, f["id_cam"])
    want = ts.score(ids_h, cam_h, t1.node_track.cpu().numpy(), ptr, 1024, 8)
    base = ts.score(ids_h, cam_h, t0.node_track.cpu().numpy(), ptr, 1024, 8)
    print("IDSW with max_gap=1:", want[2]["IDSW"], "without:", base[2]["IDSW"], "ignored:", want[1][1])
    assert base[2]["IDSW"] > want[2]["IDSW"]          # bridging the blank frame saves switches
    _same(score, s.switched, want)
    again = TrackScorer()
    _same(again, again.add(r.batch, t0).switched, base)   # a GraphBatch in place of the FrameResult
