"""FrameLinker(...)(x, times=...) on the GPU against tests/tracking_time_oracle.py, for the four modes (adjacent, max_gap, matching='optimal',
motion='velocity'): cluster_track, node_track, matched_prev, matched_gap, next_id and, with motion, velocity EXACTLY.  With times
0, 1, 2, ... the timed linker is the untimed one bit for bit; dropped frames and jittered times follow the oracle; three cases by hand;
the result does not depend on how a timed sequence is cut into calls; frames wider than a wave; the refusals, which come before any launch
and leave the state and the host-side times alone; and a FramePipeline result.

The precondition of exact equality is the one of the older tracking tests: the kernel's float64 cosine sums differ from the oracle's in
summation order only (~R * 1e-16), so no decision of the oracle may hang on less than that; the seeds are chosen so that every margin of
margins_timed is >= 1e-5, which each case asserts before it looks at the device.  Every case also asserts, on the ORACLE's numbers, that
it exercises what it is about."""
import copy

import numpy as np
import pytest
import torch

import tracking_gap_oracle as tg
import tracking_motion_oracle as tm
import tracking_time_oracle as tt

pytestmark = pytest.mark.gpu

FIELDS = ("cluster_track", "node_track", "matched_prev", "matched_gap")
MARGIN = 1e-5

# the four modes: FrameLinker's keywords, max_step, lam, max_cos, and the seed of the mode's sequences
MODES = {
    "adjacent": dict(kw=dict(), max_step=0.6, lam=1.0, max_cos=None, seed=1),
    "gap": dict(kw=dict(max_gap=2), max_step=0.6, lam=0.5, max_cos=0.3, seed=2),
    "optimal": dict(kw=dict(max_gap=1, matching="optimal"), max_step=0.6, lam=1.0, max_cos=None, seed=3),
    "motion": dict(kw=dict(max_gap=2, motion="velocity"), max_step=0.4, lam=1.0, max_cos=None, seed=4),
}
DROPPED = (3, 7, 8)


def _upload(summ, lo=0, hi=None, dev="cuda"):
    """Frames lo .. hi of an oracle sequence as a ClusterSummaries on the device."""
    from gnn_cca_amd.tracking import ClusterSummaries
    ptr = np.asarray(summ["node_ptr"], np.int64)
    hi = len(ptr) - 1 if hi is None else hi
    v0, v1 = int(ptr[lo]), int(ptr[hi])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    local = ptr[lo:hi + 1] - v0
    ones = np.ones(v1 - v0, np.int32)
    return ClusterSummaries(t(summ["count"][lo:hi]), t(summ["rank"][v0:v1]), t(ones), t(ones), t(summ["pos"][v0:v1]), t(summ["emb"][v0:v1]),
                            local.tolist(), t(local.astype(np.int32)))


def _points(frames):
    """frames: per frame a list of (x, y) -> the summaries of one-node clusters, without embeddings."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([p for f in frames for p in f], np.float64).reshape(n, 2)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, pos=pos, emb=np.zeros((n, 0), np.float32), node_ptr=node_ptr)


def _oracle_kw(mode):
    """The keywords of tt.link_timed / margins_timed for a mode."""
    c = MODES[mode]
    return dict(max_step=c["max_step"], lam=c["lam"], max_cos=c["max_cos"], max_gap=c["kw"].get("max_gap", 0),
                matching=c["kw"].get("matching", "mutual"), motion=c["kw"].get("motion", "none") == "velocity")


def _linker(mode, **more):
    from gnn_cca_amd.tracking import FrameLinker
    c = MODES[mode]
    return FrameLinker(c["max_step"], lam=c["lam"], max_cos=c["max_cos"], **c["kw"], **more)


def sequence(mode, g):
    """g frames of at most 12 clusters, R = 16: people crossing each other for the motion mode, a noisy random walk with occlusions for
    the others (a step is outside the one-period gate about one time in eight, so the gate's growth with time decides links)."""
    c = MODES[mode]
    rng = np.random.default_rng(c["seed"])
    m = c["kw"].get("max_gap", 0)
    if mode == "motion":
        return tm.cross_sequence(rng, g, 10, 16, speed=(0.3, 0.6), noise=0.04, p_hide=0.1, max_hide=m, arena=8.0)
    return tg.hide_sequence(rng, g, 10, 16, noise=0.3, p_leave=0.05, p_enter=0.3, p_hide=0.1 if m else 0.0, max_hide=max(m, 1), arena=8.0,
                            max_alive=12)


def _margins(summ, times, mode, **more):
    gaps = tt.margins_timed(summ, summ["node_ptr"], times, **_oracle_kw(mode), **more)
    print(mode, "margins (cost, d, dcos):", gaps)
    assert all(v >= MARGIN for v in gaps), gaps


def _same_tracks(t, want, mode):
    torch.cuda.synchronize()
    keys = FIELDS + (("velocity",) if _oracle_kw(mode)["motion"] else ())
    for k in keys:
        got, ref = getattr(t, k).cpu(), torch.from_numpy(want[k])
        assert got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got, ref), (mode, k)
    if not _oracle_kw(mode)["motion"]:
        assert t.velocity is None
    assert t.next_id.dtype == torch.int64 and int(t.next_id.item()) == want["next_id"]


def _cat(parts, mode):
    keys = FIELDS + (("velocity",) if _oracle_kw(mode)["motion"] else ())
    return {k: torch.cat([getattr(p, k) for p in parts]) for k in keys}


# ---- 1. times 0, 1, 2, ...: the untimed linker, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_times_0_1_2_give_the_untimed_linker(mode):
    summ = sequence(mode, 12)
    assert summ["count"].max() <= 12
    _margins(summ, np.arange(12), mode)
    want, _ = tt.link_timed(summ, summ["node_ptr"], np.arange(12), **_oracle_kw(mode))
    m = _oracle_kw(mode)["max_gap"]
    assert all((want["matched_gap"] == k).any() for k in range(m + 1)) and (want["matched_gap"][summ["node_ptr"][1]:] < 0).any()
    timed, plain = _linker(mode), _linker(mode)
    a, b = [], []
    for lo, hi in ((0, 5), (5, 6), (6, 12)):
        a.append(timed(_upload(summ, lo, hi), times=np.arange(lo, hi, dtype=np.float64)))
        b.append(plain(_upload(summ, lo, hi)))
    torch.cuda.synchronize()
    got, ref = _cat(a, mode), _cat(b, mode)
    for k in got:
        assert torch.equal(got[k], ref[k]), (mode, k)
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), (mode, k)
    assert torch.equal(a[-1].next_id, b[-1].next_id) and int(a[-1].next_id.item()) == want["next_id"]
    assert timed._frame_times == [float(v) for v in range(12 - (m + 1), 12)] and plain._frame_times == []


# ---- 2. dropped frames, 3. jittered times -----------------------------------------------------------------------------------------------
def dropped_case(mode, jitter):
    """16 frames without frames 3, 7 and 8, the times the surviving indices (+ uniform noise of +-0.2 with `jitter`, then
    max_dt = max_gap + 1.5) -> (the sequence, its times, the keywords of max_dt, the oracle's result)."""
    full = sequence(mode, 16)
    summ, times = tt.drop_frames(full, DROPPED)
    more = {}
    if jitter:
        times = times + np.random.default_rng(100 + MODES[mode]["seed"]).uniform(-0.2, 0.2, size=len(times))
        more = dict(max_dt=_oracle_kw(mode)["max_gap"] + 1.5)
    assert len(times) == 13 and summ["count"].max() <= 12 and (np.diff(times) > 0).all()
    _margins(summ, times, mode, **more)
    kw = _oracle_kw(mode)
    want, _ = tt.link_timed(summ, summ["node_ptr"], times, **kw, **more)
    blind, _ = tt.link_timed(summ, summ["node_ptr"], np.arange(13), **kw)   # what a linker that takes the frames for consecutive makes of them
    print(mode, "matches per level:", [int((want["matched_gap"] == k).sum()) for k in range(kw["max_gap"] + 1)],
          "rows whose id differs from the untimed rule's:", int((want["cluster_track"] != blind["cluster_track"]).sum()))
    assert all((want["matched_gap"] == k).any() for k in range(kw["max_gap"] + 1))
    assert not np.array_equal(want["cluster_track"], blind["cluster_track"])   # the times change the ids
    return summ, times, more, want


@pytest.mark.parametrize("jitter", [False, True], ids=["dropped", "jittered"])
@pytest.mark.parametrize("mode", list(MODES))
def test_dropped_frames_and_jitter_follow_the_oracle(mode, jitter):
    summ, times, more, want = dropped_case(mode, jitter)
    _same_tracks(_linker(mode, **more)(_upload(summ), times=times), want, mode)


# ---- 4. by hand -----------------------------------------------------------------------------------------------------------------------
def _hole_walk(link):
    """One person walks 0.5 per period along x; the frame at time 2 is absent (times 0, 1, 3, 4); max_step = 0.2.  A track's FIRST link
    is made without a velocity, and 0.5 is outside 0.2: so the frames at times 0 and 1 are one call under max_step = 1.0, which gives the
    track its velocity (0.5, 0), and the frames at times 3 and 4 a second call under max_step = 0.2 on the carried state.
    link: a FrameLinker, called with or without times."""
    def go(timed):
        link.reset()
        link.max_step = 1.0
        a = link(_upload(_points([[(0.0, 0.0)], [(0.5, 0.0)]])), times=[0, 1] if timed else None)
        link.max_step = 0.2
        b = link(_upload(_points([[(1.5, 0.0)], [(2.0, 0.0)]])), times=[3, 4] if timed else None)
        torch.cuda.synchronize()
        return a, b
    return go


def test_a_dropped_frame_by_hand():
    from gnn_cca_amd.tracking import FrameLinker
    go = _hole_walk(FrameLinker(1.0, lam=0.0, max_gap=1, motion="velocity"))
    a, b = go(timed=False)   # the prediction 0.5 + 1 * 0.5 = 1.0 is 0.5 from 1.5: outside the gate, a second id (and then a third)
    assert a.cluster_track.tolist() == [0, 0] and b.cluster_track.tolist() == [1, 2] and not b.velocity.any()
    a, b = go(timed=True)    # dt = 2: 0.5 + 2 * 0.5 = 1.5 exactly, vel = 1.0 / 2; then dt = 1
    assert a.cluster_track.tolist() == [0, 0] and b.cluster_track.tolist() == [0, 0] and int(b.next_id.item()) == 1
    assert b.matched_gap.tolist() == [0, 0] and b.matched_prev.tolist() == [0, 0]
    assert a.velocity.tolist() == [[0.0, 0.0], [0.5, 0.0]] and b.velocity.tolist() == [[0.5, 0.0], [0.5, 0.0]]
    # max_gap = 0: max_dt = 1, and the track ends at the hole
    a, b = _hole_walk(FrameLinker(1.0, lam=0.0, max_gap=0, motion="velocity"))(timed=True)
    assert a.cluster_track.tolist() == [0, 0] and b.cluster_track.tolist() == [1, 2] and not b.velocity.any()
    # times 0, 1, 5, max_gap = 3, 0.1 per period: the link over dt = 4 exists under the default max_dt = 4 and not under 3.5
    slow = _points([[(0.0, 0.0)], [(0.1, 0.0)], [(0.5, 0.0)]])
    for kw in (dict(), dict(motion="velocity"), dict(matching="optimal")):
        t = FrameLinker(0.2, lam=0.0, max_gap=3, **kw)(_upload(slow), times=[0, 1, 5])
        u = FrameLinker(0.2, lam=0.0, max_gap=3, max_dt=3.5, **kw)(_upload(slow), times=[0, 1, 5])
        torch.cuda.synchronize()
        assert t.cluster_track.tolist() == [0, 0, 0] and t.matched_gap.tolist() == [-1, 0, 0], kw
        assert u.cluster_track.tolist() == [0, 0, 1] and u.matched_gap.tolist() == [-1, 0, -1], kw
        if kw.get("motion"):
            assert t.velocity.tolist() == [[0.0, 0.0], [0.1, 0.0], [0.4 / 4.0, 0.0]]


# ---- 5. the result does not depend on how the timed sequence is cut into calls ----------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_one_call_equals_single_frame_calls(mode):
    summ, times, more, want = dropped_case(mode, jitter=True)
    link = _linker(mode, **more)
    whole = link(_upload(summ), times=times)
    _same_tracks(whole, want, mode)
    link.reset()
    parts = [link(_upload(summ, q, q + 1), times=times[q:q + 1]) for q in range(13)]
    torch.cuda.synchronize()
    got, ref = _cat(parts, mode), _cat([whole], mode)
    for k in got:
        assert torch.equal(got[k], ref[k]), (mode, k)
    assert torch.equal(parts[-1].next_id, whole.next_id)


# ---- 6. rows beyond one wave, R = 100 ---------------------------------------------------------------------------------------------------
def wide_case():
    rng = np.random.default_rng(6)
    k, r = 70, 100
    look = rng.standard_normal((k, r)).astype(np.float32)
    vel = rng.uniform(-0.3, 0.3, size=(k, 2))
    p0 = np.stack(np.meshgrid(np.arange(10) * 1.5, np.arange(7) * 1.5), -1).reshape(k, 2) + rng.normal(0, 0.02, size=(k, 2))
    times = np.array([0.0, 0.9, 1.9])
    frames = []
    for q, t in enumerate(times):
        order = rng.permutation(k)
        at = p0[order] + t * vel[order] + rng.normal(0, 0.02, size=(k, 2))
        if q == 1:
            at[np.arange(k) % 5 == 0] += (0.0, 1000.0)   # every fifth row of frame 1 is a stranger far away; frame 2 shows everybody again
        frames.append((at, (look[order] + 0.05 * rng.standard_normal((k, r)).astype(np.float32)).astype(np.float32)))
    summ = dict(count=np.array([k] * 3, np.int32), rank=np.tile(np.arange(k), 3).astype(np.int32), pos=np.concatenate([p for p, _ in frames]),
                emb=np.concatenate([e for _, e in frames]), node_ptr=np.array([0, k, 2 * k, 3 * k], np.int64))
    kw = dict(max_step=0.5, lam=1.0, max_cos=None, max_gap=1, motion=True)
    gaps = tt.margins_timed(summ, summ["node_ptr"], times, **kw)
    print("margins (cost, d, dcos):", gaps)
    assert all(v >= MARGIN for v in gaps), gaps
    want, _ = tt.link_timed(summ, summ["node_ptr"], times, **kw)
    per_level = [int((want["matched_gap"] == q).sum()) for q in (0, 1)]
    print("matches per level:", per_level, "of", 2 * k)
    assert per_level[0] > k and per_level[1] > 0 and want["velocity"][k:].any()
    return summ, times, want


def test_three_wide_frames_on_the_motion_path():
    from gnn_cca_amd.tracking import FrameLinker
    summ, times, want = wide_case()
    t = FrameLinker(0.5, lam=1.0, max_gap=1, motion="velocity")(_upload(summ), times=times)
    _same_tracks(t, want, "motion")
    assert t.cluster_track.numel() == 210


# ---- 7. the refusals leave the state alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_refusals_leave_the_state_alone(mode):
    from gnn_cca_amd.tracking import FrameLinker
    for bad in (0, -1.0, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match="max_dt"):
            FrameLinker(1.0, max_dt=bad, **MODES[mode]["kw"])
    summ, times, more, want = dropped_case(mode, jitter=True)
    link = _linker(mode, **more)
    parts = [link(_upload(summ, 0, 6), times=times[:6])]
    kept = (link._state, list(link._frame_rows), list(link._frame_times))
    for dev in ("cpu", "cuda"):   # CPU tensors: a refusal that came after the GPU was touched would not be a ValueError
        nxt = _upload(summ, 6, 9, dev=dev)
        for bad in (times[6:8], times[6:10], [], times[6:9][::-1], [times[6], times[6], times[8]], [times[6], np.nan, times[8]],
                    [times[6], times[7], np.inf], [times[6], "7", times[8]], [times[6], 7j, times[8]], [times[6], True, times[8]],
                    times[6:9] - times[6] + times[5], times[3:6], np.stack([times[6:9]] * 2)):
            with pytest.raises(ValueError):
                link(nxt, times=bad)
        with pytest.raises(ValueError, match=r"with time stamps.*reset\(\) it first"):
            link(nxt)                     # a timed state, an untimed call
        link.max_dt = -1.0
        with pytest.raises(ValueError, match="max_dt"):
            link(nxt, times=times[6:9])
        link.max_dt = _linker(mode, **more).max_dt
        assert link._state is kept[0] and link._frame_rows == kept[1] and link._frame_times == kept[2] and link._state_timed is True
    none = link(_upload(summ, 6, 6), times=[])   # no frames: no time passes, the state stays
    assert none.cluster_track.numel() == 0 and link._state is kept[0] and link._frame_times == kept[2]
    parts.append(link(_upload(summ, 6, 13), times=times[6:]))   # ... and the linker goes on as if none of these calls had been made
    torch.cuda.synchronize()
    got = _cat(parts, mode)
    for k in got:
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), (mode, k)
    assert int(parts[-1].next_id.item()) == want["next_id"]
    # the reverse: a state written without time stamps is not continued with them; after reset() it is, ids from 0
    plain = _linker(mode)
    first = plain(_upload(summ, 0, 6))
    with pytest.raises(ValueError, match=r"reset\(\) it first"):
        plain(_upload(summ, 6, 13), times=times[6:])
    second = plain(_upload(summ, 6, 13))
    untimed, _ = tt.link_timed(summ, summ["node_ptr"], np.arange(13), **_oracle_kw(mode))
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([first.cluster_track, second.cluster_track]).cpu(), torch.from_numpy(untimed["cluster_track"]))
    plain.reset()
    plain.max_dt = link.max_dt
    _same_tracks(plain(_upload(summ), times=times), want, mode)


# ---- 8. through the pipeline ----------------------------------------------------------------------------------------------------------
def test_a_pipeline_result_links_with_times_as_its_identities_do():
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(33)
    k, cams = 14, 4
    one = dict(id_cam=rng.integers(0, cams, size=k), ids=rng.integers(0, 6, size=k), xw=rng.uniform(-10, 10, k), yw=rng.uniform(-10, 10, k),
               node=rng.standard_normal((k, 2048)).astype(np.float32), reid=rng.standard_normal((k, 256)).astype(np.float32))
    # three frames of the same detections at times 0, 1, 4: everybody 0.5 further along x per period
    times = [0.0, 1.0, 4.0]
    f = {q: np.concatenate([one[q]] * 3) for q in one}
    f["xw"][k:2 * k] += 0.5
    f["xw"][2 * k:] += 2.0
    sizes, max_dist = np.array([k, k, k]), np.array([50.0, 50.0, 50.0])
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    r = FramePipeline(m)(f["xw"], f["yw"], f["ids"], f["id_cam"], sizes, max_dist, node, reid)
    a = FrameLinker(max_step=0.6, max_gap=2, motion="velocity")(r, times=times)
    b = FrameLinker(max_step=0.6, max_gap=2, motion="velocity")(r.identities(), times=times)
    torch.cuda.synchronize()
    for q in FIELDS + ("velocity", "next_id"):
        assert torch.equal(getattr(a, q), getattr(b, q)), q
    host = {q: getattr(r.identities(), q).cpu().numpy() for q in ("count", "rank", "pos", "emb")}
    ptr = np.asarray(r.batch.node_ptr, np.int64)
    kw = dict(max_step=0.6, lam=1.0, max_cos=None, max_gap=2, motion=True)   # (blind: 0.5 + 0.5 is 1.0 from where everybody is)
    gaps = tt.margins_timed(dict(host, node_ptr=ptr), ptr, times, **kw)
    assert all(v >= MARGIN for v in gaps), gaps
    want, _ = tt.link_timed(dict(host, node_ptr=ptr), ptr, times, **kw)
    blind, _ = tt.link_timed(dict(host, node_ptr=ptr), ptr, [0, 1, 2], **kw)
    n1 = int(ptr[2])
    assert (want["matched_gap"][n1:] == 0).any() and (blind["matched_gap"][n1:] < 0).sum() > (want["matched_gap"][n1:] < 0).sum()
    _same_tracks(a, want, "motion")
