"""KalmanLinker on the GPU against tests/tracking_kalman_oracle.py: cluster_track, node_track, matched_prev, matched_gap, next_id, velocity and
the five trajectories arrays exactly (ids and links ==, fp64 by bit pattern) -- over crossing walks with occlusions under every rule
variant, every cut of a sequence into calls, the shapes where the walk's loops change form, empty and refused frames, time stamps, the
smoother identity, the hand-written variance-gate case, the refusals, the stages downstream, and a captured call.  Every case first
asserts, on the ORACLE's numbers, that no decision hangs on less than 1e-9 and that it exercises what it is about."""
import copy
import functools

import numpy as np
import pytest
import torch

import track_score_oracle as tso
import track_smooth_oracle as ts
import tracking_kalman_oracle as tk
import tracking_motion_oracle as tm

pytestmark = pytest.mark.gpu

INTS = ("cluster_track", "node_track", "matched_prev", "matched_gap")
TRAJ = ("pos", "vel", "cov", "nis", "age")
Q, R_, VV = 0.001, 0.0025, 0.25


def _linker(kw):
    from gnn_cca_amd.kalman import KalmanLinker
    return KalmanLinker(kw["max_step"], kw["q"], kw["r"], kw["vel_var"], lam=kw["lam"], max_cos=kw["max_cos"], max_gap=kw["max_gap"],
                        max_nis=kw["max_nis"], max_dt=kw.get("max_dt"))


def _kw(max_step=0.5, lam=0.0, max_cos=None, max_gap=0, max_nis=None, q=Q, r=R_, vel_var=VV, **more):
    return dict(max_step=max_step, q=q, r=r, vel_var=vel_var, lam=lam, max_cos=max_cos, max_gap=max_gap, max_nis=max_nis, **more)


def _upload(summ, lo=0, hi=None, dev="cuda"):
    """Frames lo .. hi of an oracle sequence as a ClusterSummaries on the device."""
    from gnn_cca_amd.tracking import ClusterSummaries
    ptr = np.asarray(summ["node_ptr"], np.int64)
    hi = len(ptr) - 1 if hi is None else hi
    v0, v1 = int(ptr[lo]), int(ptr[hi])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    local = ptr[lo:hi + 1] - v0
    return ClusterSummaries(t(summ["count"][lo:hi]), t(summ["rank"][v0:v1]), t(summ["size"][v0:v1]), t(summ["n_cams"][v0:v1]),
                            t(summ["pos"][v0:v1]), t(summ["emb"][v0:v1]), local.tolist(), t(local.astype(np.int32)))


def _host(t):
    """A KalmanTracks as the oracle's dict."""
    from gnn_cca_amd.kalman import KalmanTracks
    from gnn_cca_amd.smoothing import Trajectories
    torch.cuda.synchronize()
    assert isinstance(t, KalmanTracks) and isinstance(t.trajectories, Trajectories)
    out = {k: getattr(t, k).cpu().numpy() for k in INTS + ("velocity",)}
    out.update({k: getattr(t.trajectories, k).cpu().numpy() for k in TRAJ})
    out["next_id"] = int(t.next_id.item())
    assert t.next_id.dtype == torch.int64
    return out


def _equal(got, want, rows=slice(None)):
    for k in INTS + ("velocity",) + TRAJ:
        a, b = got[k], want[k][rows]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), k


def _same(t, want):
    got = _host(t)
    _equal(got, want)
    assert got["next_id"] == want["next_id"]
    return got


def _cat(parts):
    out = {k: np.concatenate([p[k] for p in parts]) for k in INTS + ("velocity",) + TRAJ}
    out["next_id"] = parts[-1]["next_id"]
    return out


def _assert_margins(summ, kw, times=None, state=None):
    """The precondition of exact equality: the kernel's float64 cosine sums differ from the oracle's in summation order only (~R * 1e-16),
    so no decision of the oracle, in any table, may hang on less than 1e-9 (cost, d against the gate, dcos, nis against max_nis)."""
    gaps = tk.margins(summ, summ["node_ptr"], times=times, state=state, **kw)
    print("margins (cost, d, dcos, nis):", gaps)
    assert all(v > 1e-9 for v in gaps), gaps


# ---- 1. crossing walks with occlusions, every rule variant -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cross(seed=0, g=12, persons=5, r=8, p_hide=0.2, max_hide=2, arena=3.0):
    return tm.cross_sequence(np.random.default_rng(seed), g, persons, r, noise=0.05, p_hide=p_hide, max_hide=max_hide, arena=arena)


@pytest.mark.parametrize("max_nis", [None, 9.0])
@pytest.mark.parametrize("lam,max_cos", [(0.0, None), (1.0, None), (1.0, 0.5)])
@pytest.mark.parametrize("max_gap", [0, 1, 3])
def test_crossing_walks_link_as_the_rule_says(max_gap, lam, max_cos, max_nis):
    summ = cross(max_hide=max_gap + 1)
    kw = _kw(lam=lam, max_cos=max_cos, max_gap=max_gap, max_nis=max_nis)
    _assert_margins(summ, kw)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    per_level = [int((want["matched_gap"] == k).sum()) for k in range(max_gap + 1)]
    print("matches per level:", per_level, "clusters per frame:", summ["count"].tolist(), "oldest:", int(want["age"].max()))
    assert per_level[0] > 20 and (max_gap == 0 or sum(per_level[1:]) > 0) and want["age"].max() >= 5 and want["velocity"].any()
    assert (want["matched_gap"][summ["node_ptr"][1]:] < 0).any()                # somebody after frame 0 stays without a predecessor
    got = _same(_linker(kw)(_upload(summ)), want)
    if max_nis is not None:   # no link the variance gate would have refused
        linked = got["matched_gap"] >= 0
        assert linked.any() and (got["nis"][linked] <= max_nis).all()


def test_the_variance_gate_changes_links_on_a_noisy_walk():
    """Under a wide distance gate the variance gate is what decides: it must refuse pairs the distance gate admits."""
    summ = tm.cross_sequence(np.random.default_rng(2), 12, 5, 8, noise=0.12, p_hide=0.2, max_hide=2, arena=3.0)
    kw = _kw(max_step=1.5, max_gap=1, max_nis=9.0, r=0.0144)
    _assert_margins(summ, kw)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    free, _ = tk.link_kalman(summ, summ["node_ptr"], **dict(kw, max_nis=None))
    refused = sum(int(((t["d"] <= 1.5 * t["dt"]) & (t["nis"] > 9.0)).sum()) for t in tk.level_tables(summ, summ["node_ptr"], **kw))
    print("pairs inside the distance gate that the variance gate refuses:", refused)
    assert refused > 0 and not np.array_equal(free["matched_prev"], want["matched_prev"])
    got = _same(_linker(kw)(_upload(summ)), want)
    assert (got["nis"][got["matched_gap"] >= 0] <= 9.0).all()
    _same(_linker(dict(kw, max_nis=None))(_upload(summ)), free)


# ---- 2. cuts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap,max_nis", [(2, None), (2, 9.0), (8, 9.0)])
def test_the_result_does_not_depend_on_the_cut(max_gap, max_nis):
    summ = cross(seed=1, max_hide=3)
    kw = _kw(lam=1.0, max_gap=max_gap, max_nis=max_nis)
    _assert_margins(summ, kw)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    assert (want["matched_gap"] >= 1).any()
    link = _linker(kw)
    whole = _same(link(_upload(summ)), want)
    for sizes in ([1] * 12, [5, 1, 6], [3, 0, 9]):   # [1] * 12 with max_gap = 8: the first calls are shorter than the gap
        link.reset()
        edges = np.concatenate([[0], np.cumsum(sizes)])
        parts = [link(_upload(summ, int(lo), int(hi))) for lo, hi in zip(edges[:-1], edges[1:])]
        if 0 in sizes:    # the empty batch passes no time: empty outputs, the id counter as it stands
            empty = parts[sizes.index(0)]
            assert empty.cluster_track.numel() == 0 and empty.trajectories.pos.shape == (0, 2) and empty.trajectories.age.numel() == 0
            assert empty.velocity.shape == (0, 2) and torch.equal(empty.next_id, parts[sizes.index(0) - 1].next_id)
        cat = _cat([_host(p) for p in parts])
        _equal(cat, whole)
        assert cat["next_id"] == whole["next_id"]
    link.reset()     # after reset() ids start at 0 and every cluster of the first frame is a birth
    again = _host(link(_upload(summ, 6, 12)))
    alone = {k: summ[k][summ["node_ptr"][6]:] for k in ("rank", "size", "n_cams", "pos", "emb")}
    alone["count"], alone["node_ptr"] = summ["count"][6:], summ["node_ptr"][6:] - summ["node_ptr"][6]
    _equal(again, tk.link_kalman(alone, alone["node_ptr"], **kw)[0])
    assert again["cluster_track"][0] == 0 and (again["age"][:int(summ["count"][6])] == 0).all()


# ---- 3. the shapes where the walk's loops change form ------------------------------------------------------------------------------------
def crowd(rng, counts, persons, r, arena, refuse=(), noise=0.02, drift=0.15):
    """`persons` people on a jittered lattice of pitch 1 (nobody within 0.5 of anybody), everybody drifting by `drift` per frame; frame f
    shows the first counts[f] of them in a permuted order.  Frames in `refuse` get count -1 (their rows stay); a count of 0 with rows is
    given as a negative entry -n: n rows, count 0."""
    side = int(np.ceil(np.sqrt(persons)))
    home = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:persons].astype(np.float64) * (arena / side)
    home += rng.uniform(-0.1, 0.1, size=home.shape)
    heading = rng.uniform(-1, 1, size=(persons, 2))
    heading *= drift / np.linalg.norm(heading, axis=1, keepdims=True)
    look = rng.standard_normal((persons, r)).astype(np.float32)
    pos, emb, cnt, rows = [], [], [], []
    for f, c in enumerate(counts):
        n = abs(c)
        who = rng.permutation(persons)[:n]
        pos.append(home[who] + f * heading[who] + rng.normal(0, noise, size=(n, 2)))
        emb.append((look[who] + 0.05 * rng.standard_normal((n, r)).astype(np.float32)).astype(np.float32))
        cnt.append(-1 if f in refuse else max(c, 0))
        rows.append(n)
    total = sum(rows)
    node_ptr = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    rank = np.concatenate([np.arange(n) for n in rows]).astype(np.int32)
    return dict(count=np.array(cnt, np.int32), rank=rank, size=np.ones(total, np.int32), n_cams=np.ones(total, np.int32),
                pos=np.concatenate(pos).reshape(total, 2), emb=np.concatenate(emb).reshape(total, r), node_ptr=node_ptr)


@pytest.mark.parametrize("max_nis", [None, 9.0])
def test_wide_appearance_rows_more_than_one_pass_of_columns_an_empty_and_a_refused_frame(max_nis):
    """R = 260: the four-load cosine loop runs once and leaves a remainder.  70 against 130 clusters: more than one 64-column pass in
    either direction.  Frame 2 has rows but count 0, frame 3 is refused (count -1): rows zero, age -1, and frame 4 links past both."""
    summ = crowd(np.random.default_rng(7), [70, 130, -4, 9, 70], 130, 260, arena=16.0, refuse=(3,))
    kw = _kw(max_step=0.4, lam=1.0, max_cos=0.5, max_gap=3, max_nis=max_nis, r=0.0004)
    _assert_margins(summ, kw)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    ptr = summ["node_ptr"]
    per_level = [int((want["matched_gap"] == k).sum()) for k in range(4)]
    print("matches per level:", per_level)
    assert summ["count"].tolist() == [70, 130, 0, -1, 70] and per_level[0] > 30 and per_level[2] > 30 and per_level[1] == 0
    assert (want["age"][ptr[2]:ptr[4]] == -1).all() and not want["cov"][ptr[2]:ptr[4]].any() and (want["cluster_track"][ptr[2]:ptr[4]] == -1).all()
    assert want["age"][ptr[4]:].max() == 2
    _same(_linker(kw)(_upload(summ)), want)


@pytest.mark.parametrize("counts,arena", [((1100, 1030, 1100), 40.0), ((2100, 2060, 2100), 54.0)], ids=["1100", "2100"])
def test_frames_beyond_the_stride_of_the_commit_and_numbering_loops(counts, arena):
    """lam = 0: 1100 clusters against 1030, beyond the 1024 threads of the walking workgroup, then 1030 against 1100 over a gap.  And
    frames above 2048 rows: the LDS arrays have 4096 entries each, which with the variance gate's is above 64 KiB of dynamic LDS."""
    summ = crowd(np.random.default_rng(8), list(counts), counts[0], 0, arena=arena)
    kw = _kw(max_step=0.4, lam=0.0, max_gap=1, max_nis=9.0, r=0.0004)
    _assert_margins(summ, kw)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    per_level = [int((want["matched_gap"] == k).sum()) for k in range(2)]
    fresh = int((want["matched_gap"][summ["node_ptr"][1]:] < 0).sum())
    print("matches per level:", per_level, "births after frame 0:", fresh)
    assert per_level[0] > 1.8 * counts[1] and per_level[1] > 20 and fresh > 0 and want["next_id"] > counts[0]
    assert (want["matched_prev"][summ["node_ptr"][1]:] >= 1024).any()           # a partner beyond the first stride
    _same(_linker(kw)(_upload(summ)), want)


# ---- 4. time stamps ------------------------------------------------------------------------------------------------------------------------
def test_times_0_1_2_equal_the_untimed_bits_and_a_dropped_frame_is_a_gap():
    summ = cross(seed=3, max_hide=3)
    g = len(summ["count"])
    kw = _kw(lam=1.0, max_gap=2, max_nis=9.0)
    _assert_margins(summ, kw)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    untimed = _same(_linker(kw)(_upload(summ)), want)
    link = _linker(kw)
    parts = [_host(link(_upload(summ, 0, 5), times=np.arange(5.0))), _host(link(_upload(summ, 5, g), times=np.arange(5.0, g)))]
    _equal(_cat(parts), untimed)
    # frames 2 and 7 of a 14-frame recording were dropped: the times say so
    times = np.array([0, 1, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13], np.float64)
    _assert_margins(summ, kw, times=times)
    dropped, _ = tk.link_kalman(summ, summ["node_ptr"], times=times, **kw)
    assert not np.array_equal(dropped["cov"], want["cov"]) and (dropped["matched_gap"] >= 0).sum() > 20
    link = _linker(kw)
    parts = [_host(link(_upload(summ, 0, 3), times=times[:3])), _host(link(_upload(summ, 3, g), times=times[3:]))]
    _equal(_cat(parts), dropped)
    assert parts[-1]["next_id"] == dropped["next_id"]


def test_a_table_beyond_max_dt_is_skipped():
    summ = cross(seed=3, max_hide=3)
    kw = _kw(lam=1.0, max_gap=2, max_nis=None, max_dt=2.5)
    times = np.array([0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13], np.float64)   # three frame periods between frames 3 and 4: beyond max_dt
    _assert_margins(summ, kw, times=times)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], times=times, **kw)
    ptr = summ["node_ptr"]
    assert (want["matched_gap"][ptr[4]:ptr[5]] == -1).all() and (want["matched_gap"][ptr[5]:ptr[6]] <= 0).all()
    assert (tk.link_kalman(summ, summ["node_ptr"], **dict(kw, max_dt=None))[0]["matched_gap"][ptr[4]:ptr[5]] >= 0).any()
    _same(_linker(kw)(_upload(summ), times=times), want)


# ---- 5. the smoother behind the linker returns the linker's trajectories -------------------------------------------------------------------
@pytest.mark.parametrize("timed", [False, True])
def test_the_smoother_returns_exactly_the_trajectories(timed):
    from gnn_cca_amd.smoothing import TrackSmoother
    summ = cross(seed=5, max_hide=3)
    kw = _kw(lam=1.0, max_gap=2, max_nis=9.0)
    times = np.array([0, 1, 2.5, 3.5, 4, 5, 6.25, 7, 8, 9, 10.5, 11], np.float64) if timed else None
    _assert_margins(summ, kw, times=times)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], times=times, **kw)
    assert (want["matched_gap"] >= 1).any() and want["age"].max() >= 5
    link = _linker(kw)
    smooth = TrackSmoother(link, kw["q"], kw["r"], kw["vel_var"])
    got = []
    for lo, hi in ((0, 4), (4, 5), (5, 12)):
        x = _upload(summ, lo, hi)
        t = link(x, times=None if times is None else times[lo:hi])
        tr = smooth(x, t, times=None if times is None else times[lo:hi])
        torch.cuda.synchronize()
        for k in TRAJ:
            a, b = getattr(tr, k), getattr(t.trajectories, k)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (k, lo)
        got.append(_host(t))
    _equal(_cat(got), want)


# ---- 6. the hand-written variance-gate case ------------------------------------------------------------------------------------------------
def test_the_variance_gate_refuses_an_established_track_what_it_grants_a_newborn():
    s = tk.gate_case()
    want, _ = tk.link_kalman(s, s["node_ptr"], **tk.GATE)
    tk.check_gate_case(want, tk.level_tables(s, s["node_ptr"], **tk.GATE))
    got = _same(_linker(tk.GATE)(_upload(s)), want)
    tk.check_gate_case(got, tk.level_tables(s, s["node_ptr"], **tk.GATE))
    free = _host(_linker(dict(tk.GATE, max_nis=None))(_upload(s)))
    assert free["cluster_track"].tolist() == [0, 0, 0, 0, 0, 1, 0, 1]    # without the variance gate both are linked


# ---- 7. refusals: before any launch, the state does not move -----------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from gnn_cca_amd.tracking import ClusterSummaries
    summ = cross(seed=6, max_hide=2)
    kw = _kw(lam=1.0, max_gap=1, max_nis=9.0)
    _assert_margins(summ, kw)
    want, _ = tk.link_kalman(summ, summ["node_ptr"], **kw)
    link = _linker(kw)
    parts = [_host(link(_upload(summ, 0, 5)))]
    kept = (link._state, list(link._frame_rows))
    n = 4097
    narrow = dict(summ, emb=summ["emb"][:, :5])
    for dev in ("cpu", "cuda"):   # CPU tensors show that the refusal comes before the GPU is touched
        z32 = torch.zeros(n, dtype=torch.int32, device=dev)
        big = ClusterSummaries(torch.ones(1, dtype=torch.int32, device=dev), z32, z32, z32, torch.zeros((n, 2), dtype=torch.float64, device=dev),
                               torch.zeros((n, 8), device=dev), [0, n], torch.tensor([0, n], dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match="4097 detections"):
            link(big)
        with pytest.raises(ValueError, match=r"appearance columns.*reset\(\) it first"):       # another reid width
            link(_upload(narrow, 5, 8, dev=dev))
        link.motion = "velocity"                                                              # a linker of another kind
        with pytest.raises(ValueError):
            link(_upload(summ, 5, 8, dev=dev))
        link.motion = "kalman"
        link._state_motion = "velocity"                                                       # a state of another kind
        with pytest.raises(ValueError, match=r"motion='velocity'.*reset\(\) it first"):
            link(_upload(summ, 5, 8, dev=dev))
        link._state_motion = "kalman"
        with pytest.raises(ValueError, match="without time stamps"):                          # timed after untimed
            link(_upload(summ, 5, 8, dev=dev), times=[5.0, 6.0, 7.0])
        link.max_nis = float("nan")
        with pytest.raises(ValueError, match="max_nis"):
            link(_upload(summ, 5, 8, dev=dev))
        link.max_nis = 9.0
    assert link._state is kept[0] and link._frame_rows == kept[1]
    parts.append(_host(link(_upload(summ, 5, 12))))   # ... and the linker goes on as if none of these calls had been made
    _equal(_cat(parts), want)
    assert parts[-1]["next_id"] == want["next_id"]
    # the reverse: an untimed call does not continue a timed state
    link = _linker(kw)
    link(_upload(summ, 0, 5), times=np.arange(5.0))
    with pytest.raises(ValueError, match="with time stamps"):
        link(_upload(summ, 5, 12))
    with pytest.raises(ValueError, match="not after the last time"):
        link(_upload(summ, 5, 12), times=np.arange(4.0, 11.0))
    _equal(_cat([parts[0], _host(link(_upload(summ, 5, 12), times=np.arange(5.0, 12.0)))]), want)


# ---- 8. downstream: the scorer and the re-entry gallery take the linker and its tracks ---------------------------------------------------
def test_a_pipeline_result_links_and_the_stages_downstream_accept_the_tracks():
    import bench
    import reentry_oracle as ro
    from gnn_cca_amd.kalman import KalmanLinker
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.reentry import TrackGallery
    from gnn_cca_amd.tracking import TrackScorer
    rng = np.random.default_rng(33)
    k, cams = 14, 4
    one = dict(id_cam=rng.integers(0, cams, size=k), ids=rng.integers(0, 6, size=k), xw=rng.uniform(-10, 10, k), yw=rng.uniform(-10, 10, k),
               node=rng.standard_normal((k, 2048)).astype(np.float32), reid=rng.standard_normal((k, 256)).astype(np.float32))
    # three frames of the same detections, everybody 0.5 further along x in each
    f = {q: np.concatenate([one[q]] * 3) for q in one}
    f["xw"][k:2 * k] += 0.5
    f["xw"][2 * k:] += 1.0
    sizes, max_dist = np.array([k, k, k]), np.array([50.0, 50.0, 50.0])
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    r = FramePipeline(m)(f["xw"], f["yw"], f["ids"], f["id_cam"], sizes, max_dist, torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda())
    kw = _kw(max_step=0.8, lam=1.0, max_gap=1, max_nis=13.8, r=0.01)
    link = _linker(kw)
    assert isinstance(link, KalmanLinker)
    t = link(r)
    s = r.identities()
    host = {q: getattr(s, q).cpu().numpy() for q in ("count", "rank", "pos", "emb")}
    host["node_ptr"] = np.asarray(r.batch.node_ptr, np.int64)
    _assert_margins(host, kw)
    want, _ = tk.link_kalman(host, host["node_ptr"], **kw)
    assert (want["matched_gap"] == 0).any() and want["velocity"].any() and want["age"].max() == 2   # somebody is followed over all three frames
    got = _same(t, want)
    # the scorer takes the tracks and scores what its oracle scores for the same ids
    score = TrackScorer(max_ids=16, max_cams=cams)
    score.add(r, t)
    assert score.result() == tso.score(f["ids"].astype(np.int64), f["id_cam"].astype(np.int32), got["node_track"], host["node_ptr"], 16, cams)[2]
    # the gallery takes the linker and the tracks and gives what its oracle gives for the same tracks
    gal = TrackGallery(link, 0.3, window=64, max_batch=64)
    ids = gal(r, t)
    torch.cuda.synchronize()
    tr = {q: got[q] for q in INTS}
    gaps = ro.margins(host, host["node_ptr"], tr, 1, 0.3, window=64, max_batch=64)
    assert all(v > 1e-9 for v in gaps[:3]), gaps
    ident, _ = ro.gallery(host, host["node_ptr"], tr, 1, 0.3, window=64, max_batch=64)
    for q in ("cluster_identity", "node_identity", "reentered_from"):
        assert torch.equal(getattr(ids, q).cpu(), torch.from_numpy(ident[q])), q


# ---- 9. captured in a graph and replayed on new inputs -------------------------------------------------------------------------------------
def test_a_captured_call_replays_on_the_batch_in_its_input_buffers():
    """The captured call reads the state the warm-up call left (its pointers are fixed at capture), so every replay is `the call after the
    warm-up` for whatever batch stands in the input buffers."""
    kw = _kw(lam=1.0, max_gap=2, max_nis=9.0)
    # two batches of the same frame sizes: frames 4 .. 8 of a walk of five people nobody hides from, as detected and detected a little elsewhere
    walk = tm.cross_sequence(np.random.default_rng(9), 8, 5, 8, noise=0.05, p_hide=0.0, arena=3.0)
    walks = [walk, dict(walk, pos=walk["pos"] + np.random.default_rng(10).normal(0, 0.03, size=walk["pos"].shape))]
    assert walk["count"].tolist() == [5] * 8
    head = {k: walk[k][:20] for k in ("rank", "size", "n_cams", "pos", "emb")}
    head["count"], head["node_ptr"] = walk["count"][:4], walk["node_ptr"][:5]
    tails = []
    for w in walks:
        tail = {k: w[k][20:] for k in ("rank", "size", "n_cams", "pos", "emb")}
        tail["count"], tail["node_ptr"] = w["count"][4:], w["node_ptr"][4:] - 20
        tails.append(tail)
    _, state = tk.link_kalman(head, head["node_ptr"], **kw)
    wants = []
    for tail in tails:
        _assert_margins(tail, kw, state=state)
        wants.append(tk.link_kalman(tail, tail["node_ptr"], state=copy.deepcopy(state), **kw)[0])
    # the batches differ, and in both the first frame continues tracks of the carried state
    assert not np.array_equal(wants[0]["pos"], wants[1]["pos"]) and all((w["matched_gap"][:5] == 0).sum() >= 2 for w in wants)
    assert not np.array_equal(wants[0]["matched_gap"], wants[1]["matched_gap"])
    link = _linker(kw)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    x = _upload(tails[0])
    with torch.cuda.stream(stream):
        link(_upload(head))          # the warm-up call: loads the kernels, leaves the state every replay continues
        carried = (link._state, list(link._frame_rows))
        eager = link(x)
    stream.synchronize()
    _equal(_host(eager), wants[0])
    link._state, link._frame_rows = carried[0], list(carried[1])   # the same call again, from the same carried state
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            captured = link(x)
    torch.cuda.current_stream().wait_stream(stream)
    for tail, want in ((tails[0], wants[0]), (tails[1], wants[1]), (tails[0], wants[0])):
        x.pos.copy_(torch.from_numpy(tail["pos"]))
        x.emb.copy_(torch.from_numpy(tail["emb"]))
        for k in INTS:
            getattr(captured, k).fill_(7)
        for k in TRAJ:
            getattr(captured.trajectories, k).fill_(7)
        graph.replay()
        got = _host(captured)
        _equal(got, want)
        assert got["next_id"] == want["next_id"]
