"""FrameLinker(motion='velocity') on the GPU against tests/tracking_motion_oracle.py: cluster_track, node_track, matched_prev, matched_gap,
next_id AND velocity exactly (a velocity is one subtraction and one division, no sums) -- over people crossing each other with and
without occlusions, the hand-made crossing, the state carried across batches, frames of 4096 clusters, exact ties and pairs exactly
on a gate, empty and refused frames, FramePipeline results, the refusals, and a non-default stream.  Every case first asserts, on the
ORACLE's numbers, that it exercises what it is about."""
import copy

import numpy as np
import pytest
import torch

import tracking_gap_oracle as tg
import tracking_motion_oracle as tm

pytestmark = pytest.mark.gpu

FIELDS = ("cluster_track", "node_track", "matched_prev", "matched_gap")


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


def _same_tracks(t, want):
    torch.cuda.synchronize()
    for k in FIELDS + ("velocity",):
        got, ref = getattr(t, k).cpu(), torch.from_numpy(want[k])
        assert got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got, ref), k
    assert t.next_id.dtype == torch.int64 and int(t.next_id.item()) == want["next_id"]


def _assert_margins(summ, max_step, lam, max_cos, m):
    """The precondition of exact equality: the kernel's float64 cosine sums differ from the oracle's in summation order only (~R * 1e-16),
    so no decision of the oracle, in any table, may hang on less than 1e-9."""
    gaps = tm.margins_motion(summ, summ["node_ptr"], max_step, lam, max_cos, m)
    print("margins (cost, d, dcos):", gaps)
    assert all(v > 1e-9 for v in gaps), gaps


def _points(frames, emb_dim=0):
    """frames: per frame a list of (x, y) -> the summaries of one-node clusters."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([p for f in frames for p in f], np.float64).reshape(n, 2)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32), pos=pos,
                emb=np.zeros((n, emb_dim), np.float32), node_ptr=node_ptr)


# ---- 1. people crossing each other ----------------------------------------------------------------------------------------------------
CROSS_CASES = [  # persons, arena, lam, max_cos, M, max_step, p_hide, seed
    (70, 6.0, 0.0, None, 0, 1.0, 0.0, 0), (70, 6.0, 1.0, None, 2, 0.4, 0.12, 1), (70, 6.0, 0.5, 0.05, 1, 0.4, 0.12, 2),
    (25, 6.0, 0.0, None, 2, 1.0, 0.12, 0), (25, 6.0, 1.0, None, 0, 0.4, 0.0, 1)]


def cross_case(persons, arena, lam, max_cos, m, max_step, p_hide, seed):
    """-> (the sequence, the oracle's result) after the assertions on the oracle's numbers that make the case worth running."""
    summ = tm.cross_sequence(np.random.default_rng(seed), 12, persons, 16, speed=(0.3, 0.6), noise=0.05, p_hide=p_hide, max_hide=m + 1, arena=arena)
    _assert_margins(summ, max_step, lam, max_cos, m)
    want, _ = tm.link_motion(summ, summ["node_ptr"], max_step, lam, max_cos, m)
    base, _ = tm.link_motion(summ, summ["node_ptr"], max_step, lam, max_cos, m, motion=False)
    per_level = [int((want["matched_gap"] == k).sum()) for k in range(m + 1)]
    sw = [tm.switches(summ["person"], r["cluster_track"], summ["node_ptr"]) for r in (base, want)]
    print("matches per level:", per_level, "clusters per frame:", summ["count"].tolist(), "switches without / with motion:", sw)
    assert all(c > 0 for c in per_level), per_level                             # every level finds somebody
    assert (want["matched_gap"][summ["node_ptr"][1]:] < 0).any()                # somebody after frame 0 stays without a predecessor
    assert not np.array_equal(base["cluster_track"], want["cluster_track"])     # the prediction changes the ids
    assert want["velocity"].any()
    if persons == 70:
        assert summ["count"].max() > 64                                         # past one wave of columns
    if lam == 0.0 or max_step == 0.4:   # (not claimed where appearance already decides under a wide gate)
        assert sw[1] < sw[0], sw
    return summ, want


@pytest.mark.parametrize("persons,arena,lam,max_cos,m,max_step,p_hide,seed", CROSS_CASES)
def test_people_crossing_each_other_keep_their_ids(persons, arena, lam, max_cos, m, max_step, p_hide, seed):
    from gnn_cca_amd.tracking import FrameLinker
    summ, want = cross_case(persons, arena, lam, max_cos, m, max_step, p_hide, seed)
    _same_tracks(FrameLinker(max_step, lam=lam, max_cos=max_cos, max_gap=m, motion="velocity")(_upload(summ)), want)


# ---- 2. the hand-made crossing --------------------------------------------------------------------------------------------------------
def test_two_people_crossing_by_hand():
    from gnn_cca_amd.tracking import FrameLinker
    s = _points([[(float(t), 0.0), (5.0 - t, 0.25)] for t in range(6)])
    want, _ = tm.link_motion(s, s["node_ptr"], 1.5, 0.0, None, 0)
    assert want["cluster_track"].tolist() == [0, 1] * 6 and want["velocity"].tolist() == [[0.0, 0.0]] * 2 + [[1.0, 0.0], [-1.0, 0.0]] * 5
    t = FrameLinker(1.5, lam=0.0, motion="velocity")(_upload(s))
    _same_tracks(t, want)
    none = FrameLinker(1.5, lam=0.0)(_upload(s))   # without motion the two swap ids where they pass each other
    torch.cuda.synchronize()
    assert none.cluster_track.tolist() == [0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0] and none.velocity is None


# ---- 3. the state across batches ------------------------------------------------------------------------------------------------------
def test_the_state_carries_across_batches():
    from gnn_cca_amd.tracking import FrameLinker
    m = 2
    summ = tm.cross_sequence(np.random.default_rng(21), 12, 25, 16, p_hide=0.12, max_hide=m + 1, arena=6.0)
    _assert_margins(summ, 0.4, 1.0, None, m)
    want, _ = tm.link_motion(summ, summ["node_ptr"], 0.4, 1.0, None, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    ptr = summ["node_ptr"]
    # (5, 6): a one-frame batch, G < M + 1 -- two frames of the old state stay in the new one, velocities and flags included
    cuts = ((0, 5), (5, 6), (6, 12))
    frame_of = np.repeat(np.arange(12), np.diff(ptr))
    reach = [int(((want["matched_gap"][ptr[lo]:ptr[hi]] >= 1) & (frame_of[ptr[lo]:ptr[hi]] - 1 - want["matched_gap"][ptr[lo]:ptr[hi]] < lo)).sum())
             for lo, hi in cuts]
    moving = [int(np.abs(want["velocity"][ptr[lo - 1]:ptr[lo]]).sum(axis=1).astype(bool).sum()) for lo, _ in cuts[1:]]
    print("gap matches into an earlier batch:", reach, "moving clusters in the last frame before a cut:", moving)
    assert reach[1] > 0 and reach[2] > 0 and all(v > 0 for v in moving)
    link = FrameLinker(0.4, lam=1.0, max_gap=m, motion="velocity")
    whole = link(_upload(summ))
    _same_tracks(whole, want)
    link.reset()
    parts = []
    for lo, hi in cuts:
        parts.append(link(_upload(summ, lo, hi)))
        if hi == 6:       # an empty batch in between passes no time and changes nothing
            none = link(_upload(summ, 3, 3))
            assert none.cluster_track.numel() == 0 and none.matched_gap.numel() == 0 and torch.equal(none.next_id, parts[-1].next_id)
            assert none.velocity.shape == (0, 2) and none.velocity.dtype == torch.float64
    torch.cuda.synchronize()
    for k in FIELDS + ("velocity",):
        assert torch.equal(torch.cat([getattr(p, k) for p in parts]), getattr(whole, k)), k
    assert torch.equal(parts[-1].next_id, whole.next_id) and int(parts[0].next_id.item()) < int(parts[-1].next_id.item())
    # after reset() ids start at 0 and nobody has a velocity
    link.reset()
    again = link(_upload(summ, 6, 12))
    alone = tg.frames_of(summ, 6, 12)
    _same_tracks(again, tm.link_motion(alone, alone["node_ptr"], 0.4, 1.0, None, m)[0])
    assert int(again.cluster_track[0].item()) == 0 and not again.velocity[:int(summ["count"][6])].any()


# ---- 4. the size limit ----------------------------------------------------------------------------------------------------------------
def test_three_frames_of_4096_clusters_on_a_drifting_lattice():
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(11)
    k, drift = 4096, np.array([0.3, 0.2])
    p0 = np.stack(np.meshgrid(np.arange(64) * 2.0, np.arange(64) * 2.0), -1).reshape(k, 2) + rng.normal(0, 0.02, size=(k, 2))
    order1, order2 = rng.permutation(k), rng.permutation(k)
    p1 = p0[order1] + drift + rng.normal(0, 0.02, size=(k, 2))
    p1[np.arange(k) % 3 == 0] += (0.0, 1000.0)                         # every third row of frame 1 is a stranger far away ...
    p2 = p0[order2] + 2 * drift + rng.normal(0, 0.02, size=(k, 2))     # ... and frame 2 shows everybody again
    n = 3 * k
    summ = dict(count=np.array([k] * 3, np.int32), rank=np.tile(np.arange(k), 3).astype(np.int32), size=np.ones(n, np.int32),
                n_cams=np.ones(n, np.int32), pos=np.concatenate([p0, p1, p2]), emb=np.zeros((n, 0), np.float32),
                node_ptr=np.array([0, k, 2 * k, 3 * k], np.int64))
    want, _ = tm.link_motion(summ, summ["node_ptr"], 0.5, 0.0, None, 1)
    per_level = [int((want["matched_gap"] == q).sum()) for q in (0, 1)]
    print("matches per level:", per_level)
    assert per_level[0] > k and 0.25 * k < per_level[1] < 0.4 * k      # about the third that frame 1 missed is found again over the gap
    assert np.abs(want["velocity"][2 * k:] - drift).max() < 0.2 and want["velocity"][2 * k:].all()
    _same_tracks(FrameLinker(0.5, lam=0.0, max_gap=1, motion="velocity")(_upload(summ)), want)


def test_a_4097_node_frame_is_refused_before_any_launch():
    from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker
    n = 4097
    for dev in ("cpu", "cuda"):   # CPU tensors: a refusal that came after the GPU was touched would be a RuntimeError
        z32 = torch.zeros(n, dtype=torch.int32, device=dev)
        s = ClusterSummaries(torch.ones(1, dtype=torch.int32, device=dev), z32, z32, z32, torch.zeros((n, 2), dtype=torch.float64, device=dev),
                             torch.zeros((n, 0), device=dev), [0, n], torch.tensor([0, n], dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match="4097 detections"):
            FrameLinker(1.0, lam=0.0, max_gap=1, motion="velocity")(s)
    torch.cuda.synchronize()


# ---- 5. exact ties, pairs exactly on a gate -------------------------------------------------------------------------------------------
LATTICE = dict(seed=3, g=8, persons=40, arena=12, max_step=2.0, m=2)


def lattice_walk(rng, g, persons, arena, p_hide, max_hide):
    """Integer start points, integer velocities in {-1, 0, 1}^2, no noise: exact distances, exact ties, integer velocities wherever a
    person is linked to itself.  Occlusions as in cross_sequence."""
    start = rng.integers(0, arena, size=(persons, 2)).astype(np.float64)
    step = rng.integers(-1, 2, size=(persons, 2)).astype(np.float64)
    hidden, seen_before = np.zeros(persons, np.int64), np.zeros(persons, bool)
    frames = []
    for q in range(g):
        rows = []
        for p in rng.permutation(persons):
            if seen_before[p] and hidden[p] == 0 and rng.random() < p_hide:
                hidden[p] = int(rng.integers(1, max_hide + 1))
            if hidden[p] > 0:
                hidden[p] -= 1
                continue
            rows.append(tuple(start[p] + q * step[p]))
            seen_before[p] = True
        frames.append(rows)
    return _points(frames, emb_dim=4)


def lattice_case():
    c = LATTICE
    summ = lattice_walk(np.random.default_rng(c["seed"]), c["g"], c["persons"], c["arena"], 0.25, 3)
    ties, on_gate = [0, 0], 0   # tied rows at level 0 / at a level >= 1
    for k, t, d, dcos, cost, ok in tm.level_tables(summ, summ["node_ptr"], c["max_step"], 0.0, None, c["m"]):
        if k >= 1:
            on_gate += int((d == c["max_step"] * (k + 1)).sum())
        for row in np.where(ok, cost, np.inf):
            fin = np.sort(row[np.isfinite(row)])
            ties[min(k, 1)] += int(len(fin) >= 2 and fin[0] == fin[1])
    want, _ = tm.link_motion(summ, summ["node_ptr"], c["max_step"], 0.0, None, c["m"])
    whole = (want["velocity"] == np.round(want["velocity"])).all(axis=1) & want["velocity"].any(axis=1)
    print("tied rows at level 0 / above:", ties, "pairs on a gate of level >= 1:", on_gate, "rows with a non-zero integer velocity:", int(whole.sum()))
    assert ties[0] > 0 and ties[1] > 0 and on_gate > 0 and whole.sum() > 20
    assert all((want["matched_gap"] == k).any() for k in range(c["m"] + 1))
    return summ, want


def test_exact_ties_and_pairs_on_a_gate_resolve_as_the_rule_says():
    from gnn_cca_amd.tracking import FrameLinker
    summ, want = lattice_case()
    _same_tracks(FrameLinker(LATTICE["max_step"], lam=0.0, max_gap=LATTICE["m"], motion="velocity")(_upload(summ)), want)


# ---- 6. an empty frame and a refused frame in the middle ------------------------------------------------------------------------------
def test_time_passes_in_an_empty_and_in_a_refused_frame():
    from gnn_cca_amd.tracking import FrameLinker
    # two people, one step per frame along x and along y; frame 2 shows nobody: frame 3 finds both at pos + 2 * vel over the gap
    s = _points([[(0.0, 0.0), (5.0, 0.0)], [(1.0, 0.0), (5.0, 1.0)], [], [(3.0, 0.0), (5.0, 3.0)], [(4.0, 0.0), (5.0, 4.0)]])
    want, _ = tm.link_motion(s, s["node_ptr"], 1.0, 0.0, None, 1)
    assert want["cluster_track"].tolist() == [0, 1] * 4 and want["matched_gap"].tolist() == [-1, -1, 0, 0, 1, 1, 0, 0]
    assert want["velocity"].tolist() == [[0.0, 0.0]] * 2 + [[1.0, 0.0], [0.0, 1.0]] * 3
    _same_tracks(FrameLinker(1.0, lam=0.0, max_gap=1, motion="velocity")(_upload(s)), want)
    # without max_gap nobody looks past the empty frame: the two start again in frame 3, without a velocity
    want0, _ = tm.link_motion(s, s["node_ptr"], 1.0, 0.0, None, 0)
    assert want0["cluster_track"].tolist() == [0, 1, 0, 1, 2, 3, 2, 3] and not want0["velocity"][4:6].any() and want0["velocity"][6:].any()
    _same_tracks(FrameLinker(1.0, lam=0.0, motion="velocity")(_upload(s)), want0)
    # a refused frame (count -1) with rows of its own: nothing links to them, its detections get track -1, time passes
    r = _points([[(0.0, 0.0), (5.0, 0.0)], [(1.0, 0.0), (5.0, 1.0)], [(2.0, 0.0), (5.0, 2.0), (9.0, 9.0)], [(3.0, 0.0), (5.0, 3.0)]])
    r["count"][2] = -1
    want, _ = tm.link_motion(r, r["node_ptr"], 1.0, 0.0, None, 1)
    assert want["cluster_track"].tolist() == [0, 1, 0, 1, -1, -1, -1, 0, 1] and want["node_track"].tolist() == want["cluster_track"].tolist()
    assert want["matched_gap"].tolist() == [-1, -1, 0, 0, -1, -1, -1, 1, 1] and not want["velocity"][4:7].any()
    _same_tracks(FrameLinker(1.0, lam=0.0, max_gap=1, motion="velocity")(_upload(r)), want)


# ---- 7. through the pipeline ----------------------------------------------------------------------------------------------------------
def test_a_pipeline_result_links_as_its_identities_do():
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.tracking import FrameLinker
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
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    r = FramePipeline(m)(f["xw"], f["yw"], f["ids"], f["id_cam"], sizes, max_dist, node, reid)
    a = FrameLinker(max_step=0.6, max_gap=1, motion="velocity")(r)
    b = FrameLinker(max_step=0.6, max_gap=1, motion="velocity")(r.identities())
    torch.cuda.synchronize()
    for q in FIELDS + ("velocity", "next_id"):
        assert torch.equal(getattr(a, q), getattr(b, q)), q
    assert a.velocity.dtype == torch.float64 and a.velocity.shape == (3 * k, 2)
    host = {q: getattr(r.identities(), q).cpu().numpy() for q in ("count", "rank", "pos", "emb")}
    ptr = np.asarray(r.batch.node_ptr, np.int64)
    _assert_margins(dict(host, node_ptr=ptr), 0.6, 1.0, None, 1)
    want, _ = tm.link_motion(host, ptr, 0.6, 1.0, None, 1)
    assert (want["matched_gap"] == 0).any() and want["velocity"].any()   # somebody is followed, and moves
    _same_tracks(a, want)


# ---- 8. refusals: before any launch, the state does not move --------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker
    for kw in (dict(motion="kalman"), dict(motion=None), dict(motion=1), dict(motion="velocity", matching="optimal")):
        with pytest.raises(ValueError):
            FrameLinker(1.0, **kw)
    s = _points([[(0.0, 0.0), (5.0, 0.0)], [(1.0, 0.0), (5.0, 1.0)], [(2.0, 0.0), (5.0, 2.0)], [(3.0, 0.0), (5.0, 3.0)]])
    want, _ = tm.link_motion(s, s["node_ptr"], 1.0, 0.0, None, 1)
    assert want["cluster_track"].tolist() == [0, 1] * 4
    link = FrameLinker(1.0, lam=0.0, max_gap=1, motion="velocity")
    parts = [link(_upload(s, 0, 2))]
    n = 4097
    for dev in ("cpu", "cuda"):   # a frame above the limit, a state of another kind, a combination there is no kernel for: CPU tensors
        z32 = torch.zeros(n, dtype=torch.int32, device=dev)   # show that the refusal comes before the GPU is touched
        big = ClusterSummaries(torch.ones(1, dtype=torch.int32, device=dev), z32, z32, z32, torch.zeros((n, 2), dtype=torch.float64, device=dev),
                               torch.zeros((n, 0), device=dev), [0, n], torch.tensor([0, n], dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match="4097 detections"):
            link(big)
        link.motion = "none"
        with pytest.raises(ValueError, match=r"motion='velocity'.*reset\(\) it first"):
            link(_upload(s, 2, 3, dev=dev))
        link.motion, link.matching = "velocity", "optimal"
        with pytest.raises(ValueError):
            link(_upload(s, 2, 3, dev=dev))
        link.matching = "mutual"
    parts.append(link(_upload(s, 2, 4)))   # ... and the linker goes on as if none of these calls had been made
    torch.cuda.synchronize()
    for k in FIELDS + ("velocity",):
        assert torch.equal(torch.cat([getattr(p, k) for p in parts]).cpu(), torch.from_numpy(want[k])), k
    assert int(parts[-1].next_id.item()) == want["next_id"] == 2
    # the other way round: a state written without motion is refused by a linker with motion, for both of the older state kinds
    for gap in (0, 1):
        link = FrameLinker(1.0, lam=0.0, max_gap=gap)
        t0 = link(_upload(s, 0, 2))
        link.motion = "velocity"
        with pytest.raises(ValueError, match=r"motion='none'.*reset\(\) it first"):
            link(_upload(s, 2, 4))
        link.motion = "none"
        t1 = link(_upload(s, 2, 4))
        ref, _ = tg.link_gap(s, s["node_ptr"], 1.0, 0.0, None, gap)
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([t0.cluster_track, t1.cluster_track]).cpu(), torch.from_numpy(ref["cluster_track"])) and t1.velocity is None
        link.motion = "velocity"
        link.reset()   # mixing needs reset(): after it the same linker links with motion, ids from 0
        _same_tracks(link(_upload(s)), tm.link_motion(s, s["node_ptr"], 1.0, 0.0, None, gap)[0])


# ---- 9. a non-default stream ----------------------------------------------------------------------------------------------------------
def test_two_calls_on_a_side_stream():
    from gnn_cca_amd.tracking import FrameLinker
    m = 1
    summ = tm.cross_sequence(np.random.default_rng(5), 12, 25, 16, p_hide=0.12, max_hide=m + 1, arena=6.0)
    _assert_margins(summ, 0.4, 1.0, None, m)
    want, _ = tm.link_motion(summ, summ["node_ptr"], 0.4, 1.0, None, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    link = FrameLinker(0.4, lam=1.0, max_gap=m, motion="velocity")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the first call's state and workspace are allocated on this stream and read by the second call on it
        first = link(_upload(summ, 0, 7))
        second = link(_upload(summ, 7, 12))
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for k in FIELDS + ("velocity",):
        assert torch.equal(torch.cat([getattr(first, k), getattr(second, k)]).cpu(), torch.from_numpy(want[k])), k
    assert int(second.next_id.item()) == want["next_id"]
