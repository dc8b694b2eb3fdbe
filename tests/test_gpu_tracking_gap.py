"""FrameLinker(max_gap=M) on the GPU against tests/tracking_gap_oracle.py: cluster_track, node_track, matched_prev, matched_gap and next_id
exactly -- over sequences with occlusions shorter and longer than M, exact ties and pairs exactly on a gate, the state carried across
batches (kept frames from the old state AND the new batch), the new entry at level 0 against the old entry, frames of 4096 clusters,
and through FramePipeline results.  Every case first asserts, on the ORACLE's numbers, that it exercises what it is about."""
import copy

import numpy as np
import pytest
import torch

import tracking_gap_oracle as tg
import tracking_oracle as to

pytestmark = pytest.mark.gpu

FIELDS = ("cluster_track", "node_track", "matched_prev", "matched_gap")


def _upload(summ, lo=0, hi=None):
    """Frames lo .. hi of an oracle sequence as a ClusterSummaries on the device."""
    from gnn_cca_amd.tracking import ClusterSummaries
    ptr = np.asarray(summ["node_ptr"], np.int64)
    hi = len(ptr) - 1 if hi is None else hi
    v0, v1 = int(ptr[lo]), int(ptr[hi])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    local = ptr[lo:hi + 1] - v0
    return ClusterSummaries(t(summ["count"][lo:hi]), t(summ["rank"][v0:v1]), t(summ["size"][v0:v1]), t(summ["n_cams"][v0:v1]),
                            t(summ["pos"][v0:v1]), t(summ["emb"][v0:v1]), local.tolist(), t(local.astype(np.int32)))


def _same_tracks(t, want):
    torch.cuda.synchronize()
    for k in FIELDS:
        got, ref = getattr(t, k).cpu(), torch.from_numpy(want[k])
        assert got.dtype == ref.dtype and torch.equal(got, ref), k
    assert t.next_id.dtype == torch.int64 and int(t.next_id.item()) == want["next_id"]


def _assert_margins(summ, max_step, lam, max_cos, m):
    """The precondition of exact equality: the kernel's float64 cosine sums differ from the oracle's in summation order only (~R * 1e-16),
    so no decision of the oracle, at any level, may hang on less than 1e-9."""
    gaps = tg.margins_gap(summ, summ["node_ptr"], max_step, lam, max_cos, m)
    print("margins (cost, d, dcos):", gaps)
    assert all(v > 1e-9 for v in gaps), gaps


# ---- 1. hide sequences ----------------------------------------------------------------------------------------------------------------
HIDE_CASES = [  # persons, arena, lam, max_cos, M, empty, seed
    (70, 12.0, 1.0, None, 1, (), 1), (70, 12.0, 0.5, 0.05, 2, (5,), 2), (70, 12.0, 0.0, None, 3, (4, 5), 3),
    (25, 8.0, 1.0, None, 2, (7,), 4), (25, 8.0, 0.0, 1.0, 1, (0,), 5)]


def hide_case(persons, arena, lam, max_cos, m, empty, seed):
    """-> (the sequence, the oracle's result) after the assertions on the oracle's numbers that make the case worth running."""
    summ = tg.hide_sequence(np.random.default_rng(seed), 12, persons, 16, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=arena, empty=empty)
    _assert_margins(summ, 1.0, lam, max_cos, m)
    want, _ = tg.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, m)
    per_level = [int((want["matched_gap"] == k).sum()) for k in range(m + 1)]
    print("matches per level:", per_level, "clusters per frame:", summ["count"].tolist())
    assert all(c > 0 for c in per_level[1:]), per_level                         # every level finds somebody
    assert (want["matched_gap"][summ["node_ptr"][1]:] < 0).any()                # somebody after frame 0 stays without a predecessor
    base, _ = tg.link_gap(summ, summ["node_ptr"], 1.0, lam, max_cos, 0)
    assert not np.array_equal(base["cluster_track"], want["cluster_track"])     # the gaps change the ids
    if persons == 70:
        assert summ["count"].max() > 64                                         # past one wave of columns
    # max_hide = M + 1 (and the empty frames): somebody comes back after MORE than M missed frames, which no level may bridge
    frame_of = np.repeat(np.arange(12), np.diff(summ["node_ptr"]))
    seen_in = {}
    for p, q in zip(summ["person"].tolist(), frame_of.tolist()):
        seen_in.setdefault(p, []).append(q)
    too_long = sum(int((np.diff(fr) > m + 1).any()) for fr in seen_in.values())
    print("persons who come back after more than M missed frames:", too_long)
    assert too_long > 0
    return summ, want


@pytest.mark.parametrize("persons,arena,lam,max_cos,m,empty,seed", HIDE_CASES)
def test_hidden_persons_keep_their_ids(persons, arena, lam, max_cos, m, empty, seed):
    from gnn_cca_amd.tracking import FrameLinker
    summ, want = hide_case(persons, arena, lam, max_cos, m, empty, seed)
    _same_tracks(FrameLinker(1.0, lam=lam, max_cos=max_cos, max_gap=m)(_upload(summ)), want)


# ---- 2. exact ties, pairs exactly on a gate -------------------------------------------------------------------------------------------
LATTICE = dict(seed=8, g=8, persons=40, arena=14.0, max_step=5.0, m=2)


def lattice_case():
    c = LATTICE
    summ = tg.hide_sequence(np.random.default_rng(c["seed"]), c["g"], c["persons"], 4, p_leave=0.1, p_enter=0.5, p_hide=0.25, max_hide=3,
                            arena=c["arena"], lattice=True)
    ties = on_gate = 0
    for k, t, d, dcos, cost, ok in tg.level_tables(summ, summ["node_ptr"], c["max_step"], 0.0, None, c["m"]):
        if k >= 1:
            on_gate += int((d == c["max_step"] * (k + 1)).sum())
        for row in np.where(ok, cost, np.inf):
            fin = np.sort(row[np.isfinite(row)])
            ties += int(len(fin) >= 2 and fin[0] == fin[1])
    print("tied rows:", ties, "pairs on a gate of level >= 1:", on_gate)
    assert ties > 0 and on_gate > 0
    want, _ = tg.link_gap(summ, summ["node_ptr"], c["max_step"], 0.0, None, c["m"])
    assert all((want["matched_gap"] == k).any() for k in range(c["m"] + 1))
    return summ, want


def test_exact_ties_and_pairs_on_a_gate_resolve_as_the_rule_says():
    from gnn_cca_amd.tracking import FrameLinker
    summ, want = lattice_case()
    _same_tracks(FrameLinker(LATTICE["max_step"], lam=0.0, max_gap=LATTICE["m"])(_upload(summ)), want)


# ---- 3. the state across batches ------------------------------------------------------------------------------------------------------
def test_the_state_carries_across_batches():
    from gnn_cca_amd.tracking import FrameLinker
    m = 2
    summ = tg.hide_sequence(np.random.default_rng(21), 12, 25, 16, noise=0.15, p_leave=0.04, p_enter=0.6, p_hide=0.12, max_hide=m + 1,
                            arena=8.0, empty=(7,))
    _assert_margins(summ, 1.0, 1.0, None, m)
    want, _ = tg.link_gap(summ, summ["node_ptr"], 1.0, 1.0, None, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    ptr = summ["node_ptr"]
    # matches that reach from a later batch into an earlier one, over a gap: the state's flags and older frames are what decides them
    cuts = ((0, 5), (5, 6), (6, 7), (7, 12))
    frame_of = np.repeat(np.arange(12), np.diff(ptr))
    reach = [int(((want["matched_gap"][ptr[lo]:ptr[hi]] >= 1) & (frame_of[ptr[lo]:ptr[hi]] - 1 - want["matched_gap"][ptr[lo]:ptr[hi]] < lo)).sum())
             for lo, hi in cuts]
    print("gap matches into an earlier batch:", reach)
    assert sum(reach) > 0
    link = FrameLinker(1.0, lam=1.0, max_gap=m)
    whole = link(_upload(summ))
    _same_tracks(whole, want)
    link.reset()
    parts = []
    for lo, hi in cuts:   # the two one-frame batches: the new state keeps frames of BOTH the old state and the batch
        parts.append(link(_upload(summ, lo, hi)))
        if hi == 6:       # an empty batch in between passes no time and changes nothing
            none = link(_upload(summ, 3, 3))
            assert none.cluster_track.numel() == 0 and none.matched_gap.numel() == 0 and torch.equal(none.next_id, parts[-1].next_id)
    torch.cuda.synchronize()
    for k in FIELDS:
        assert torch.equal(torch.cat([getattr(p, k) for p in parts]), getattr(whole, k)), k
    assert torch.equal(parts[-1].next_id, whole.next_id) and int(parts[0].next_id.item()) < int(parts[-1].next_id.item())
    # another number of appearance columns is refused until reset(); after reset() ids start at 0
    short = tg.hide_sequence(np.random.default_rng(1), 2, 5, 8)
    with pytest.raises(ValueError):
        link(_upload(short))
    link.reset()
    again = link(_upload(summ, 0, 5))
    torch.cuda.synchronize()
    assert torch.equal(again.cluster_track, parts[0].cluster_track) and int(again.cluster_track[0].item()) == 0
    assert torch.equal(again.next_id, parts[0].next_id)
    link.reset()
    _same_tracks(link(_upload(short)), tg.link_gap(short, short["node_ptr"], 1.0, 1.0, None, m)[0])


# ---- 4. the new entry at level 0 against the old entry --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [41, 42, 43])
def test_without_anybody_to_find_again_the_gap_linker_is_the_adjacent_frame_linker(seed):
    from gnn_cca_amd.tracking import FrameLinker
    summ = to.walk_sequence(np.random.default_rng(seed), 9, 70, 16, noise=0.3, p_leave=0.1, p_enter=0.6, arena=200.0)
    _assert_margins(summ, 1.0, 1.0, None, 2)
    want, _ = tg.link_gap(summ, summ["node_ptr"], 1.0, 1.0, None, 2)
    assert (want["matched_gap"] == 0).any() and not (want["matched_gap"] >= 1).any()   # sparse arena, nobody hides: levels 1 and 2 find nothing
    s = _upload(summ)
    new, old = FrameLinker(1.0, lam=1.0, max_gap=2)(s), FrameLinker(1.0, lam=1.0)(s)
    _same_tracks(new, want)
    for k in ("cluster_track", "node_track", "matched_prev", "next_id", "matched_gap"):
        assert torch.equal(getattr(new, k), getattr(old, k)), k


# ---- 5. the size limit ----------------------------------------------------------------------------------------------------------------
def test_three_frames_of_up_to_4096_clusters():
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(11)
    k = 4096
    p0 = rng.uniform(0, 150, size=(k, 2))
    stay = rng.permutation(np.flatnonzero(np.arange(k) % 3 != 0))      # frame 1 drops every third cluster of frame 0 ...
    p1 = p0[stay] + rng.normal(0, 0.2, size=(len(stay), 2))
    p2 = p0[rng.permutation(k)] + rng.normal(0, 0.2, size=(k, 2))     # ... and frame 2 shows all of them again
    counts = [k, len(stay), k]
    n = sum(counts)
    summ = dict(count=np.array(counts, np.int32), rank=np.concatenate([np.arange(c) for c in counts]).astype(np.int32),
                size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32), pos=np.concatenate([p0, p1, p2]),
                emb=np.zeros((n, 0), np.float32), node_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    want, _ = tg.link_gap(summ, summ["node_ptr"], 1.0, 0.0, None, 1)
    per_level = [int((want["matched_gap"] == q).sum()) for q in (0, 1)]
    print("matches per level:", per_level)
    assert per_level[0] > k and 0.25 * k < per_level[1] < 0.4 * k   # about the dropped third is found again over the gap
    _same_tracks(FrameLinker(1.0, lam=0.0, max_gap=1)(_upload(summ)), want)


def test_a_4097_node_frame_is_refused_before_any_launch():
    from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker
    n = 4097
    for dev in ("cpu", "cuda"):   # CPU tensors: a refusal that came after the GPU was touched would be a RuntimeError
        z32 = torch.zeros(n, dtype=torch.int32, device=dev)
        s = ClusterSummaries(torch.ones(1, dtype=torch.int32, device=dev), z32, z32, z32, torch.zeros((n, 2), dtype=torch.float64, device=dev),
                             torch.zeros((n, 0), device=dev), [0, n], torch.tensor([0, n], dtype=torch.int32, device=dev))
        with pytest.raises(ValueError):
            FrameLinker(1.0, lam=0.0, max_gap=1)(s)
    torch.cuda.synchronize()


# ---- 6. through the pipeline ----------------------------------------------------------------------------------------------------------
def test_a_blanked_frame_of_a_pipeline_result_is_bridged():
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(33)
    k, cams = 14, 4
    one = dict(id_cam=rng.integers(0, cams, size=k), ids=rng.integers(0, 6, size=k), xw=rng.uniform(-10, 10, k), yw=rng.uniform(-10, 10, k),
               node=rng.standard_normal((k, 2048)).astype(np.float32), reid=rng.standard_normal((k, 256)).astype(np.float32))
    # frame 2 shows frame 0's detections again, moved a little; the frame between them has no detections at all
    f = {q: np.concatenate([one[q], one[q]]) for q in one}
    f["xw"][k:] += rng.normal(0, 0.05, k)
    f["yw"][k:] += rng.normal(0, 0.05, k)
    sizes, max_dist = np.array([k, 0, k]), np.array([50.0, 50.0, 50.0])
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    pipe = FramePipeline(m)
    args = (f["xw"], f["yw"], f["ids"], f["id_cam"], sizes, max_dist, node, reid)
    r = pipe(*args)
    with torch.no_grad():   # put the decision boundary inside the logits so that the partition is neither trivial one
        sd = m.state_dict()
        key = [q for q in sd if q.startswith("classifier.") and q.endswith(".bias")][-1]
        sd[key] -= r.outputs["classified_edges"][-1].median()
        m.load_state_dict(sd)
    r = pipe(*args)
    s = r.identities()
    host = {q: getattr(s, q).cpu().numpy() for q in ("count", "rank", "pos", "emb")}
    ptr = np.asarray(r.batch.node_ptr, np.int64)
    assert host["count"].tolist()[1] == 0 and host["count"][0] > 0 and host["count"][2] > 0
    _assert_margins(dict(host, node_ptr=ptr), 3.0, 1.0, None, 1)
    want, _ = tg.link_gap(host, ptr, 3.0, 1.0, None, 1)
    c2 = int(host["count"][2])
    again = want["matched_gap"][k:k + c2] == 1
    assert again.any()                                                # a cluster of frame 0 reappears in frame 2 ...
    t = FrameLinker(max_step=3.0, max_gap=1)(r)
    _same_tracks(t, want)
    track, prev = t.cluster_track.cpu().numpy(), t.matched_prev.cpu().numpy()
    assert np.array_equal(track[k:k + c2][again], track[:k][prev[k:k + c2][again]])   # ... and keeps its id
    t0 = FrameLinker(max_step=3.0)(r)                                 # without max_gap every cluster of frame 2 is a stranger
    torch.cuda.synchronize()
    assert (t0.matched_prev.cpu().numpy() < 0).all() and (t0.matched_gap.cpu().numpy() == -1).all()
    assert int(t0.next_id.item()) == int(host["count"][0]) + c2 > int(t.next_id.item())
