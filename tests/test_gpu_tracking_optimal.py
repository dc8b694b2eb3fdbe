"""FrameLinker(matching='optimal') on the GPU against tests/tracking_assign_oracle.py: cluster_track, node_track, matched_prev, matched_gap
and next_id exactly -- the hand-written case where the two rules differ, crowded sequences (a 102-cluster frame: more than one pass of 64
columns), sparse ones with appearance, exact ties on a lattice, the state carried across batches, the edges of the shape (128 clusters
against 1, empty tables, a refused frame, NaN), miss_cost, and the refusals, which come before any launch and leave the state alone.
Every case first asserts, on the ORACLE's numbers, that it exercises what it is about.

Where the rule reads embeddings, the kernel's float64 cosine sums differ from the oracle's in summation order only (~R * 1e-16).  A gate
decision is asserted not to hang on less than 1e-9; the assignment itself would change only if two different sets of pairs had totals
within that distance, which continuous random data does not produce (the lattice case, with exact ties, reads no embeddings)."""
import numpy as np
import pytest
import torch

import track_score_oracle as ts
import tracking_assign_oracle as ta
import tracking_gap_oracle as tg

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
    ones = np.ones(v1 - v0, np.int32)
    return ClusterSummaries(t(summ["count"][lo:hi]), t(summ["rank"][v0:v1]), t(ones), t(ones), t(summ["pos"][v0:v1]), t(summ["emb"][v0:v1]),
                            local.tolist(), t(local.astype(np.int32)))


def _same_tracks(t, want):
    torch.cuda.synchronize()
    for k in FIELDS:
        got, ref = getattr(t, k).cpu(), torch.from_numpy(want[k])
        assert got.dtype == ref.dtype and torch.equal(got, ref), k
    assert t.next_id.dtype == torch.int64 and int(t.next_id.item()) == want["next_id"]


def _seq(frames, emb=None):
    """frames: per frame a list of (x, y) -> the summaries of one-node clusters; emb: float32 [N, R] or None (R = 0)."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([p for f in frames for p in f], np.float64).reshape(n, 2)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, pos=pos, emb=np.zeros((n, 0), np.float32) if emb is None else np.asarray(emb, np.float32),
                node_ptr=node_ptr)


def _gate_margins(summ, max_step, lam, max_cos, m):
    """The smallest |d - gate_k| and |dcos - max_cos| over every table the optimal rule looks at."""
    gd = gc = np.inf
    for k, t, d, dcos, cost, ok in ta.level_tables(summ, summ["node_ptr"], max_step, lam, max_cos, m):
        gd = min(gd, float(np.abs(d - np.float64(max_step) * np.float64(k + 1)).min()))
        if max_cos is not None:
            gc = min(gc, float(np.abs(dcos - max_cos).min()))
    return gd, gc


def _optimal(summ, max_step, lam=1.0, max_cos=None, m=0, miss_cost=None):
    from gnn_cca_amd.tracking import FrameLinker
    want, _ = ta.link_gap(summ, summ["node_ptr"], max_step, lam, max_cos, m, matching="optimal", miss_cost=miss_cost)
    got = FrameLinker(max_step, lam=lam, max_cos=max_cos, max_gap=m, matching="optimal", miss_cost=miss_cost)(_upload(summ))
    _same_tracks(got, want)
    return got, want


# ---- 1. the hand-written case where the two rules differ -------------------------------------------------------------------------------
def test_two_by_two_where_the_rules_differ():
    from gnn_cca_amd.tracking import FrameLinker
    #            b0          b1             a0          a1
    s = _seq([[(0.0, 0.0), (0.7, 0.0)], [(0.3, 0.0), (-0.6, 0.0)]])
    mutual = FrameLinker(0.8, lam=0.0)(_upload(s))
    gap = FrameLinker(0.8, lam=0.0, max_gap=1)(_upload(s))
    opt = FrameLinker(0.8, lam=0.0, matching="optimal")(_upload(s))
    torch.cuda.synchronize()
    for t in (mutual, gap):   # a0 - b0 are each other's best; a1's only admissible partner is taken: a new id.  Untouched by this mode.
        assert t.matched_prev.tolist() == [-1, -1, 0, -1] and t.cluster_track.tolist() == [0, 1, 0, 2] and int(t.next_id.item()) == 3
        assert t.matched_gap.tolist() == [-1, -1, 0, -1]
    # (0.5 - 1) + (0.75 - 1) for a0 - b1 with a1 - b0 is less than 0.375 - 1 for a0 - b0 alone
    assert opt.matched_prev.tolist() == [-1, -1, 1, 0] and opt.cluster_track.tolist() == [0, 1, 1, 0] and int(opt.next_id.item()) == 2
    assert opt.matched_gap.tolist() == [-1, -1, 0, 0] and opt.node_track.tolist() == [0, 1, 1, 0]
    _same_tracks(opt, ta.link_gap(s, s["node_ptr"], 0.8, 0.0, matching="optimal")[0])
    _same_tracks(gap, ta.link_gap(s, s["node_ptr"], 0.8, 0.0, max_gap=1, matching="mutual")[0])


# ---- 2. sequences ---------------------------------------------------------------------------------------------------------------------
CROWDED = [  # seed, persons, arena, M -> the oracle's IDSW, IDF1 (3 places), tracks for mutual best and for the optimal assignment
    (1, 70, 8.0, 1, (80, 0.652, 81), (54, 0.752, 64)), (4, 70, 8.0, 2, (75, 0.618, 76), (55, 0.699, 66)),
    (7, 40, 6.0, 0, (46, 0.649, 64), (33, 0.681, 46)), (7, 120, 10.0, 1, (141, 0.626, 153), (94, 0.698, 119))]


def _scores(summ, node_track):
    n = len(summ["rank"])
    r = ts.score(summ["person"], np.zeros(n, np.int32), node_track, summ["node_ptr"], 4096, 1)[2]
    return r["IDSW"], round(r["IDF1"], 3), r["tracks"]


@pytest.mark.parametrize("seed,persons,arena,m,mutual_scores,optimal_scores", CROWDED)
def test_crowded_sequences(seed, persons, arena, m, mutual_scores, optimal_scores):
    summ = tg.hide_sequence(np.random.default_rng(seed), 12, persons, 8, arena=arena, max_hide=max(m, 1), noise=0.3, max_alive=max(70, persons))
    print("clusters per frame:", summ["count"].tolist())
    assert 35 <= summ["count"].max() <= 102 and (persons < 120 or summ["count"].max() > 64)
    base, _ = ta.link_gap(summ, summ["node_ptr"], 0.8, 0.0, None, m, matching="mutual")
    got, want = _optimal(summ, 0.8, 0.0, None, m)
    assert not np.array_equal(base["cluster_track"], want["cluster_track"])
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    # the scores of the device's ids, by the scoring ORACLE: what the rule is worth on this sequence
    assert _scores(summ, base["node_track"]) == mutual_scores
    assert _scores(summ, got.node_track.cpu().numpy()) == optimal_scores


@pytest.mark.parametrize("seed,m,lam,max_cos", [(1, 1, 1.0, None), (4, 2, 1.0, 0.5)])
def test_sparse_sequences_with_appearance(seed, m, lam, max_cos):
    summ = tg.hide_sequence(np.random.default_rng(seed), 12, 70, 8, arena=20.0, max_hide=max(m, 1), noise=0.3, max_alive=70)
    margins = _gate_margins(summ, 0.8, lam, max_cos, m)
    print("smallest |d - gate|, |dcos - max_cos|:", margins)
    assert all(v > 1e-9 for v in margins), margins
    got, want = _optimal(summ, 0.8, lam, max_cos, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    if max_cos is None:   # row 1 of the design's table: even here the two rules differ
        base, _ = ta.link_gap(summ, summ["node_ptr"], 0.8, lam, max_cos, m, matching="mutual")
        assert _scores(summ, base["node_track"]) == (8, 0.907, 65) and _scores(summ, got.node_track.cpu().numpy()) == (7, 0.925, 64)


def test_exact_ties_and_pairs_on_a_gate():
    max_step, m = 5.0, 2
    summ = tg.hide_sequence(np.random.default_rng(8), 8, 40, 4, p_leave=0.1, p_enter=0.5, p_hide=0.25, max_hide=3, arena=14.0, lattice=True)
    ties = on_gate = 0
    for k, t, d, dcos, cost, ok in ta.level_tables(summ, summ["node_ptr"], max_step, 0.0, None, m):
        on_gate += int((d == max_step * (k + 1)).sum())
        for table in (np.where(ok, cost, np.inf), np.where(ok, cost, np.inf).T):
            for row in table:
                fin = np.sort(row[np.isfinite(row)])
                ties += int(len(fin) >= 2 and fin[0] == fin[1])
    print("rows and columns whose two cheapest pairs tie:", ties, "pairs exactly on a gate:", on_gate)
    assert ties > 0 and on_gate > 0
    _, want = _optimal(summ, max_step, 0.0, None, m)
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))


# ---- 3. the state across batches ------------------------------------------------------------------------------------------------------
def test_the_state_carries_across_batches():
    from gnn_cca_amd.tracking import FrameLinker
    m = 2
    summ = tg.hide_sequence(np.random.default_rng(4), 12, 70, 8, arena=8.0, max_hide=m, noise=0.3, max_alive=70)
    want, _ = ta.link_gap(summ, summ["node_ptr"], 0.8, 0.0, None, m, matching="optimal")
    assert all((want["matched_gap"] == k).any() for k in range(m + 1))
    link = FrameLinker(0.8, lam=0.0, max_gap=m, matching="optimal")
    whole = link(_upload(summ))
    _same_tracks(whole, want)
    link.reset()
    parts = []
    for lo, hi in ((0, 5), (5, 6), (6, 6), (6, 7), (7, 12)):
        t = link(_upload(summ, lo, hi))
        if lo == hi:   # an empty call passes no time and changes nothing
            assert t.cluster_track.numel() == 0 and t.matched_gap.numel() == 0 and torch.equal(t.next_id, parts[-1].next_id)
        else:
            parts.append(t)
    torch.cuda.synchronize()
    for k in FIELDS:
        assert torch.equal(torch.cat([getattr(p, k) for p in parts]), getattr(whole, k)), k
    assert torch.equal(parts[-1].next_id, whole.next_id) and int(parts[0].next_id.item()) < int(parts[-1].next_id.item())
    link.reset()
    again = link(_upload(summ, 0, 5))
    torch.cuda.synchronize()
    assert torch.equal(again.cluster_track, parts[0].cluster_track) and int(again.cluster_track[0].item()) == 0


# ---- 4. the edges of the shape --------------------------------------------------------------------------------------------------------
def test_128_clusters_next_to_one():
    rng = np.random.default_rng(12)
    p0 = rng.uniform(0, 6, size=(128, 2))
    p2 = p0[rng.permutation(128)] + rng.normal(0, 0.3, size=(128, 2))
    s = _seq([[tuple(p) for p in p0], [tuple(p0[5] + 0.1)], [tuple(p) for p in p2]])
    tables = [(k, t, ok.shape, int(ok.sum())) for k, t, d, dcos, cost, ok in ta.level_tables(s, s["node_ptr"], 0.8, 0.0, None, 1)]
    print("tables (level, frame, shape, admissible pairs):", tables)
    # m > n (1 x 128), n > m (128 x 1), and at level 1 the full table of the limit: 127 free columns, crowded
    assert [q[2] for q in tables] == [(1, 128), (128, 1), (127, 127)] and tables[2][3] > 4 * 127
    _, want = _optimal(s, 0.8, 0.0, None, 1)
    assert (want["matched_gap"] == 1).sum() > 100
    assert not np.array_equal(want["matched_prev"], ta.link_gap(s, s["node_ptr"], 0.8, 0.0, None, 1, matching="mutual")[0]["matched_prev"])


def test_empty_tables_a_refused_frame_and_nan():
    # no cluster at all, then frames whose clusters all find their partner at level 0 (A is empty at level 1), then nobody again
    s = _seq([[], [(0.0, 0.0), (5.0, 0.0)], [(0.1, 0.0), (5.1, 0.0)], [(0.2, 0.0), (5.2, 0.0)], [], [(0.3, 0.0)], []])
    seen = [(k, t) for k, t, *_ in ta.level_tables(s, s["node_ptr"], 0.8, 0.0, None, 1)]
    assert seen == [(0, 2), (0, 3), (1, 5)]   # every other (level, frame) has an empty A or an empty B
    _, want = _optimal(s, 0.8, 0.0, None, 1)
    assert want["cluster_track"].tolist() == [0, 1, 0, 1, 0, 1, 0] and want["matched_gap"].tolist() == [-1, -1, 0, 0, 0, 0, 1]
    # a refused frame (count -1) in the middle still counts as a frame and links to nothing
    s = _seq([[(0.0, 0.0), (1.0, 0.0)], [(0.1, 0.0), (9.0, 9.0), (1.1, 0.0)], [(0.2, 0.0), (1.2, 0.0)]])
    s["count"][1] = -1
    _, want = _optimal(s, 0.8, 0.0, None, 1)
    assert want["cluster_track"].tolist() == [0, 1, -1, -1, -1, 0, 1] and want["matched_gap"].tolist() == [-1, -1, -1, -1, -1, 1, 1]
    _optimal(s, 0.8, 0.0, None, 0)
    # a NaN position is outside every gate
    s = _seq([[(0.0, 0.0), (0.7, 0.0)], [(0.3, 0.0), (float("nan"), 0.0)], [(0.3, 0.0), (0.6, float("nan")), (-0.4, 0.0)]])
    _, want = _optimal(s, 0.8, 0.0, None, 1)   # (the last cluster finds frame 0's second one again at level 1: 1.1 <= 1.6)
    assert want["matched_prev"].tolist() == [-1, -1, 0, -1, 0, -1, 1] and want["matched_gap"].tolist() == [-1, -1, 0, -1, 0, -1, 1]
    # a NaN embedding with lam = 1: the cost is NaN, the pair not admissible, and the call returns
    emb = np.array([[1, 0], [0, 1], [1, 0], [np.nan, 0], [1, 0], [0, 1]], np.float32)
    s = _seq([[(0.0, 0.0), (0.7, 0.0)], [(0.3, 0.0), (-0.6, 0.0)], [(0.3, 0.1), (0.7, 0.1)]], emb)
    _, want = _optimal(s, 0.8, 1.0, None, 1)
    assert want["matched_prev"].tolist() == [-1, -1, 0, -1, 0, 1] and want["matched_gap"].tolist() == [-1, -1, 0, -1, 0, 1]


# ---- 5. miss_cost ---------------------------------------------------------------------------------------------------------------------
def test_miss_cost():
    summ = tg.hide_sequence(np.random.default_rng(7), 12, 40, 8, arena=6.0, max_hide=1, noise=0.3, max_alive=70)
    _, at_default = _optimal(summ, 0.8, 0.0, None, 1)
    _, explicit = _optimal(summ, 0.8, 0.0, None, 1, miss_cost=1.0)   # the default of lam = 0, spelled out
    _, cheap = _optimal(summ, 0.8, 0.0, None, 1, miss_cost=0.5)
    _, dear = _optimal(summ, 0.8, 0.0, None, 1, miss_cost=4.0)
    for k in FIELDS:
        assert np.array_equal(at_default[k], explicit[k]), k
    # below some admissible costs: no pair dearer than 0.5 is taken any more, and some were
    def dearest(want, miss):
        worst = []
        def visit(k, t, d, dcos, cost, ok):
            worst.append((k, t, cost, ok))
        ta._walk(summ, summ["node_ptr"], 0.8, 0.0, None, 1, tg.new_state(), "optimal", miss, visit)
        ptr, out = summ["node_ptr"], 0.0
        for v in np.flatnonzero(want["matched_gap"] >= 0):
            t = int(np.searchsorted(ptr, v, side="right") - 1)
            k, b = int(want["matched_gap"][v]), int(want["matched_prev"][v])
            d = np.linalg.norm(summ["pos"][v] - summ["pos"][ptr[t - 1 - k] + b])
            out = max(out, float(d / (0.8 * (k + 1))))
        return out
    print("dearest pair taken at miss_cost 1, 0.5, 4:", dearest(at_default, 1.0), dearest(cheap, 0.5), dearest(dear, 4.0))
    assert dearest(at_default, 1.0) > 0.5 >= dearest(cheap, 0.5)
    assert (cheap["matched_gap"] >= 0).sum() < (at_default["matched_gap"] >= 0).sum()
    # above the default, on a table without ties: w = cost - miss_cost moves every pair alike and no pair was dearer than the default,
    # so in exact arithmetic the optimum is the same set; in fp64 the sums round differently, which only a tie could turn into other pairs
    s = _seq([[(0.0, 0.0), (0.7, 0.0), (3.0, 0.0)], [(0.3, 0.0), (-0.6, 0.0), (3.5, 0.0), (0.9, 0.0)]])
    _, a = _optimal(s, 0.8, 0.0)
    _, b = _optimal(s, 0.8, 0.0, miss_cost=7.0)
    assert a["matched_prev"].tolist() == b["matched_prev"].tolist() == [-1, -1, -1, 0, -1, 2, 1]
    for k in FIELDS:
        assert np.array_equal(dear[k], at_default[k]), k   # (and on this crowded sequence too)


# ---- 6. refusals: before any launch, the state does not move --------------------------------------------------------------------------
def _ring(n, shift=0.0):
    return [(3.0 * i + shift, 0.0) for i in range(n)]


def test_refusals_leave_the_state_alone():
    from gnn_cca_amd.tracking import MAX_OPTIMAL_FRAME_NODES, FrameLinker
    assert MAX_OPTIMAL_FRAME_NODES == 128
    first, second, big = _seq([_ring(128)]), _seq([_ring(100, 0.2)]), _seq([_ring(5, 0.1), _ring(129, 0.1)])
    both = _seq([_ring(128), _ring(100, 0.2)])
    want, _ = ta.link_gap(both, both["node_ptr"], 0.8, 0.0, None, 1, matching="optimal")
    link = FrameLinker(0.8, lam=0.0, max_gap=1, matching="optimal")
    t0 = link(_upload(first))
    for dev in ("cpu", "cuda"):   # CPU tensors: a refusal that came after the GPU was touched would be a RuntimeError
        with pytest.raises(ValueError, match="129 detections"):
            link(_upload(big, dev=dev))
    t1 = link(_upload(second))   # ... and the 128-frame is still what frame 0 of this call is linked to
    torch.cuda.synchronize()
    for k in FIELDS:
        assert torch.equal(torch.cat([getattr(t0, k), getattr(t1, k)]).cpu(), torch.from_numpy(want[k])), k
    assert int(t1.next_id.item()) == want["next_id"] == 128 and (t1.matched_gap == 0).all()

    # a 129-detection frame in the carried history: only a linker whose matching was changed after it had linked can hold one
    both = _seq([_ring(129), _ring(100, 0.2)])
    want, _ = tg.link_gap(both, both["node_ptr"], 0.8, 0.0, None, 1)
    link = FrameLinker(0.8, lam=0.0, max_gap=1)
    t0 = link(_upload(both, 0, 1))
    link.matching = "optimal"
    with pytest.raises(ValueError, match=r"carried history has 129 detections.*reset\(\)"):
        link(_upload(second))
    link.matching = "mutual"
    t1 = link(_upload(both, 1, 2))
    torch.cuda.synchronize()
    for k in FIELDS:
        assert torch.equal(torch.cat([getattr(t0, k), getattr(t1, k)]).cpu(), torch.from_numpy(want[k])), k
    assert int(t1.next_id.item()) == want["next_id"] == 129
    link.matching = "optimal"
    link.reset()   # mixing needs reset(): after it the same linker takes the frames it can hold, ids from 0
    _same_tracks(link(_upload(second)), ta.link_gap(second, second["node_ptr"], 0.8, 0.0, None, 1, matching="optimal")[0])
    # the state of the adjacent-frame linker (max_gap = 0, mutual) has another layout: refused by name
    link = FrameLinker(0.8, lam=0.0)
    t0 = link(_upload(first))
    link.matching = "optimal"
    with pytest.raises(ValueError, match=r"adjacent-frame linker.*reset\(\)"):
        link(_upload(second))
    link.matching = "mutual"
    t1 = link(_upload(second))
    torch.cuda.synchronize()
    assert int(t1.next_id.item()) == 128 and t1.matched_prev.tolist() == list(range(100))

    # a bad matching, and miss_cost with 'mutual': refused when the linker is made
    for kw in (dict(matching="hungarian"), dict(matching=None), dict(miss_cost=1.0), dict(matching="mutual", miss_cost=2.0),
               dict(matching="optimal", miss_cost=0.0), dict(matching="optimal", miss_cost=float("nan"))):
        with pytest.raises(ValueError):
            FrameLinker(0.8, **kw)
