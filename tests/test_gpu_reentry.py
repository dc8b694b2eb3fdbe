"""TrackGallery on the GPU against tests/reentry_oracle.py: cluster_identity, node_identity, reentered_from and the ring's owner / last /
continued / identity exactly, the ring's fp32 sums bit for bit -- over look-alike sequences with occlusions longer than the linker's
max_gap, with max_speed, a small window that wraps the ring, the state carried across calls, appearance rows of 2048 and of 17 columns,
empty and refused frames, a FramePipeline result, another stream, the refusals, and TrackScorer on the identities.  The frames are linked
on the DEVICE (max_step = 0.8, lam = 1) and the oracle is given those tracks.  Every case first asserts, on the ORACLE's numbers, that
no decision hangs on less than 1e-9 and that it exercises what it is about."""
import copy
import functools

import numpy as np
import pytest
import torch

import reentry_oracle as ro
import track_score_oracle as ts
import tracking_gap_oracle as tg
from test_gpu_tracking_gap import _upload

pytestmark = pytest.mark.gpu

OUT = ("cluster_identity", "node_identity", "reentered_from")
RING = ("owner", "last", "continued", "identity")
CASES = [(1, 12, 24, 1, 6, 0.15), (3, 30, 24, 0, 5, 0.2), (7, 40, 12, 1, 5, 0.25), (4, 70, 16, 2, 8, 0.15)]   # seed, persons, g, M, max_hide, p_hide
MAX_COS = 0.3


@functools.lru_cache(maxsize=None)
def sequence(case):
    seed, persons, g, m, max_hide, p_hide = CASES[case]
    return ro.lookalike_sequence(seed, g, persons, max_hide, p_hide)


def _linker(m):
    from gnn_cca_amd.tracking import FrameLinker
    return FrameLinker(max_step=0.8, lam=1.0, max_gap=m)


def _host_tracks(t):
    torch.cuda.synchronize()
    return {k: getattr(t, k).cpu().numpy() for k in ("cluster_track", "node_track", "matched_prev", "matched_gap")}


def _assert_margins(seq, tr, m, state=None, **kw):
    """The precondition of exact equality: the kernel's fp64 dot product is a chain of fused multiply-adds and its norms are lane-strided
    sums, so it differs from the oracle's in rounding only (~R * 1e-16): no decision of the oracle may hang on less than 1e-9."""
    gaps = ro.margins(seq, seq["node_ptr"], tr, m, MAX_COS, state=state, **kw)
    print("margins (cost, dcos, d) and rows / columns with two admissible entries:", gaps)
    assert all(v > 1e-9 for v in gaps[:3]), gaps
    return gaps


def _same(ids, want):
    torch.cuda.synchronize()
    for k in OUT:
        got, ref = getattr(ids, k).cpu(), torch.from_numpy(want[k])
        assert got.dtype == torch.int64 and torch.equal(got, ref), k


def _same_ring(gal, st):
    torch.cuda.synchronize()
    ring = gal.ring
    for k in RING:
        assert torch.equal(ring[k].cpu(), torch.from_numpy(st[k])), k
    assert torch.equal(ring["pos"].cpu(), torch.from_numpy(st["pos"]))
    assert torch.equal(ring["sum"].cpu().view(torch.int32), torch.from_numpy(st["sum"]).view(torch.int32))   # fp32 additions in a stated order
    assert gal.frames_seen == st["seen"]
    hist = gal._hist.cpu().numpy()
    off = 0
    for rows, ident in zip(gal._frame_rows, st["ident_frames"]):     # the identity history: a frame's rows, -1 beyond its count
        assert np.array_equal(hist[off:off + len(ident)], ident) and (hist[off + len(ident):off + rows] == -1).all()
        off += rows


def _idsw(seq, node_ids):
    return ts.score(seq["person"], np.zeros(len(seq["person"]), np.int32), node_ids, seq["node_ptr"], 1024, 8)[2]["IDSW"]


def _run(case, **kw):
    """Link on the device, the gallery on the device, the oracle on the device's tracks -> (seq, tracks, oracle out, oracle state, gallery)."""
    from gnn_cca_amd.reentry import TrackGallery
    m = CASES[case][3]
    seq = sequence(case)
    link = _linker(m)
    s = _upload(seq)
    t = link(s)
    gal = TrackGallery(link, MAX_COS, **kw)
    ids = gal(s, t)
    tr = _host_tracks(t)
    gaps = _assert_margins(seq, tr, m, **kw)
    want, st = ro.gallery(seq, seq["node_ptr"], tr, m, MAX_COS, **kw)
    _same(ids, want)
    _same_ring(gal, st)
    return seq, tr, want, gaps, ids


@pytest.mark.parametrize("case", range(len(CASES)))
def test_returning_persons_get_their_identity_back(case):
    seq, tr, want, gaps, _ = _run(case)
    births = (tr["matched_prev"] < 0) & (tr["cluster_track"] >= 0)
    print("births:", int(births.sum()), "re-entries:", int((want["reentered_from"] >= 0).sum()), "clusters per frame:", seq["count"].tolist())
    assert (want["reentered_from"] >= 0).any()                          # somebody comes back
    assert (births & (want["reentered_from"] < 0)).any()                # a birth is left alone
    assert gaps[3] >= 1                                                 # a row or a column with two admissible entries
    assert _idsw(seq, want["node_identity"]) < _idsw(seq, tr["node_track"])
    if case == 3:
        # past one wave of clusters per frame, and of tracks in the window of a birth that re-enters
        assert seq["count"].max() > 64 and (tr["cluster_track"][want["reentered_from"] >= 0] > 64).any()


@pytest.mark.parametrize("case", [0, 3])
def test_max_speed_keeps_far_tracks_away(case):
    seq, tr, want, _, _ = _run(case, max_speed=0.5)
    free, _ = ro.gallery(seq, seq["node_ptr"], tr, CASES[case][3], MAX_COS)
    changed = int((free["cluster_identity"] != want["cluster_identity"]).sum())
    print("decisions max_speed changes:", changed)
    assert (want["reentered_from"] >= 0).any()
    if case == 3:
        assert changed >= 1


def _in_calls(case, edges, **kw):
    """The sequence cut at `edges`, linker and gallery carried across the calls on the device, the oracle carried beside them."""
    from gnn_cca_amd.reentry import TrackGallery
    m = CASES[case][3]
    seq = sequence(case)
    link = _linker(m)
    gal = TrackGallery(link, MAX_COS, **kw)
    st, wants, trs = None, [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        part = tg.frames_of(seq, lo, hi)
        s = _upload(seq, lo, hi)
        t = link(s)
        ids = gal(s, t)
        tr = _host_tracks(t)
        _assert_margins(part, tr, m, state=st, **kw)
        want, st = ro.gallery(part, part["node_ptr"], tr, m, MAX_COS, state=st, **kw)
        _same(ids, want)
        wants.append(want)
        trs.append(tr)
    _same_ring(gal, st)
    return seq, {k: np.concatenate([w[k] for w in wants]) for k in OUT}, {k: np.concatenate([t[k] for t in trs]) for k in trs[0]}, st


@pytest.mark.parametrize("edges", [(0, 5, 6, 17, 24), tuple(range(25))], ids=["three-cuts", "frame-by-frame"])
def test_the_state_carries_across_calls(edges):
    seq, got, tr, st = _in_calls(0, edges)
    whole, wst = ro.gallery(seq, seq["node_ptr"], tr, CASES[0][3], MAX_COS)     # the same tracks in ONE call of the oracle
    for k in OUT:
        assert np.array_equal(got[k], whole[k]), k
    assert (got["reentered_from"] >= 0).sum() >= 10 and np.array_equal(st["sum"], wst["sum"])


def test_a_small_window_forgets_and_the_ring_wraps():
    seq = sequence(0)
    max_batch = int(np.diff(seq["node_ptr"]).max())
    _, got, tr, st = _in_calls(0, tuple(range(25)), window=8, max_batch=max_batch)
    wide, _ = ro.gallery(seq, seq["node_ptr"], tr, CASES[0][3], MAX_COS)
    lost = (wide["reentered_from"] >= 0) & (tr["cluster_track"] - wide["reentered_from"] > 8)
    assert lost.any() and (got["reentered_from"][lost] != wide["reentered_from"][lost]).all()     # older than W births: forgotten
    hit = got["reentered_from"] >= 0
    assert hit.any() and (tr["cluster_track"][hit] - got["reentered_from"][hit] <= 8).all()
    assert (st["owner"] >= 8 + max_batch).any()                                                   # slots were re-used


def _three_frames(r, seed):
    """3 frames of 3 clusters, M = 0: A and B are seen in frame 0, nobody known in frame 1, A and B come back in frame 2 with a stranger."""
    rng = np.random.default_rng(seed)
    look = rng.standard_normal((9, r))
    row = lambda p: (look[p] + 0.05 * rng.standard_normal(r)).astype(np.float32)
    who = [[0, 1, 2], [3, 4, 5], [1, 6, 0]]
    pos = np.array([[5.0 * p, 3.0] for p in range(9)])     # nobody within the linker's reach of anybody else
    n = 9
    return dict(count=np.full(3, 3, np.int32), rank=np.tile(np.arange(3), 3).astype(np.int32), size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32),
                pos=np.array([pos[p] for f in who for p in f], np.float64), emb=np.stack([row(p) for f in who for p in f]),
                node_ptr=np.array([0, 3, 6, 9], np.int64), person=np.array([p for f in who for p in f], np.int64))


@pytest.mark.parametrize("r", [2048, 17])
def test_full_depth_rows_and_a_tail_that_does_not_fill_a_tile(r):
    from gnn_cca_amd.reentry import TrackGallery
    seq = _three_frames(r, 50 + r)
    link = _linker(0)
    s = _upload(seq)
    t = link(s)
    gal = TrackGallery(link, MAX_COS, window=16, max_batch=16)
    ids = gal(s, t)
    tr = _host_tracks(t)
    assert (tr["matched_prev"] < 0).all()
    _assert_margins(seq, tr, 0, window=16, max_batch=16)
    want, st = ro.gallery(seq, seq["node_ptr"], tr, 0, MAX_COS, window=16, max_batch=16)
    assert want["reentered_from"].tolist() == [-1] * 6 + [1, -1, 0] and want["cluster_identity"].tolist() == [0, 1, 2, 3, 4, 5, 1, 7, 0]
    _same(ids, want)
    _same_ring(gal, st)


def test_an_empty_and_a_refused_frame_in_the_middle_of_a_batch():
    from gnn_cca_amd.reentry import TrackGallery
    seed, persons, g, m, max_hide, p_hide = CASES[0]
    seq = ro.lookalike_sequence(seed, g, persons, max_hide, p_hide, empty=(9,))
    v0, v1 = (int(v) for v in seq["node_ptr"][14:16])
    seq["count"][14], seq["rank"][v0:v1], seq["pos"][v0:v1], seq["emb"][v0:v1] = -1, -1, 0.0, 0.0     # as the summaries leave a refused frame
    assert seq["count"][9] == 0 and v1 > v0
    link = _linker(m)
    s = _upload(seq)
    t = link(s)
    gal = TrackGallery(link, MAX_COS)
    ids = gal(s, t)
    tr = _host_tracks(t)
    _assert_margins(seq, tr, m)
    want, st = ro.gallery(seq, seq["node_ptr"], tr, m, MAX_COS)
    after = np.arange(len(seq["rank"])) >= v1
    assert (want["reentered_from"][after] >= 0).any() and (want["cluster_identity"][v0:v1] == -1).all() and (want["node_identity"][v0:v1] == -1).all()
    _same(ids, want)
    _same_ring(gal, st)
    assert st["seen"] == g                                          # both frames count as frames
    # ... and frame by frame: a call whose only frame is empty (N = 0) or refused passes time and nothing else
    link, gal, parts = _linker(m), TrackGallery(link, MAX_COS), []
    for q in range(g):
        s1 = _upload(seq, q, q + 1)
        parts.append(gal(s1, link(s1)))
    _same(type(ids)(*(torch.cat([getattr(p, k) for p in parts]) for k in OUT)), want)
    _same_ring(gal, st)


def test_another_stream():
    from gnn_cca_amd.reentry import TrackGallery
    seq, m = sequence(0), CASES[0][3]
    stream = torch.cuda.Stream()
    link = _linker(m)
    with torch.cuda.stream(stream):
        s = _upload(seq)
        t = link(s)
        gal = TrackGallery(link, MAX_COS)
        ids = gal(s, t)
    stream.synchronize()
    tr = _host_tracks(t)
    want, st = ro.gallery(seq, seq["node_ptr"], tr, m, MAX_COS)
    _same(ids, want)
    _same_ring(gal, st)


def test_refusals_leave_the_state_where_it_was():
    from gnn_cca_amd.reentry import TrackGallery
    from gnn_cca_amd.tracking import ClusterSummaries, Tracks
    seq, m = sequence(0), CASES[0][3]
    link = _linker(m)
    gal = TrackGallery(link, MAX_COS, max_batch=160)
    s5 = _upload(seq, 0, 5)
    t5 = link(s5)
    gal(s5, t5)
    torch.cuda.synchronize()
    before = (gal._ring.clone(), gal._hist.clone(), list(gal._frame_rows), gal.frames_seen)
    s_all = _upload(seq)
    t_all = _linker(m)(s_all)
    other = ClusterSummaries(s5.count, s5.rank, s5.size, s5.n_cams, s5.pos, s5.emb[:, :8].contiguous(), s5.node_ptr, s5.node_ptr_dev)
    no_emb = ClusterSummaries(s5.count, s5.rank, s5.size, s5.n_cams, s5.pos, s5.emb[:, :0].contiguous(), s5.node_ptr, s5.node_ptr_dev)
    cpu = ClusterSummaries(*(getattr(s5, k).cpu() for k in ("count", "rank", "size", "n_cams", "pos", "emb")), s5.node_ptr, s5.node_ptr_dev.cpu())
    cpu_t = Tracks(t5.cluster_track.cpu(), t5.node_track.cpu(), t5.matched_prev.cpu(), t5.next_id.cpu(), None, t5.matched_gap.cpu())
    for x, tracks, err in ((s_all, t_all, ValueError), (other, t5, ValueError), (no_emb, t5, ValueError), (s5, t_all, ValueError),
                           (s5, object(), ValueError), (object(), t5, ValueError), (cpu, cpu_t, RuntimeError)):
        with pytest.raises(err):
            gal(x, tracks)
    torch.cuda.synchronize()
    assert torch.equal(gal._ring, before[0]) and torch.equal(gal._hist, before[1]) and (gal._frame_rows, gal.frames_seen) == before[2:]
    # ... and the sequence goes on as if nothing had been tried
    s_rest = _upload(seq, 5, 24)
    t_rest = link(s_rest)
    ids = gal(s_rest, t_rest)
    first, rest = tg.frames_of(seq, 0, 5), tg.frames_of(seq, 5, 24)
    _, st = ro.gallery(first, first["node_ptr"], _host_tracks(t5), m, MAX_COS, max_batch=160)
    _assert_margins(rest, _host_tracks(t_rest), m, state=st, max_batch=160)
    want, st = ro.gallery(rest, rest["node_ptr"], _host_tracks(t_rest), m, MAX_COS, max_batch=160, state=st)
    assert (want["reentered_from"] >= 0).any()
    _same(ids, want)
    _same_ring(gal, st)
    gal.reset()
    assert gal.ring is None and gal.frames_seen == 0


def test_the_scorer_takes_identities_where_tracks_stood():
    from gnn_cca_amd.tracking import TrackScorer
    seq, tr, want, _, ids = _run(2)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    person, cam = dev(seq["person"], np.int64), dev(np.zeros(len(seq["person"])), np.int32)
    ptr = seq["node_ptr"].tolist()
    with_gallery, without = TrackScorer(), TrackScorer()
    with_gallery.add_raw(person, cam, ids.node_identity, ptr)
    without.add_raw(person, cam, dev(tr["node_track"], np.int64), ptr)
    cam_h = np.zeros(len(seq["person"]), np.int32)
    res = with_gallery.result()
    assert res == ts.score(seq["person"], cam_h, want["node_identity"], seq["node_ptr"], 1024, 8)[2]
    base = without.result()
    print("without the gallery:", {k: base[k] for k in ("IDSW", "IDF1", "tracks")}, "with:", {k: res[k] for k in ("IDSW", "IDF1", "tracks")})
    assert res["IDSW"] < base["IDSW"] and res["IDF1"] > base["IDF1"] and res["tracks"] < base["tracks"]


def test_a_pipeline_result_goes_in_directly():
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.reentry import TrackGallery
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(34)
    k, cams = 14, 4
    one = dict(id_cam=rng.integers(0, cams, size=k), ids=rng.integers(0, 6, size=k), xw=rng.uniform(-10, 10, k), yw=rng.uniform(-10, 10, k),
               node=rng.standard_normal((k, 2048)).astype(np.float32), reid=rng.standard_normal((k, 256)).astype(np.float32))
    # frame 2 shows frame 0's detections again after an empty frame: too long for a linker without max_gap, the gallery's business
    f = {q: np.concatenate([one[q], one[q]]) for q in one}
    f["xw"][k:] += rng.normal(0, 0.05, k)
    f["yw"][k:] += rng.normal(0, 0.05, k)
    sizes, max_dist = np.array([k, 0, k]), np.array([50.0, 50.0, 50.0])
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    pipe = FramePipeline(m)
    args = (f["xw"], f["yw"], f["ids"], f["id_cam"], sizes, max_dist, torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda())
    r = pipe(*args)
    with torch.no_grad():   # put the decision boundary inside the logits so that the partition is neither trivial one
        sd = m.state_dict()
        key = [q for q in sd if q.startswith("classifier.") and q.endswith(".bias")][-1]
        sd[key] -= r.outputs["classified_edges"][-1].median()
        m.load_state_dict(sd)
    r = pipe(*args)
    link = FrameLinker(max_step=3.0)
    t = link(r)
    gal = TrackGallery(link, MAX_COS, window=64, max_batch=64)
    ids = gal(r, t)
    s = r.identities()
    host = {q: getattr(s, q).cpu().numpy() for q in ("count", "rank", "pos", "emb")}
    host["node_ptr"] = np.asarray(r.batch.node_ptr, np.int64)
    tr = _host_tracks(t)
    assert (tr["matched_prev"] < 0).all() and host["count"][1] == 0
    _assert_margins(host, tr, 0, window=64, max_batch=64)
    want, st = ro.gallery(host, host["node_ptr"], tr, 0, MAX_COS, window=64, max_batch=64)
    c0, c2 = int(host["count"][0]), int(host["count"][2])
    back = want["reentered_from"][k:k + c2]
    print("clusters:", c0, c2, "re-entries:", int((back >= 0).sum()))
    assert (back >= 0).any() and (back < c0).all()     # clusters of frame 2 are frame 0's again
    _same(ids, want)
    _same_ring(gal, st)
