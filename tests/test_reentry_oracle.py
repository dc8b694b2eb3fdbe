"""The re-entry gallery's rule on its numpy restatement (tests/reentry_oracle.py, which the GPU tests compare the kernels with): hand-made
walks with every identity spelled out, the mutual best and its tie, the consequences the oracle's docstring states (cut independence, the
ring's wrap, a track that outlives its slot), and what the Python front end and the ctypes binding declare and refuse, which needs no GPU."""
import os
import re

import numpy as np
import pytest

import reentry_oracle as ro
import tracking_gap_oracle as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 8
LOOK = np.random.default_rng(5).standard_normal((6, R)).astype(np.float32)   # six unlike appearances


def seq_of(frames):
    """frames: per frame a list of (x, y, appearance row) -> a summaries dict, one single-node cluster per entry."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    rows = [c for f in frames for c in f]
    return dict(count=np.array(counts, np.int32), rank=np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32),
                size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32), pos=np.array([[c[0], c[1]] for c in rows], np.float64).reshape(n, 2),
                emb=np.array([c[2] for c in rows], np.float32).reshape(n, R), node_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))


def run(seq, m, max_cos=0.3, **kw):
    tr, _ = ro.link(seq, m)
    out, st = ro.gallery(seq, seq["node_ptr"], tr, m, max_cos, **kw)
    return tr, out, st


def returning_walk(back_at=(1.0, 1.0)):
    """Person A (appearance 0) is seen at frames 0-2, absent 3-6, back at 7-8, absent 9-12, back at 13; person B (appearance 1) is
    always there, ten units away.  A is rank 0 whenever present."""
    frames = []
    for q in range(14):
        f = []
        if q <= 2:
            f.append((1.0, 1.0, LOOK[0]))
        elif q in (7, 8, 13):
            f.append((back_at[0], back_at[1], LOOK[0]))
        f.append((11.0, 1.0, LOOK[1]))
        frames.append(f)
    return seq_of(frames)


def test_a_returning_person_gets_the_old_identity_back_and_the_chain_goes_on():
    seq = returning_walk()
    tr, out, st = run(seq, 1)
    ptr = seq["node_ptr"]
    assert tr["cluster_track"][ptr[7]] == 2 and tr["cluster_track"][ptr[13]] == 3      # the linker: two fresh tracks
    assert out["cluster_identity"][ptr[7]] == 0 and out["reentered_from"][ptr[7]] == 0  # ... the gallery: A's first identity, from track 0
    assert out["cluster_identity"][ptr[8]] == 0                                         # continued by the linker: through the history
    assert out["cluster_identity"][ptr[13]] == 0 and out["reentered_from"][ptr[13]] == 2   # the second return re-uses the chain
    a_rows = [int(ptr[q]) for q in (0, 1, 2, 7, 8, 13)]
    assert (out["cluster_identity"][a_rows] == 0).all()
    b_rows = [int(ptr[q + 1]) - 1 for q in range(14)]
    assert (out["cluster_identity"][b_rows] == 1).all() and (out["reentered_from"][b_rows] == -1).all()
    assert np.array_equal(out["node_identity"], out["cluster_identity"])
    assert int((out["reentered_from"] >= 0).sum()) == 2
    assert st["continued"][0] == 1 and st["continued"][2] == 1 and st["continued"][3] == 0 and st["seen"] == 14
    assert st["last"][0] == 2 and st["last"][2] == 8 and st["last"][3] == 13 and st["identity"][3] == 0
    assert np.array_equal(st["sum"][0], (LOOK[0] + LOOK[0]) + LOOK[0])                  # one fp32 addition per cluster, in frame order


def test_max_age_and_max_speed_keep_the_identity_away():
    seq = returning_walk()
    _, out, _ = run(seq, 1, max_age=3)          # absent for 7 - 2 = 5 frames
    assert int((out["reentered_from"] >= 0).sum()) == 0 and out["cluster_identity"][seq["node_ptr"][7]] == 2
    _, out, _ = run(seq, 1, max_age=5)
    assert out["cluster_identity"][seq["node_ptr"][7]] == 0
    far = returning_walk(back_at=(1.0, 9.0))    # eight units in five frames
    _, out, _ = run(far, 1, max_speed=1.5)
    assert out["cluster_identity"][far["node_ptr"][7]] == 2 and out["reentered_from"][far["node_ptr"][7]] == -1
    _, out, _ = run(far, 1, max_speed=1.7)
    assert out["cluster_identity"][far["node_ptr"][7]] == 0
    _, out, _ = run(far, 1)
    assert out["cluster_identity"][far["node_ptr"][7]] == 0


def test_two_births_want_the_same_track_the_cheaper_gets_it_a_tie_goes_to_the_smaller_rank():
    near = (LOOK[0] + 0.02 * LOOK[2]).astype(np.float32)
    nearer = (LOOK[0] + 0.01 * LOOK[2]).astype(np.float32)
    for first, second, winner in ((near, nearer, 1), (nearer, near, 0), (near, near, 0)):
        frames = [[(1.0, 1.0, LOOK[0])]] + [[] for _ in range(3)] + [[(5.0, 5.0, first), (9.0, 9.0, second)]]
        seq = seq_of(frames)
        tr, out, st = run(seq, 1)
        v = int(seq["node_ptr"][4])
        assert tr["cluster_track"][v:v + 2].tolist() == [1, 2]
        want = [1, 2]
        want[winner] = 0
        assert out["cluster_identity"][v:v + 2].tolist() == want
        assert out["reentered_from"][v:v + 2].tolist() == [0 if i == winner else -1 for i in range(2)]
        mg = ro.margins(seq, seq["node_ptr"], tr, 1, 0.3)
        assert mg[3] == 1 and (mg[0] == 0.0) == (first is second)     # one column with two admissible entries; the tie is exact


CUT_CASE = dict(g=24, persons=12, max_hide=6, p_hide=0.15, m=1)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("cuts", [(5, 6, 17), None])
def test_cutting_a_sequence_into_calls_changes_nothing(seed, cuts):
    c = CUT_CASE
    seq = ro.lookalike_sequence(seed, c["g"], c["persons"], c["max_hide"], c["p_hide"])
    _, want, wst = run(seq, c["m"])
    assert (want["reentered_from"] >= 0).any()
    edges = [0] + (list(cuts) if cuts else list(range(1, c["g"]))) + [c["g"]]
    lst, gst, parts = None, None, []
    for lo, hi in zip(edges[:-1], edges[1:]):
        part = tg.frames_of(seq, lo, hi)
        tr, lst = ro.link(part, c["m"], state=lst)
        out, gst = ro.gallery(part, part["node_ptr"], tr, c["m"], 0.3, state=gst)
        parts.append(out)
    for k in ("cluster_identity", "node_identity", "reentered_from"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), want[k]), k
    for k in ("owner", "sum", "last", "pos", "identity", "continued"):
        assert np.array_equal(gst[k], wst[k]), k
    assert gst["seen"] == wst["seen"] == c["g"] and len(gst["ident_frames"]) == c["m"] + 1
    assert all(np.array_equal(a, b) for a, b in zip(gst["ident_frames"], wst["ident_frames"]))


def test_the_window_forgets_and_the_ring_wraps():
    """W = 8 and max_batch = the call's N (one frame per call): a track older than 8 births is not found, slots are re-used, and an
    eligible track's slot was never taken by a birth of the same call."""
    c = CUT_CASE
    seq = ro.lookalike_sequence(1, c["g"], c["persons"], c["max_hide"], c["p_hide"])
    tr_all, wide, _ = run(seq, c["m"])
    births = tr_all["matched_prev"] < 0
    lost = births & (wide["reentered_from"] >= 0) & (tr_all["cluster_track"] - wide["reentered_from"] > 8)
    assert lost.any()
    max_batch = int(np.diff(seq["node_ptr"]).max())
    lst, gst, parts = None, None, []
    for q in range(c["g"]):
        part = tg.frames_of(seq, q, q + 1)
        tr, lst = ro.link(part, c["m"], state=lst)
        before = gst
        out, gst = ro.gallery(part, part["node_ptr"], tr, c["m"], 0.3, window=8, max_batch=max_batch, state=gst)
        parts.append(out)
        for j in out["reentered_from"][out["reentered_from"] >= 0].tolist():     # the track that was taken up ...
            sl = j % (8 + max_batch)
            assert before["owner"][sl] == j == gst["owner"][sl]                   # ... still owns its slot after the call's births
            assert before["last"][sl] == gst["last"][sl] and np.array_equal(before["sum"][sl], gst["sum"][sl])   # ... and was final
            assert before["seen"] - before["last"][sl] >= c["m"] + 2 and not before["continued"][sl] and gst["continued"][sl]
    got = np.concatenate([p["reentered_from"] for p in parts])
    assert (got[lost] != wide["reentered_from"][lost]).all()
    hit = got >= 0
    assert hit.any() and ((tr_all["cluster_track"][hit] - got[hit] >= 1) & (tr_all["cluster_track"][hit] - got[hit] <= 8)).all()
    s = 8 + max_batch
    assert len(gst["owner"]) == s and int(tr_all["next_id"]) > s and (gst["owner"] >= s).any()     # the ring wrapped
    with pytest.raises(ValueError):    # N > max_batch
        ro.gallery(seq, seq["node_ptr"], tr_all, c["m"], 0.3, window=8, max_batch=max_batch)


def test_a_track_alive_for_longer_than_the_ring_keeps_its_identity():
    rng = np.random.default_rng(9)
    frames = [[(1.0, 1.0, LOOK[1])] + [(20.0 + 5 * q, 40.0, rng.standard_normal(R).astype(np.float32))] for q in range(12)]
    seq = seq_of(frames)
    lst, gst, ids = None, None, []
    for q in range(12):
        part = tg.frames_of(seq, q, q + 1)
        tr, lst = ro.link(part, 0, state=lst)
        out, gst = ro.gallery(part, part["node_ptr"], tr, 0, 0.3, window=1, max_batch=2, state=gst)
        ids.append(out["cluster_identity"].tolist())
        assert tr["cluster_track"][0] == 0
    assert all(i[0] == 0 for i in ids) and [i[1] for i in ids] == list(range(1, 13))
    assert gst["owner"][0] == 12 and (gst["owner"] != 0).all()      # track 0's slot went to younger tracks long ago
    assert gst["last"][0] == 11 and np.array_equal(gst["sum"][0], seq["emb"][-1])   # ... whose sums do not hold track 0's later rows


def _cpu_summaries(seq):
    import torch
    from gnn_cca_amd.tracking import ClusterSummaries
    t = torch.from_numpy
    return ClusterSummaries(t(seq["count"]), t(seq["rank"]), t(seq["size"]), t(seq["n_cams"]), t(seq["pos"]), t(seq["emb"]),
                            seq["node_ptr"].tolist(), t(seq["node_ptr"].astype(np.int32)))


def _cpu_tracks(tr):
    import torch
    from gnn_cca_amd.tracking import Tracks
    t = torch.from_numpy
    return Tracks(t(tr["cluster_track"]), t(tr["node_track"]), t(tr["matched_prev"]), torch.tensor([tr["next_id"]]), None, t(tr["matched_gap"]))


BAD_ARGS = [dict(max_cos=-0.1), dict(max_cos=2.5), dict(max_cos="0.3"), dict(max_cos=True), dict(max_cos=float("nan")), dict(window=0),
            dict(window=1.5), dict(window=True), dict(max_batch=0), dict(max_batch=2.0), dict(max_age=2), dict(max_age=3.0), dict(max_age=True),
            dict(max_speed=0), dict(max_speed=-1.0), dict(max_speed=float("inf")), dict(max_speed=float("nan")), dict(max_speed="1")]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda b: "-".join(f"{k}={v!r}" for k, v in b.items()))
def test_the_constructor_refuses(bad):
    from gnn_cca_amd.reentry import TrackGallery
    from gnn_cca_amd.tracking import FrameLinker
    args = dict(max_cos=0.3)
    args.update(bad)
    with pytest.raises(ValueError):
        TrackGallery(FrameLinker(0.8, max_gap=1), **args)
    with pytest.raises(ValueError):
        ro.check_args(1, **args)


def test_the_front_end_refuses_before_it_touches_the_gpu():
    import torch
    from gnn_cca_amd.reentry import MAX_WINDOW, Identities, TrackGallery
    from gnn_cca_amd.tracking import FrameLinker
    link = FrameLinker(0.8, max_gap=1)
    with pytest.raises(ValueError):
        TrackGallery(object(), 0.3)
    with pytest.raises(ValueError, match="window"):     # the walking workgroup keeps a frame's candidate tracks in LDS
        TrackGallery(link, 0.3, window=MAX_WINDOW + 1)
    assert MAX_WINDOW == 4096 and TrackGallery(link, 0.3, window=MAX_WINDOW).n_slots == 4096 + 2048
    gal = TrackGallery(link, 0.3, window=8, max_batch=40, max_age=3, max_speed=1.0)   # the smallest max_age a linker with max_gap = 1 allows
    assert (gal.n_slots, gal.frames_seen, gal.ring) == (48, 0, None)
    seq = returning_walk()
    tr, _ = ro.link(seq, 1)
    s, t = _cpu_summaries(seq), _cpu_tracks(tr)
    with pytest.raises(RuntimeError, match="MI355X"):     # CPU tensors, as in the other modules
        gal(s, t)
    with pytest.raises(ValueError, match="ClusterSummaries"):
        gal(object(), t)
    with pytest.raises(ValueError, match="Tracks"):
        gal(s, object())
    no_emb = _cpu_summaries(seq)
    no_emb.emb = torch.zeros((len(seq["rank"]), 0))
    with pytest.raises(ValueError, match="appearance"):
        gal(no_emb, t)
    with pytest.raises(ValueError, match="max_batch"):
        TrackGallery(link, 0.3, max_batch=len(seq["rank"]) - 1)(s, t)
    short = _cpu_tracks({k: (v[:-1] if isinstance(v, np.ndarray) else v) for k, v in tr.items()})
    with pytest.raises(ValueError, match="rows"):
        gal(s, short)
    big = seq_of([[(float(i), 0.0, LOOK[0]) for i in range(4097)]])
    big_tr = dict(cluster_track=np.arange(4097), node_track=np.arange(4097), matched_prev=np.full(4097, -1, np.int32),
                  matched_gap=np.full(4097, -1, np.int32), next_id=4097)
    with pytest.raises(ValueError, match="4096"):
        TrackGallery(link, 0.3, max_batch=8192)(_cpu_summaries(big), _cpu_tracks(big_tr))
    gal._reid_dim = R + 1      # as after a call with other summaries
    with pytest.raises(ValueError, match="reset"):
        gal(s, t)
    gal.reset()
    assert (gal.frames_seen, gal.ring, gal._frame_rows) == (0, None, [])     # nothing moved
    assert Identities.__slots__ == ("cluster_identity", "node_identity", "reentered_from")
    # the oracle refuses the same calls
    for kw, args in ((dict(max_batch=len(seq["rank"]) - 1), (seq, tr)), (dict(), (big, big_tr))):
        with pytest.raises(ValueError):
            ro.gallery(args[0], args[0]["node_ptr"], args[1], 1, 0.3, **kw)
    with pytest.raises(ValueError):
        ro.gallery(seq, seq["node_ptr"], tr, 1, 0.3, state=ro.new_state(1024, 2048, R + 1))


def test_tracking_exports_what_it_did():
    import gnn_cca_amd.reentry as re_mod
    import gnn_cca_amd.tracking as tracking
    assert sorted(tracking.__all__) == sorted(["MAX_FRAME_NODES", "MAX_GAP", "MAX_OPTIMAL_FRAME_NODES", "ClusterSummaries", "Tracks",
                                               "cluster_summaries", "cluster_summaries_raw", "FrameLinker", "TrackScorer", "TrackScores"])
    assert re_mod.__all__ == ["MAX_WINDOW", "Identities", "TrackGallery"]


def test_the_new_entries_are_exported_and_declared():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    declared = set(re.findall(r"GNNCCA_API[^;(]*?\b(gnncca_\w+)\s*\(", header))
    names = {"gnncca_reentry_state_bytes", "gnncca_reentry_workspace_bytes", "gnncca_reentry_update"}
    assert names <= declared and names <= set(nat.exported_symbols())
    assert int(re.search(r"#define GNNCCA_REENTRY_MAX_WINDOW (\d+)", header).group(1)) == nat.REENTRY_MAX_WINDOW
    lib = nat.lib()     # loading checks every declared symbol against the library
    s, r = 1024 + 2048, 2048
    assert lib.gnncca_reentry_state_bytes(s, r) == ((44 * s + 255) // 256 * 256 + 4 * s * r + 255) // 256 * 256      # 25 MB, as the docs say
    assert lib.gnncca_reentry_workspace_bytes(512, 1024, 2048) >= 512 * 1024 * 8
    assert lib.gnncca_reentry_workspace_bytes(512, nat.REENTRY_MAX_WINDOW + 1, 2048) == 0
    # the refusals of the entry itself come before any launch and any dereference: no GPU is touched here
    import ctypes as C
    rows = (C.c_int32 * 1)(4)
    def call(**kw):
        a = dict(reid_dim=8, n_nodes=4, n_frames=1, max_frame_nodes=4, max_gap=1, max_cos=0.3, window=8, max_batch=16, has_max_age=0,
                 max_age=0, has_max_speed=0, max_speed=0.0, seen=0)
        a.update(kw)
        return lib.gnncca_reentry_update(None, None, None, None, None, a["reid_dim"], a["n_nodes"], a["n_frames"], a["max_frame_nodes"], None,
                                         None, None, a["max_gap"], a["max_cos"], a["window"], a["max_batch"], a["has_max_age"], a["max_age"],
                                         a["has_max_speed"], a["max_speed"], a["seen"], None, None, None, 0, None, rows, 1, None, None, None,
                                         None, 0, None)
    assert call(n_frames=0) == nat.OK                     # nothing to do
    for kw in (dict(), dict(max_cos=2.5), dict(window=0), dict(max_batch=3), dict(has_max_age=1, max_age=2), dict(has_max_speed=1, max_speed=0.0),
               dict(reid_dim=0), dict(max_gap=9), dict(max_frame_nodes=4097, n_nodes=5000, max_batch=8192), dict(seen=-1)):
        assert call(**kw) == nat.ERR_INVALID_ARG, kw      # (the first: every array is NULL)
