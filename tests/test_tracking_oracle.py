"""The rules of gnn_cca_amd.tracking (cluster summaries, mutual-best linking of consecutive frames, track ids) on hand-written cases
with literal expected ids, properties of their numpy restatement (tests/tracking_oracle.py, which the GPU tests compare the kernels
with), and the argument refusals of the Python front end, which need no GPU."""
import numpy as np
import pytest

import tracking_oracle as to


def _singletons(frames, r=0):
    """frames: per frame a list of (x, y) or (x, y, emb) -> the summaries of one-node clusters."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([p[:2] for f in frames for p in f], np.float64).reshape(n, 2)
    emb = np.array([p[2] for f in frames for p in f], np.float32).reshape(n, r) if r else np.zeros((n, 0), np.float32)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, pos=pos, emb=emb), node_ptr


def test_two_persons_cross_one_leaves_one_enters():
    ea, eb = (1.0, 0.0), (0.0, 1.0)
    frames = [[(0.0, 0.0, ea), (2.0, 0.0, eb)],           # A, B
              [(0.8, 0.0, eb), (1.2, 0.0, ea)],           # B then A: they have crossed, and the rows come in the other order
              [(5.0, 5.0, ea), (0.5, 0.0, eb)]]           # A has left; C enters far away (with A's appearance); B
    s, ptr = _singletons(frames, r=2)
    out, state = to.link(s, ptr, max_step=1.5, lam=1.0)
    assert out["cluster_track"].tolist() == [0, 1, 1, 0, 2, 1]
    assert out["matched_prev"].tolist() == [-1, -1, 1, 0, -1, 0]
    assert out["node_track"].tolist() == [0, 1, 1, 0, 2, 1]
    assert out["next_id"] == 3 and state["next_id"] == 3 and state["track"].tolist() == [2, 1]
    # position alone swaps the two at the crossing: each is nearer to where the OTHER one was
    out0, _ = to.link(s, ptr, max_step=1.5, lam=0.0)
    assert out0["cluster_track"].tolist() == [0, 1, 0, 1, 2, 0] and out0["matched_prev"].tolist() == [-1, -1, 0, 1, -1, 0]
    # somebody who looks like neither takes the nearer one's id unless the appearance gate refuses the pair
    ec = (-1.0, 0.0)
    s2, ptr2 = _singletons(frames[:2] + [[(1.2, 0.0, ec)]], r=2)
    out2, _ = to.link(s2, ptr2, max_step=1.5, lam=1.0)
    assert out2["cluster_track"].tolist()[4:] == [1] and out2["matched_prev"].tolist()[4:] == [0]   # cost 0.4 / 1.5 + 1 against 0 + 2
    out2, _ = to.link(s2, ptr2, max_step=1.5, lam=1.0, max_cos=0.5)
    assert out2["cluster_track"].tolist()[4:] == [2] and out2["matched_prev"].tolist()[4:] == [-1]


def test_exact_ties_on_a_lattice_go_to_the_smaller_index():
    # 3-4-5: both current clusters are exactly 5 from both previous ones, and 5 == max_step is admissible
    s, ptr = _singletons([[(0.0, 0.0), (6.0, 0.0)], [(3.0, 4.0), (3.0, -4.0)]])
    d, _, cost, ok = to.pair_tables(s["pos"][2:4], None, s["pos"][0:2], None, 5.0, lam=0.0)
    assert np.array_equal(d, np.full((2, 2), 5.0)) and ok.all() and np.array_equal(cost, np.ones((2, 2)))
    out, _ = to.link(s, ptr, max_step=5.0, lam=0.0)
    # fwd = [0, 0], bwd = [0, 0]: only (a0, b0) is mutual
    assert out["matched_prev"].tolist() == [-1, -1, 0, -1]
    assert out["cluster_track"].tolist() == [0, 1, 0, 2] and out["next_id"] == 3
    out, _ = to.link(s, ptr, max_step=4.999, lam=0.0)   # just outside: nobody continues
    assert out["cluster_track"].tolist() == [0, 1, 2, 3]


def test_an_empty_frame_ends_every_track():
    s, ptr = _singletons([[(0.0, 0.0)], [], [(0.0, 0.0)]])
    out, state = to.link(s, ptr, max_step=1.0, lam=0.0)
    assert out["cluster_track"].tolist() == [0, 1] and out["matched_prev"].tolist() == [-1, -1] and out["next_id"] == 2
    # the same through the carried state: a batch that ends on an empty frame carries nothing
    s01, ptr01 = _singletons([[(0.0, 0.0)], []])
    _, st = to.link(s01, ptr01, max_step=1.0, lam=0.0)
    assert st["count"] == 0 and st["next_id"] == 1
    s2, ptr2 = _singletons([[(0.0, 0.0)]])
    out2, _ = to.link(s2, ptr2, max_step=1.0, lam=0.0, state=st)
    assert out2["cluster_track"].tolist() == [1]
    # a refused frame (count -1) links to nothing either
    s["count"][0] = -1
    out3, _ = to.link(s, ptr, max_step=1.0, lam=0.0)
    assert out3["cluster_track"].tolist() == [-1, 0]


def test_summaries_by_hand():
    #         frame 0: clusters {0, 2, 3} and {1};   frame 1: empty;   frame 2: one cluster {4, 5}
    labels = np.array([0, 1, 0, 0, 4, 4])
    node_ptr = [0, 4, 4, 6]
    xw, yw = np.array([1.0, 10.0, 2.0, 6.0, 0.5, 1.5]), np.array([0.0, -1.0, 0.0, 3.0, 2.0, 4.0])
    cam = np.array([7, 7, 9, 7, -3, -3])
    emb = np.array([[1, 0], [0, 1], [3, 0], [2, 3], [1, 1], [3, 5]], np.float32)
    s = to.summaries(labels, node_ptr, xw, yw, cam, emb)
    assert s["count"].tolist() == [2, 0, 1] and s["rank"].tolist() == [0, 1, 0, 0, 0, 0]
    assert s["size"].tolist() == [3, 1, 0, 0, 2, 0] and s["n_cams"].tolist() == [2, 1, 0, 0, 1, 0]
    assert s["pos"].tolist() == [[3.0, 1.0], [10.0, -1.0], [0, 0], [0, 0], [1.0, 3.0], [0, 0]]
    assert s["emb"].tolist() == [[2.0, 1.0], [0.0, 1.0], [0, 0], [0, 0], [2.0, 3.0], [0, 0]]
    # a label outside its frame, and a label that is not a root: the frame is refused, its neighbours are not
    for bad in (np.array([0, 1, 0, 4, 4, 4]), np.array([0, 1, 0, 2, 4, 4])):
        r = to.summaries(bad, node_ptr, xw, yw, cam, emb)
        assert r["count"].tolist() == [-1, 0, 1] and r["rank"].tolist() == [-1, -1, -1, -1, 0, 0]
        assert not r["size"][:4].any() and not r["pos"][:4].any() and not r["emb"][:4].any()
        assert np.array_equal(r["pos"][4:], s["pos"][4:]) and np.array_equal(r["emb"][4:], s["emb"][4:])


@pytest.mark.parametrize("seed,lam,max_cos", [(0, 0.0, None), (1, 1.0, None), (2, 0.5, 0.6), (3, 1.0, None)])
def test_matches_are_one_to_one_and_ids_never_return(seed, lam, max_cos):
    rng = np.random.default_rng(seed)
    s = to.walk_sequence(rng, 12, 9, 8, noise=0.4, arena=6.0)   # crowded: many candidates inside max_step
    out, _ = to.link(s, s["node_ptr"], max_step=1.0, lam=lam, max_cos=max_cos)
    ptr = s["node_ptr"]
    seen_before, last_frame = set(), {}
    assert (out["matched_prev"] >= 0).any() and (out["matched_prev"] < 0).any()
    for q in range(len(ptr) - 1):
        tr = out["cluster_track"][ptr[q]:ptr[q + 1]]
        m = out["matched_prev"][ptr[q]:ptr[q + 1]]
        assert len(set(tr.tolist())) == len(tr)                        # no id twice in a frame
        hit = m[m >= 0]
        assert len(set(hit.tolist())) == len(hit)                      # one-to-one
        if q:
            assert (hit < s["count"][q - 1]).all()
            prev = out["cluster_track"][ptr[q - 1]:ptr[q]]
            assert np.array_equal(tr[m >= 0], prev[hit])               # a matched cluster takes its partner's id
        for t, mm in zip(tr.tolist(), m.tolist()):
            if mm < 0:
                assert t not in seen_before                            # a fresh id is fresh
            else:
                assert last_frame[t] == q - 1                          # a chain has no gap
            seen_before.add(t)
            last_frame[t] = q
    fresh = out["cluster_track"][out["matched_prev"] < 0]
    assert fresh.tolist() == list(range(len(fresh))) and out["next_id"] == len(fresh)   # ascending (frame, rank) order from 0


def test_relabelling_the_cameras_changes_nothing():
    rng = np.random.default_rng(5)
    sizes = [5, 0, 9, 1, 12]
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(node_ptr[-1])
    labels = np.concatenate([v0 + _partition(rng, k) for v0, k in zip(node_ptr[:-1], sizes)]).astype(np.int64)
    xw, yw = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    cam = rng.integers(0, 4, size=n)
    emb = rng.standard_normal((n, 6)).astype(np.float32)
    relabel = np.array([1000, -7, 3, 2 ** 31 - 1])
    a, b = to.summaries(labels, node_ptr, xw, yw, cam, emb), to.summaries(labels, node_ptr, xw, yw, relabel[cam], emb)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["n_cams"].max() > 1
    la, _ = to.link(a, node_ptr, 3.0, 1.0)
    lb, _ = to.link(b, node_ptr, 3.0, 1.0)
    for k in ("cluster_track", "node_track", "matched_prev"):
        assert np.array_equal(la[k], lb[k]), k


def _partition(rng, k):
    """A random partition of k nodes in the smallest-id convention (frame-local labels)."""
    group = rng.integers(0, max(k // 2, 1), size=k)
    first = {}
    for v, gq in enumerate(group.tolist()):
        first.setdefault(gq, v)
    return np.array([first[gq] for gq in group.tolist()], dtype=np.int64).reshape(k)


def test_linker_and_summaries_refuse_bad_arguments_before_the_gpu():
    import torch
    from gnn_cca_amd.pipeline import FrameResult
    from gnn_cca_amd.tracking import MAX_FRAME_NODES, FrameLinker, cluster_summaries_raw
    for kw in (dict(max_step=0), dict(max_step=-1.0), dict(max_step=float("inf")), dict(max_step=float("nan")), dict(max_step="1"),
               dict(max_step=1.0, lam=-0.1), dict(max_step=1.0, lam=float("inf")), dict(max_step=1.0, lam=float("nan")),
               dict(max_step=1.0, max_cos=-0.01), dict(max_step=1.0, max_cos=2.5), dict(max_step=1.0, max_cos=float("nan"))):
        with pytest.raises(ValueError):
            FrameLinker(**kw)
    link = FrameLinker(0.5)
    assert (link.max_step, link.lam, link.max_cos, link.needs_embeddings) == (0.5, 1.0, None, True)
    assert not FrameLinker(2, lam=0).needs_embeddings and FrameLinker(2, lam=0, max_cos=2).needs_embeddings
    with pytest.raises(ValueError):
        link(object())
    assert MAX_FRAME_NODES == 4096 and "_ident" in FrameResult.__slots__ and callable(FrameResult.identities)
    n = MAX_FRAME_NODES + 1   # CPU tensors: a refusal that came after the GPU was touched would be a RuntimeError
    with pytest.raises(ValueError):
        cluster_summaries_raw(torch.zeros(n, dtype=torch.int32), [0, n], torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64),
                              torch.zeros(n, dtype=torch.int32))
