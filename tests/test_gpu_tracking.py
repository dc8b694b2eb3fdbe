"""gnn_cca_amd.tracking on the GPU against tests/tracking_oracle.py: the cluster summaries bit for bit (the sum orders are part of the
contract), the frame-to-frame links and track ids exactly, the state carried across calls, and both through FramePipeline results.
The feature has no counterpart in the reference, so the oracle is the numpy restatement of the documented rules."""
import copy

import numpy as np
import pytest
import torch

import tracking_oracle as to

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 7, 64, 65, 0, 257, 300)   # one wave / two waves / the 256-thread kernel; an empty frame; sizes that are no power of two


def _partition(rng, k, mode):
    """Frame-local labels of k nodes in the smallest-id convention."""
    if mode == "singletons":
        return np.arange(k, dtype=np.int64)
    if mode == "one":
        return np.zeros(k, dtype=np.int64)
    group = rng.integers(0, max(k // 3, 1), size=k)
    first = {}
    for v, q in enumerate(group.tolist()):
        first.setdefault(q, v)
    return np.array([first[q] for q in group.tolist()], dtype=np.int64).reshape(k)


def _batch(seed, sizes, r, mode="random"):
    rng = np.random.default_rng(seed)
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(node_ptr[-1])
    labels = np.concatenate([v0 + _partition(rng, k, mode) for v0, k in zip(node_ptr[:-1], sizes)]).astype(np.int32)
    cams = np.array([3, -12, 70000, 0, 2 ** 31 - 1, 5])
    return dict(labels=labels, node_ptr=node_ptr, xw=rng.uniform(-30, 30, n), yw=rng.uniform(-30, 30, n), cam=cams[rng.integers(0, 6, size=n)].astype(np.int32),
                emb=rng.standard_normal((n, r)).astype(np.float32) if r else None)


def _run(b):
    from gnn_cca_amd.tracking import cluster_summaries_raw
    dev = "cuda"
    s = cluster_summaries_raw(torch.from_numpy(b["labels"]).to(dev), b["node_ptr"].tolist(), torch.from_numpy(b["xw"]).to(dev),
                              torch.from_numpy(b["yw"]).to(dev), torch.from_numpy(b["cam"]).to(dev),
                              torch.from_numpy(b["emb"]).to(dev) if b["emb"] is not None else None)
    torch.cuda.synchronize()
    return s


def _same_summaries(s, want):
    for k in ("count", "rank", "size", "n_cams", "pos", "emb"):
        got = getattr(s, k).cpu()
        ref = torch.from_numpy(want[k])
        assert got.dtype == ref.dtype and got.shape == ref.shape, k
        assert torch.equal(got, ref), k


@pytest.mark.parametrize("r,mode", [(0, "random"), (1, "random"), (70, "random"), (257, "random"), (70, "singletons"), (70, "one")])
def test_summaries_equal_the_numpy_loops_bit_for_bit(r, mode):
    b = _batch(10 + r, SIZES, r, mode)
    want = to.summaries(b["labels"], b["node_ptr"], b["xw"], b["yw"], b["cam"], b["emb"])
    s = _run(b)
    _same_summaries(s, want)
    if mode == "random":
        assert want["n_cams"].max() > 1 and want["size"].max() > 3 and 1 < want["count"][-1] < SIZES[-1]
    assert want["count"][5] == 0 and want["count"].min() == 0


def test_summaries_of_a_4096_node_frame():
    b = _batch(77, (3, 4096, 5), 8)
    want = to.summaries(b["labels"], b["node_ptr"], b["xw"], b["yw"], b["cam"], b["emb"])
    _same_summaries(_run(b), want)
    assert want["count"][1] > 64


def test_a_4097_node_frame_is_refused_before_any_launch():
    from gnn_cca_amd.tracking import cluster_summaries_raw
    n = 4097
    z32 = torch.zeros(n, dtype=torch.int32, device="cuda")
    z64 = torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        cluster_summaries_raw(z32, [0, n], z64, z64, z32)
    with pytest.raises(ValueError):
        cluster_summaries_raw(z32, torch.tensor([0, n], dtype=torch.int32, device="cuda"), z64, z64, z32)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["outside", "not_a_root"])
def test_a_frame_with_a_bad_label_is_refused_alone(kind):
    b = _batch(5, (9, 70, 12), 5)
    good = to.summaries(b["labels"], b["node_ptr"], b["xw"], b["yw"], b["cam"], b["emb"])
    v = 9 + 33
    if kind == "outside":
        b["labels"][v] = 9 + 70 + 2       # a node of the next frame
    else:
        other = next(u for u in range(9, 9 + 70) if b["labels"][u] != u and b["labels"][u] != b["labels"][v])
        b["labels"][v] = other             # inside the frame, but `other` is not its own label
    s = _run(b)
    want = to.summaries(b["labels"], b["node_ptr"], b["xw"], b["yw"], b["cam"], b["emb"])
    _same_summaries(s, want)
    assert s.count.tolist() == [int(good["count"][0]), -1, int(good["count"][2])]
    for k in ("size", "n_cams", "pos", "emb"):
        got = getattr(s, k).cpu().numpy()
        assert not got[9:79].any(), k
        assert np.array_equal(got[:9], good[k][:9]) and np.array_equal(got[79:], good[k][79:]), k
    assert (s.rank.cpu().numpy()[9:79] == -1).all()


# ---- linking ---------------------------------------------------------------------------------------------------------------------
def _upload(summ, lo=0, hi=None):
    """Frames lo .. hi of an oracle sequence as a ClusterSummaries on the device."""
    from gnn_cca_amd.tracking import ClusterSummaries
    ptr = summ["node_ptr"]
    hi = len(ptr) - 1 if hi is None else hi
    v0, v1 = int(ptr[lo]), int(ptr[hi])
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    local = (ptr[lo:hi + 1] - v0)
    return ClusterSummaries(t(summ["count"][lo:hi]), t(summ["rank"][v0:v1]), t(summ["size"][v0:v1]), t(summ["n_cams"][v0:v1]),
                            t(summ["pos"][v0:v1]), t(summ["emb"][v0:v1]), local.tolist(), t(local.astype(np.int32)))


def _same_tracks(t, want):
    torch.cuda.synchronize()
    assert torch.equal(t.cluster_track.cpu(), torch.from_numpy(want["cluster_track"]))
    assert torch.equal(t.node_track.cpu(), torch.from_numpy(want["node_track"]))
    assert torch.equal(t.matched_prev.cpu(), torch.from_numpy(want["matched_prev"]))
    assert t.next_id.dtype == torch.int64 and int(t.next_id.item()) == want["next_id"]


def _assert_margins(summ, max_step, lam, max_cos):
    """The precondition of exact equality when the cosine takes part: the kernel's float64 dots differ from the oracle's in summation
    order only (~R * 1e-16), so no decision of the oracle may hang on less than 1e-9."""
    gap_cost, gap_d, gap_cos = to.margins(summ, summ["node_ptr"], max_step, lam, max_cos)
    assert gap_cost > 1e-9 and gap_d > 1e-9 and gap_cos > 1e-9, (gap_cost, gap_d, gap_cos)


LINK_CASES = [  # g, persons, seed, lam, max_cos, empty
    (1, 70, 1, 1.0, None, ()), (2, 70, 2, 1.0, None, ()), (9, 70, 3, 1.0, None, (4,)), (9, 70, 4, 0.5, 0.05, ()),
    (1, 70, 1, 0.0, None, ()), (2, 70, 2, 0.0, None, ()), (9, 70, 3, 0.0, None, (4,)), (9, 20, 6, 0.0, 1.0, (0,))]


@pytest.mark.parametrize("g,persons,seed,lam,max_cos,empty", LINK_CASES)
def test_links_equal_the_oracle(g, persons, seed, lam, max_cos, empty):
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(seed)
    summ = to.walk_sequence(rng, g, persons, 16, noise=0.3, p_leave=0.04, p_enter=0.6, arena=12.0, empty=empty)
    max_step = 1.0
    if lam != 0 or max_cos is not None:
        _assert_margins(summ, max_step, lam, max_cos)
    want, _ = to.link(summ, summ["node_ptr"], max_step, lam, max_cos)
    t = FrameLinker(max_step, lam=lam, max_cos=max_cos)(_upload(summ))
    _same_tracks(t, want)
    assert summ["count"].max() > 64 or persons < 64   # past the 64-lane boundary
    if g > 1:
        assert (want["matched_prev"] >= 0).any() and (want["matched_prev"][summ["node_ptr"][1]:] < 0).any()


def test_exact_ties_on_a_lattice_resolve_as_the_rule_says():
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(8)
    summ = to.walk_sequence(rng, 5, 40, 4, p_leave=0.1, p_enter=0.5, arena=9.0, lattice=True)
    want, _ = to.link(summ, summ["node_ptr"], 5.0, 0.0)
    ties = 0   # the case is about ties: count the rows whose two best admissible costs are EQUAL, and the pairs exactly on the gate
    on_gate = 0
    ptr = summ["node_ptr"]
    for q in range(1, 5):
        d, _, cost, ok = to.pair_tables(summ["pos"][ptr[q]:ptr[q + 1]], None, summ["pos"][ptr[q - 1]:ptr[q]], None, 5.0, lam=0.0)
        on_gate += int((d == 5.0).sum())
        for row in np.where(ok, cost, np.inf):
            fin = np.sort(row[np.isfinite(row)])
            ties += int(len(fin) >= 2 and fin[0] == fin[1])
    assert ties > 0 and on_gate > 0
    _same_tracks(FrameLinker(5.0, lam=0.0)(_upload(summ)), want)


def test_links_of_two_4096_cluster_frames():
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(11)
    k = 4096
    p0 = rng.uniform(0, 150, size=(k, 2))
    keep = rng.permutation(k)
    p1 = p0[keep] + rng.normal(0, 0.2, size=(k, 2))
    p1[::17] += 40.0   # some leave, others appear
    summ = dict(count=np.array([k, k], np.int32), rank=np.concatenate([np.arange(k), np.arange(k)]).astype(np.int32),
                size=np.ones(2 * k, np.int32), n_cams=np.ones(2 * k, np.int32), pos=np.concatenate([p0, p1]),
                emb=np.zeros((2 * k, 0), np.float32), node_ptr=np.array([0, k, 2 * k], np.int64))
    want, _ = to.link(summ, summ["node_ptr"], 1.0, 0.0)
    assert 0.5 * k < (want["matched_prev"] >= 0).sum() < k
    _same_tracks(FrameLinker(1.0, lam=0.0)(_upload(summ)), want)


def test_the_state_carries_across_batches():
    from gnn_cca_amd.tracking import FrameLinker
    rng = np.random.default_rng(21)
    summ = to.walk_sequence(rng, 12, 25, 16, noise=0.3, p_leave=0.1, p_enter=0.5, arena=8.0, empty=(7,))
    _assert_margins(summ, 1.0, 1.0, None)
    want, _ = to.link(summ, summ["node_ptr"], 1.0, 1.0)
    link = FrameLinker(1.0, lam=1.0)
    whole = link(_upload(summ))
    _same_tracks(whole, want)
    link.reset()
    parts = [link(_upload(summ, lo, hi)) for lo, hi in ((0, 5), (5, 6), (6, 12))]
    torch.cuda.synchronize()
    for k in ("cluster_track", "node_track", "matched_prev"):
        assert torch.equal(torch.cat([getattr(p, k) for p in parts]), getattr(whole, k)), k
    assert torch.equal(parts[-1].next_id, whole.next_id) and int(parts[0].next_id.item()) < int(parts[-1].next_id.item())
    # an empty batch leaves the state alone; another number of appearance columns is refused until reset()
    none = link(_upload(summ, 3, 3))
    assert none.cluster_track.numel() == 0 and torch.equal(none.next_id, whole.next_id)
    short = to.walk_sequence(np.random.default_rng(1), 2, 5, 8)
    with pytest.raises(ValueError):
        link(_upload(short))
    link.reset()
    again = link(_upload(summ, 0, 5))
    torch.cuda.synchronize()
    assert torch.equal(again.cluster_track, parts[0].cluster_track) and int(again.cluster_track[0].item()) == 0
    assert torch.equal(again.next_id, parts[0].next_id)


# ---- through the pipeline --------------------------------------------------------------------------------------------------------
def _frames(rng, g, lo=0, hi=24, cams=4):
    sizes = rng.integers(lo, hi, size=g)
    if sizes.sum() == 0:
        sizes[0] = 6
    n = int(sizes.sum())
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, 2048)).astype(np.float32),
                reid=rng.standard_normal((n, 256)).astype(np.float32))


@pytest.mark.parametrize("cap", [None, dict(top_k=3, symmetric="union")])
def test_identities_of_a_pipeline_result(cap):
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.tracking import FrameLinker, cluster_summaries_raw
    rng = np.random.default_rng(31)
    f = _frames(rng, 7)
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    pipe = FramePipeline(m, **(cap or {}))
    args = (f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    r = pipe(*args)
    with torch.no_grad():   # put the decision boundary inside the logits so that the partition is neither trivial one
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= r.outputs["classified_edges"][-1].median()
        m.load_state_dict(sd)
    r = pipe(*args)
    assert (r._d2h is None) == (cap is not None)   # the one-call path, and the step-by-step path a symmetric cap takes
    xw, yw = torch.from_numpy(f["xw"]).cuda(), torch.from_numpy(f["yw"]).cuda()
    cam = torch.from_numpy(f["id_cam"].astype(np.int32)).cuda()
    fin = r.final()
    for final, labels in ((True, fin["labels"]), (False, r.labels)):
        s = r.identities(final=final)
        assert s is r.identities(final=final)
        raw = cluster_summaries_raw(labels, r.batch.node_ptr, xw, yw, cam, r.batch.reid_embeds)
        torch.cuda.synchronize()
        for k in ("count", "rank", "size", "n_cams", "pos", "emb"):
            assert torch.equal(getattr(s, k), getattr(raw, k)), (final, k)
        want = to.summaries(labels.cpu().numpy(), r.batch.node_ptr, f["xw"], f["yw"], f["id_cam"], r.batch.reid_embeds.cpu().numpy())
        _same_summaries(s, want)
    assert r.identities() is not r.identities(final=False)
    s = r.identities()
    assert 0 < int(s.count.sum().item()) < f["n"] and int(s.count.min().item()) >= 0
    t = FrameLinker(max_step=3.0)(r)
    torch.cuda.synchronize()
    track, lab = t.node_track.cpu().numpy(), fin["labels"].cpu().numpy()
    assert (track >= 0).all() and int(t.next_id.item()) == len(set(track.tolist()))
    for q in range(len(f["sizes"])):
        v0, v1 = r.batch.node_ptr[q], r.batch.node_ptr[q + 1]
        same_track = track[v0:v1, None] == track[None, v0:v1]
        same_label = lab[v0:v1, None] == lab[None, v0:v1]
        assert np.array_equal(same_track, same_label), q
