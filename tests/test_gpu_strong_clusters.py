"""Clusters without pruning on the MI355X (csrc/strong.cuh: postprocess.strong_clusters, finalize(pruning=False),
FramePipeline(pruning=False), gnncca_post_strong_frames) against oracle/post_oracle.py: `clusters` (scipy's strongly connected
components, labels = the smallest node id), `flows`, and the trigger rule computed on the host.  Every comparison is exact: ORs, integer
counts and a scan in id order, so there is no tolerance to choose."""
import copy
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from oracle import post_oracle as po

pytestmark = pytest.mark.gpu

KEYS = ("labels", "n_clusters", "flow_out", "flow_in", "triggers", "flags")
BAD_RANGE = 2

Z = np.load(os.path.join(GOLDEN_DIR, "post_unpruned.npz"))
NAMES = [str(n) for n in Z["names"]]


def golden(name):
    g = lambda k: Z[f"{name}::{k}"]   # noqa: E731
    n, ei, probs = int(g("n_nodes")), g("edge_index"), g("probs")
    return (n, ei[0], ei[1], (probs >= 0.5).astype(np.int64)), g


# ---- batches and what to expect of them -------------------------------------------------------------------------------------------------
def _batch(frames):
    """frames: list of (n, src, dst[, pred]) with frame-local ids (pred defaults to all ones) -> host arrays and device tensors."""
    node_ptr, edge_ptr, ei, pr = [0], [0], [np.zeros((2, 0), np.int64)], [np.zeros(0, np.int64)]
    for f in frames:
        n, src, dst = f[0], np.asarray(f[1], np.int64), np.asarray(f[2], np.int64)
        v0 = node_ptr[-1]
        ei.append(np.stack([src + v0, dst + v0]).reshape(2, -1))
        pr.append(np.asarray(f[3], np.int64) if len(f) > 3 else np.ones(len(src), np.int64))
        node_ptr.append(v0 + n), edge_ptr.append(edge_ptr[-1] + len(src))
    h = types.SimpleNamespace(ei=np.concatenate(ei, axis=1), pred=np.concatenate(pr), node_ptr=node_ptr, edge_ptr=edge_ptr, n=node_ptr[-1])
    h.ei_dev, h.pred_dev = torch.from_numpy(h.ei).cuda(), torch.from_numpy(h.pred).cuda()
    return h


def _expect(ei, pred, node_ptr, edge_ptr, bad=()):
    """The rule on the host: per frame, the active edges with both ends inside the frame; labels = post_oracle.clusters, flows =
    post_oracle.flows, bit 0 = a flow above 3, bit 1 = a component of more than four.  Frames listed in `bad`: identity, zeros, flag 2."""
    n_all, g = node_ptr[-1], len(node_ptr) - 1
    labels, fo, fi = np.arange(n_all, dtype=np.int32), np.zeros(n_all, np.int32), np.zeros(n_all, np.int32)
    trig, flags, total = np.zeros(g, np.int32), np.zeros(g, np.int32), 0
    for q in range(g):
        v0, v1, k0, k1 = node_ptr[q], node_ptr[q + 1], edge_ptr[q], edge_ptr[q + 1]
        n = v1 - v0
        if q in bad:
            flags[q], total = BAD_RANGE, total + n
            continue
        a, b, p = ei[0, k0:k1], ei[1, k0:k1], pred[k0:k1]
        keep = (p == 1) & (a >= v0) & (a < v1) & (b >= v0) & (b < v1)
        loc = np.stack([a[keep] - v0, b[keep] - v0])
        lab, k = po.clusters(loc, np.ones(loc.shape[1], np.int64), n) if n else (np.zeros(0, np.int64), 0)
        f_out, f_in = po.flows(loc, np.ones(loc.shape[1], np.int64), n) if n else (np.zeros(0), np.zeros(0))
        labels[v0:v1], fo[v0:v1], fi[v0:v1], total = lab + v0, f_out, f_in, total + k
        trig[q] = (1 if n and ((f_out > 3).any() or (f_in > 3).any()) else 0) | (2 if n and np.bincount(lab).max() > 4 else 0)
    return {"labels": labels, "n_clusters": total, "flow_out": fo, "flow_in": fi, "triggers": trig, "flags": flags}


def _host(res):
    out = {k: res[k].cpu().numpy() for k in KEYS}
    out["n_clusters"] = int(out["n_clusters"][0])
    return out


def _assert_equal(got, want, where):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (where, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:6].tolist())


def _run(h, **kw):
    from gnn_cca_amd.postprocess import strong_clusters
    res = strong_clusters(h.ei_dev, h.pred_dev, h.n, h.node_ptr, h.edge_ptr, **kw)
    g = len(h.node_ptr) - 1
    assert res["labels"].dtype == res["flow_out"].dtype == res["flow_in"].dtype == res["triggers"].dtype == res["flags"].dtype == torch.int32
    assert res["labels"].shape == res["flow_out"].shape == res["flow_in"].shape == (h.n,) and res["n_clusters"].shape == (1,)
    assert res["triggers"].shape == res["flags"].shape == (g,) and res["labels"].is_cuda
    assert res["predictions"].dtype == torch.int64 and torch.equal(res["predictions"], h.pred_dev)   # nothing is pruned
    return _host(res)


def _check(h, where, **kw):
    got = _run(h, **kw)
    _assert_equal(got, _expect(h.ei, h.pred, h.node_ptr, h.edge_ptr), where)
    return got


def _random_frame(rng, n, m, active=0.8):
    """n nodes, m random directed edges (self loops and duplicates as they fall), a share of them active."""
    if n == 0:
        return (0, np.zeros(0, np.int64), np.zeros(0, np.int64))
    src, dst = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    return (n, src, dst, (rng.random(m) < active).astype(np.int64))


# ---- the golden frames ------------------------------------------------------------------------------------------------------------------
def test_every_golden_frame_singly_and_as_one_batch():
    frames = [golden(name)[0] for name in NAMES]
    for name, f in zip(NAMES, frames):
        got = _check(_batch([f]), name)
        ids = golden(name)[1]("id_unpruned")
        assert po.same_partition(got["labels"], ids) and got["n_clusters"] == len(set(ids.tolist())), name   # the reference's partition
        # without frame ranges the whole graph is the one frame: the same result
        from gnn_cca_amd.postprocess import strong_clusters
        h = _batch([f])
        _assert_equal(_host(strong_clusters(h.ei_dev, h.pred_dev, h.n)), got, name + " (no ranges)")
    h = _batch(frames)
    got = _check(h, "all golden frames")
    want_ids = np.concatenate([golden(name)[1]("id_unpruned") + 1000 * q for q, name in enumerate(NAMES)])
    assert po.same_partition(got["labels"], want_ids) and got["flags"].sum() == 0
    by_name = dict(zip(NAMES, got["triggers"].tolist()))
    assert by_name["cycle5"] == 2 and by_name["hub_four_out"] == 1 and by_name["cycle3_no_mutual_pair"] == 0 and by_name["nothing_active"] == 0
    assert by_name["two_cycles_share_a_node"] == 2 and all(by_name[n] == 3 for n in NAMES if re.search(r"_s\d+$", n))
    v0 = h.node_ptr[NAMES.index("cycle3_no_mutual_pair")]
    assert (got["labels"][v0:v0 + 12] - v0).tolist() == [0, 1, 0, 3, 0, 5, 6, 7, 8, 9, 10, 11]


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
def test_word_wave_and_block_boundaries():
    rng = np.random.default_rng(3)
    sizes = [1, 2, 31, 32, 33, 64, 65]
    frames = [_random_frame(rng, n, 2 * n) for n in sizes]
    for n, f in zip(sizes, frames):                      # singly: LDS and block size follow the frame (one word / two / three words per row)
        _check(_batch([f]), f"n={n}")
    got = _check(_batch(frames + [_random_frame(rng, 0, 0)]), "sizes 1 .. 65 and an empty frame")
    assert got["flags"].sum() == 0 and (got["triggers"] & 2).any()


def test_a_giant_component_next_to_singletons_at_257():
    rng = np.random.default_rng(12)
    n = 257
    f = (n, rng.integers(0, n, size=400), rng.integers(0, n, size=400))
    got = _check(_batch([(3, [0, 1], [1, 0]), f]), "257")
    sizes = np.bincount(got["labels"][3:] - 3)
    assert sizes.max() >= 60 and (sizes == 1).sum() >= 20       # a giant strongly connected component plus singletons


def test_rings_paths_and_two_cycles_at_1024():
    n = 1024
    v = np.arange(n)
    ring = (n, v, (v + 1) % n)                                                       # one component after the full count of rounds
    path = (n, v[:-1], v[1:])                                                        # weakly connected, all singletons
    pairs = (n, np.concatenate([v[0::2], v[1::2], v[1:-1:2]]), np.concatenate([v[1::2], v[0::2], v[2::2]]))   # 512 two-cycles linked one way
    h = _batch([(5, [0, 1, 2], [1, 2, 0]), ring, path, pairs])
    got = _check(h, "1024")
    assert (got["labels"][5:5 + n] == 5).all()                                       # the frame's first node
    assert got["labels"][5 + n:5 + 2 * n].tolist() == list(range(5 + n, 5 + 2 * n))
    v0 = 5 + 2 * n
    assert (got["labels"][v0:] == v0 + (v // 2) * 2).all()
    assert got["n_clusters"] == 3 + 1 + n + n // 2 and got["triggers"].tolist() == [0, 2, 0, 0] and got["flags"].sum() == 0


def test_frames_of_very_different_sizes_share_one_launch():
    rng = np.random.default_rng(21)
    frames = [_random_frame(rng, 1, 2), _random_frame(rng, 1024, 1500), _random_frame(rng, 32, 80)]   # the LDS is sized by the largest
    got = _check(_batch(frames), "1, 1024, 32")
    alone = _check(_batch([frames[2]]), "32 alone")
    assert np.array_equal(got["labels"][1025:] - 1025, alone["labels"]) and got["triggers"][2] == alone["triggers"][0]


def test_too_wide_a_frame_is_refused_on_the_host_and_flagged_on_the_device():
    from gnn_cca_amd.postprocess import strong_clusters
    rng = np.random.default_rng(8)
    frames = [_random_frame(rng, 20, 60), _random_frame(rng, 1025, 1500), _random_frame(rng, 33, 90)]
    h = _batch(frames)
    with pytest.raises(ValueError, match="at most 1024"):
        strong_clusters(h.ei_dev, h.pred_dev, h.n, h.node_ptr, h.edge_ptr)
    nptr, eptr = torch.tensor(h.node_ptr, dtype=torch.int32).cuda(), torch.tensor(h.edge_ptr, dtype=torch.int32).cuda()
    got = _host(strong_clusters(h.ei_dev, h.pred_dev, h.n, nptr, eptr, max_frame_nodes=1024))
    want = _expect(h.ei, h.pred, h.node_ptr, h.edge_ptr, bad=(1,))
    _assert_equal(got, want, "1025 between 20 and 33")
    assert got["flags"].tolist() == [0, BAD_RANGE, 0] and got["labels"][20:1045].tolist() == list(range(20, 1045))
    assert got["flow_out"][20:1045].sum() == 0 and got["flow_in"][20:1045].sum() == 0 and got["triggers"][1] == 0
    # device offsets without max_frame_nodes: the worst case, the same result
    _assert_equal(_host(strong_clusters(h.ei_dev, h.pred_dev, h.n, nptr, eptr)), want, "default max_frame_nodes")
    # offsets that do not fit at all: the frame is flagged, nothing is written out of range
    for bad_ptr in ([0, 20, 1045, h.n + 7], [0, 1045, 20, h.n]):
        nb = torch.tensor(bad_ptr, dtype=torch.int32).cuda()
        res = _host(strong_clusters(h.ei_dev, h.pred_dev, h.n, nb, eptr, max_frame_nodes=1024))
        assert res["flags"][0] == (0 if bad_ptr[1] == 20 else BAD_RANGE) and res["flags"][1] == BAD_RANGE and res["flags"][2] == BAD_RANGE
        if bad_ptr[1] == 20:
            assert np.array_equal(res["labels"][:20], want["labels"][:20]) and res["triggers"][0] == want["triggers"][0]


# ---- what the edge list may look like ---------------------------------------------------------------------------------------------------
def test_stray_edges_self_loops_duplicates_and_order_change_nothing():
    rng = np.random.default_rng(17)
    sizes = [9, 40, 70]
    clean = []
    for n in sizes:                                       # no self loops, no duplicates
        p = np.unique(rng.integers(0, n, size=(2, 2 * n)), axis=1)
        p = p[:, p[0] != p[1]]
        clean.append((n, p[0], p[1]))
    hc = _batch(clean)
    want = _check(hc, "clean")
    dirty, n_all = [], sum(sizes)
    for q, (n, src, dst) in enumerate(clean):
        v0 = hc.node_ptr[q]
        loops = rng.integers(0, n, size=5)
        dup = rng.integers(0, len(src), size=7)
        # active edges with an end in another frame or outside the batch (batch-global ids, written frame-local: _batch adds v0 again)
        other = (v0 + n) % n_all
        stray = np.array([[v0, other], [other, v0 + 1], [-1, v0 + 2], [n_all + 5, v0 + 3], [1 << 40, v0 + 4], [v0 + 2, -7], [v0 + 3, n_all]]).T - v0
        inactive = rng.integers(0, n, size=(2, 6))         # inactive edges are not edges
        s = np.concatenate([src, loops, src[dup], stray[0], inactive[0]])
        d = np.concatenate([dst, loops, dst[dup], stray[1], inactive[1]])
        p = np.concatenate([np.ones(len(s) - 6, np.int64), np.zeros(6, np.int64)])
        order = rng.permutation(len(s))
        dirty.append((n, s[order], d[order], p[order]))
    got = _check(_batch(dirty), "dirty")                   # the rule itself: flows count a duplicate and a self loop, as scatter_add does
    for k in ("labels", "n_clusters", "flags"):
        assert np.array_equal(got[k], want[k]), k          # the partition is the cleaned list's
    for k in ("flow_out", "flow_in"):                      # five loops and seven duplicates per frame, no stray edge
        assert (got[k] >= want[k]).all() and got[k].sum() == want[k].sum() + len(sizes) * (5 + 7), k


def test_symmetric_predictions_give_prune_and_clusters_results_exactly():
    from gnn_cca_amd.postprocess import prune_and_cluster, strong_clusters
    rng = np.random.default_rng(29)
    frames = []
    for n in (12, 33, 7, 64, 100):
        p = np.unique(np.sort(rng.integers(0, n, size=(2, 2 * n)), axis=0), axis=1)
        p = p[:, p[0] != p[1]]
        src, dst = np.concatenate([p[0], p[1]]), np.concatenate([p[1], p[0]])
        pred = np.tile((rng.random(p.shape[1]) < 0.6).astype(np.int64), 2)     # a pair is active in both directions or in none
        order = np.lexsort((dst, src))
        frames.append((n, src[order], dst[order], pred[order]))
    h = _batch(frames)
    a = strong_clusters(h.ei_dev, h.pred_dev, h.n, h.node_ptr, h.edge_ptr)
    b = prune_and_cluster(h.ei_dev, h.pred_dev, h.n, h.node_ptr, h.edge_ptr)
    assert torch.equal(b["pruned"], h.pred_dev)                                  # nothing to prune
    for k in ("labels", "n_clusters", "flow_out", "flow_in", "triggers"):
        assert torch.equal(a[k], b[k]), k
    assert int(a["triggers"].sum()) > 0 and int(a["flags"].sum()) == 0


def test_a_batch_without_edges_and_two_runs_bitwise_equal():
    none = np.zeros(0, np.int64)
    h = _batch([(7, none, none), (0, none, none), (40, none, none)])
    got = _check(h, "E == 0")
    assert got["n_clusters"] == 47 and got["labels"].tolist() == list(range(47)) and got["triggers"].tolist() == [0, 0, 0]
    from gnn_cca_amd.postprocess import strong_clusters
    rng = np.random.default_rng(31)
    h = _batch([_random_frame(rng, n, 3 * n) for n in (30, 200, 64, 5)])
    runs = [strong_clusters(h.ei_dev, h.pred_dev, h.n, h.node_ptr, h.edge_ptr) for _ in range(2)]
    for k in KEYS:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_raw_entry_with_separate_dirty_buffers_and_finalize_without_pruning():
    """The C entry zeroes its counters itself whether or not they lie back to back (one memset or three), on buffers that held garbage,
    with and without frame ranges; postprocess.finalize(pruning=False) on its result is the reference's ROUNDING on unpruned predictions."""
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.postprocess import finalize, strong_clusters
    frames = [golden(name)[0] for name in NAMES]
    h = _batch(frames)
    want = _expect(h.ei, h.pred, h.node_ptr, h.edge_ptr)
    g, lib, stream = len(NAMES), nat.lib(), torch.cuda.current_stream().cuda_stream
    nptr, eptr = torch.tensor(h.node_ptr, dtype=torch.int32).cuda(), torch.tensor(h.edge_ptr, dtype=torch.int32).cuda()
    bufs = {k: torch.full((m,), 12345, dtype=torch.int32, device="cuda") for k, m in
            (("flow_out", h.n), ("flow_in", h.n), ("labels", h.n), ("n_clusters", 1), ("triggers", g), ("flags", g))}
    st = lib.gnncca_post_strong_frames(h.ei_dev.data_ptr(), h.pred_dev.data_ptr(), h.n, h.ei.shape[1], nptr.data_ptr(), eptr.data_ptr(), g, 32,
                                       bufs["flow_out"].data_ptr(), bufs["flow_in"].data_ptr(), bufs["labels"].data_ptr(),
                                       bufs["n_clusters"].data_ptr(), bufs["triggers"].data_ptr(), bufs["flags"].data_ptr(), stream)
    assert st == nat.OK
    _assert_equal(_host(bufs), want, "separate buffers")
    # no frame ranges: the whole graph is one frame (the first golden frame), one trigger and one flag word
    h0 = _batch(frames[:1])
    one = {k: torch.full((m,), 12345, dtype=torch.int32, device="cuda") for k, m in
           (("flow_out", h0.n), ("flow_in", h0.n), ("labels", h0.n), ("n_clusters", 1), ("triggers", 1), ("flags", 1))}
    st = lib.gnncca_post_strong_frames(h0.ei_dev.data_ptr(), h0.pred_dev.data_ptr(), h0.n, h0.ei.shape[1], None, None, 0, h0.n,
                                       one["flow_out"].data_ptr(), one["flow_in"].data_ptr(), one["labels"].data_ptr(),
                                       one["n_clusters"].data_ptr(), one["triggers"].data_ptr(), one["flags"].data_ptr(), stream)
    assert st == nat.OK
    _assert_equal(_host(one), _expect(h0.ei, h0.pred, h0.node_ptr, h0.edge_ptr), "whole graph")
    # finalize(pruning=False): ROUNDING on the unpruned predictions, the golden's pred_rounded / id_rounded
    probs = torch.from_numpy(np.concatenate([golden(name)[1]("probs") for name in NAMES])).cuda()
    post = strong_clusters(h.ei_dev, h.pred_dev, h.n, h.node_ptr, h.edge_ptr)
    fin = finalize(h.ei_dev, probs, post["predictions"], post["labels"], post["n_clusters"], post["triggers"], h.node_ptr, h.edge_ptr,
                   rounding=True, pruning=False, splitting=False)
    assert fin["frames_finalized"] == [q for q, t in enumerate(want["triggers"]) if t & 1] and len(fin["frames_finalized"]) >= 19
    assert np.array_equal(fin["predictions"].cpu().numpy(), np.concatenate([golden(name)[1]("pred_rounded") for name in NAMES]))
    want_ids = np.concatenate([golden(name)[1]("id_rounded") + 1000 * q for q, name in enumerate(NAMES)])
    assert po.same_partition(fin["labels"].cpu().numpy(), want_ids) and int(fin["n_clusters"].item()) == len(set(want_ids.tolist()))
    none = finalize(h.ei_dev, probs, post["predictions"], post["labels"], post["n_clusters"], post["triggers"], h.node_ptr, h.edge_ptr,
                    rounding=False, pruning=False, splitting=False)
    assert none["frames_finalized"] == [] and none["predictions"] is post["predictions"] and none["labels"] is post["labels"]


def test_the_call_replays_from_a_graph_captured_on_a_side_stream():
    from gnn_cca_amd.postprocess import strong_clusters
    rng = np.random.default_rng(4)
    h = _batch([_random_frame(rng, n, 3 * n) for n in (25, 9, 40, 0, 33)])
    nptr, eptr = torch.tensor(h.node_ptr, dtype=torch.int32).cuda(), torch.tensor(h.edge_ptr, dtype=torch.int32).cuda()
    eager = _host(strong_clusters(h.ei_dev, h.pred_dev, h.n, nptr, eptr, max_frame_nodes=40))   # (also loads the code object before the capture)
    _assert_equal(eager, _expect(h.ei, h.pred, h.node_ptr, h.edge_ptr), "eager")
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):            # one memset node and one kernel node: no workspace, no wait
        res = strong_clusters(h.ei_dev, h.pred_dev, h.n, nptr, eptr, max_frame_nodes=40)
    for k in KEYS:
        res[k].fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(_host(res), eager, "replay")


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------
def _frames(rng, g, lo=0, hi=24, cams=4):
    sizes = rng.integers(lo, hi, size=g)
    if sizes.sum() == 0:
        sizes[0] = 6
    n = int(sizes.sum())
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, 2048)).astype(np.float32),
                reid=rng.standard_normal((n, 256)).astype(np.float32))


@pytest.fixture(scope="module")
def scene():
    """One synthetic batch and a model whose decision boundary lies inside its logits, shared by the pipeline tests (read only)."""
    import bench
    from gnn_cca_amd.graph_build import build_graph_batch
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    f = _frames(np.random.default_rng(1), 24)
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    b = build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    with torch.no_grad():
        med = m(b)["classified_edges"][-1].median()
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= med
        m.load_state_dict(sd)
    return m, f, node, reid


def _call(pipe, scene):
    _, f, node, reid = scene
    r = pipe(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    torch.cuda.synchronize()
    return r


def _frames_of(r):
    b = r.batch
    return [(b.node_ptr[q], b.node_ptr[q + 1], b.edge_ptr[q], b.edge_ptr[q + 1]) for q in range(len(b.node_ptr) - 1)]


def test_pipeline_without_pruning_end_to_end(scene):
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.pipeline import FramePipeline
    r = _call(FramePipeline(scene[0], pruning=False, splitting=False), scene)
    ei, preds, probs = r.batch.edge_index.cpu().numpy(), r.preds.cpu().numpy(), r.probs.cpu().numpy()
    assert torch.equal(r.pruned, r.preds) and 0 < preds.sum() < preds.size          # nothing is pruned
    want = _expect(ei, preds, list(r.batch.node_ptr), list(r.batch.edge_ptr))
    for k in ("labels", "flow_out", "flow_in", "triggers"):
        assert np.array_equal(getattr(r, k).cpu().numpy(), want[k]), k
    assert int(r.n_clusters.item()) == want["n_clusters"]
    fin = r.final()
    assert fin is r.final()
    got_pred, got_lab, total = fin["predictions"].cpu().numpy(), fin["labels"].cpu().numpy(), 0
    for q, (v0, v1, k0, k1) in enumerate(_frames_of(r)):
        _, p, ids, k = po.finalize(ei[:, k0:k1] - v0, None, v1 - v0, rounding_on=True, pruning_on=False, splitting_on=False, probs=probs[k0:k1])
        assert np.array_equal(got_pred[k0:k1], p), q
        assert po.same_partition(got_lab[v0:v1], ids), q
        total += k
    assert int(fin["n_clusters"].item()) == total
    assert fin["frames_finalized"] == [q for q, t in enumerate(want["triggers"]) if t & 1] and len(fin["frames_finalized"]) >= 1
    res = r.final_async().result()
    assert np.array_equal(res["predictions"], got_pred) and np.array_equal(res["labels"], got_lab) and res["n_clusters"] == total
    assert torch.equal(r.evaluate(final=False), evaluate_frames(r.batch, r.preds, r.labels))
    assert torch.equal(r.evaluate(final=True), evaluate_frames(r.batch, fin["predictions"], fin["labels"]))
    # ROUNDING off: nothing can change a frame, the device chain's result is final
    r0 = _call(FramePipeline(scene[0], rounding=False, pruning=False, splitting=False), scene)
    f0 = r0.final()
    assert f0["frames_finalized"] == [] and torch.equal(f0["labels"], r.labels) and torch.equal(f0["predictions"], r.preds)


def test_pipeline_on_a_capped_graph_clusters_the_directed_list(scene):
    from gnn_cca_amd.pipeline import FramePipeline
    r = _call(FramePipeline(scene[0], pruning=False, splitting=False, top_k=2), scene)
    ei, preds = r.batch.edge_index.cpu().numpy(), r.preds.cpu().numpy()
    pairs = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert any((b, a) not in pairs for a, b in pairs)                               # the capped list is directed
    want = _expect(ei, preds, list(r.batch.node_ptr), list(r.batch.edge_ptr))
    for k in ("labels", "flow_out", "flow_in", "triggers"):
        assert np.array_equal(getattr(r, k).cpu().numpy(), want[k]), k
    assert int(r.n_clusters.item()) == want["n_clusters"] and torch.equal(r.pruned, r.preds)


def test_a_pruning_pipeline_next_to_it_gives_what_it_gave_before(scene):
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.postprocess import prune_and_cluster, threshold
    m, f, node, reid = scene
    _call(FramePipeline(m, pruning=False, splitting=False), scene)
    r = _call(FramePipeline(m), scene)
    b = build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    with torch.no_grad():
        out = m(b)
    probs, preds = threshold(out["classified_edges"][-1])
    post = prune_and_cluster(b.edge_index, preds, b.x.shape[0], b.node_ptr_dev, b.edge_ptr_dev)
    assert torch.equal(r.probs, probs) and torch.equal(r.preds, preds) and torch.equal(r.batch.edge_index, b.edge_index)
    for k in ("pruned", "flow_out", "flow_in", "labels", "n_clusters", "triggers"):
        assert torch.equal(getattr(r, k), post[k]), k
    ei, pr = b.edge_index.cpu().numpy(), preds.cpu().numpy()
    want = np.concatenate([po.clusters(ei[:, k0:k1] - v0, po.prune(ei[:, k0:k1] - v0, pr[k0:k1]), v1 - v0)[0] + v0
                           for v0, v1, k0, k1 in _frames_of(r) if v1 > v0])
    assert np.array_equal(r.labels.cpu().numpy(), want)


@pytest.mark.parametrize("n", [64, 65, 256, 257])
def test_block_rungs_a_directed_ring_with_a_chord_as_the_only_frame(n):
    """The sizes at which the launch changes its block (64 / 256 / 1024 threads, one node per thread in the label phase): a single frame, so
    the frame itself sizes the launch.  A ring is one component only after the full count of rounds; the chord gives node 0 a second edge."""
    v = np.arange(n)
    got = _check(_batch([(n, np.append(v, 0), np.append((v + 1) % n, n // 2))]), f"ring of {n}")
    assert got["labels"].tolist() == [0] * n and got["n_clusters"] == 1 and got["triggers"].tolist() == [2] and got["flags"].tolist() == [0]
    assert got["flow_out"][0] == 2 and got["flow_in"][n // 2] == 2 and got["flow_out"].sum() == n + 1
