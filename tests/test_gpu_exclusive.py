"""Camera-exclusive identity clusters on the MI355X (csrc/exclusive.cuh: postprocess.exclusive_clusters, FrameResult.exclusive,
gnncca_post_exclusive_frames) against the sequential walk of tests/exclusive_oracle.py.  Every comparison is exact: the rule compares
float32 values and nothing else, so there is no tolerance to choose."""
import copy
import types

import numpy as np
import pytest
import torch

import exclusive_oracle as oracle

pytestmark = pytest.mark.gpu

KEYS = ("labels", "predictions", "cut", "n_clusters", "flags")


# ---- hand batches ---------------------------------------------------------------------------------------------------------------------
def _hand_batch(frames):
    """frames: list of (n, src, dst, scores, cam) with frame-local ids -> the device tensors exclusive_clusters takes, and host copies."""
    node_ptr, edge_ptr, ei, sc, cam = [0], [0], [np.zeros((2, 0), np.int64)], [np.zeros(0, np.float32)], [np.zeros(0, np.int32)]
    for n, src, dst, s, c in frames:
        v0 = node_ptr[-1]
        assert len(c) == n and len(src) == len(dst) == len(s)
        ei.append(np.stack([np.asarray(src, np.int64) + v0, np.asarray(dst, np.int64) + v0]).reshape(2, -1))
        sc.append(np.asarray(s, np.float32)), cam.append(np.asarray(c, np.int32))
        node_ptr.append(v0 + n), edge_ptr.append(edge_ptr[-1] + len(src))
    h = types.SimpleNamespace(ei=np.concatenate(ei, axis=1), scores=np.concatenate(sc), cam=np.concatenate(cam), node_ptr=node_ptr,
                              edge_ptr=edge_ptr, n=node_ptr[-1])
    h.ei_dev, h.scores_dev, h.cam_dev = torch.from_numpy(h.ei).cuda(), torch.from_numpy(h.scores).cuda(), torch.from_numpy(h.cam).cuda()
    return h


def _host(res):
    out = {k: res[k].cpu().numpy() for k in KEYS}
    out["n_clusters"] = int(out["n_clusters"][0])
    return out


def _run(h, th):
    from gnn_cca_amd.postprocess import exclusive_clusters
    res = exclusive_clusters(h.ei_dev, h.scores_dev, h.cam_dev, h.n, h.node_ptr, h.edge_ptr, at=th)
    assert res["predictions"].dtype == torch.int64 and res["labels"].dtype == torch.int32 and res["n_clusters"].shape == (1,)
    assert res["cut"].shape == res["flags"].shape == (len(h.node_ptr) - 1,) and res["labels"].is_cuda
    return _host(res)


def _assert_equal(got, want, where):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (where, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:6].tolist())


def _check(h, th, where):
    got = _run(h, th)
    want = oracle.exclusive_oracle(h.ei, h.scores, h.cam, h.node_ptr, h.edge_ptr, th)
    _assert_equal(got, want, where)
    assert oracle.one_per_camera(got["labels"], h.cam), where
    return got


def _pairs_frame(n, pairs, weights, cam):
    src, dst, scores = oracle.mutual_pairs(n, pairs, weights)
    return (n, src, dst, scores, cam)


def _random_frame(rng, n, cams, n_pairs, coarse=False, shuffle=False):
    """n nodes on `cams` cameras, about n_pairs random cross-camera pairs, both directions with scores of their own."""
    cam = rng.integers(0, cams, size=n).astype(np.int32)
    if n < 2 or n_pairs == 0:
        return (n, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), cam)
    p = rng.integers(0, n, size=(2, n_pairs))
    p = p[:, cam[p[0]] != cam[p[1]]]
    p = np.unique(np.sort(p, axis=0), axis=1)
    src, dst = np.concatenate([p[0], p[1]]), np.concatenate([p[1], p[0]])
    order = rng.permutation(len(src)) if shuffle else np.lexsort((dst, src))
    e = len(src)
    scores = (rng.integers(1, 9, size=e) / 8.0 if coarse else rng.random(e)).astype(np.float32)
    return (n, src[order], dst[order], scores, cam)


HAND = [
    # two triangles joined by one strong cross pair whose cameras clash with the rest: {0}, {1, 2, 3}, {4, 5}
    ((6, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)], [0.6, 0.6, 0.8, 0.7, 0.6, 0.6, 0.9], [0, 1, 2, 0, 1, 2]), [0, 1, 1, 1, 4, 4], 4),
    # a path with increasing weights on nine cameras: one cluster after n - 1 rounds
    ((9, [(v, v + 1) for v in range(8)], [0.55 + 0.05 * v for v in range(8)], list(range(9))), [0] * 9, 0),
    # a star whose leaves share a camera: only the heaviest leaf joins
    ((5, [(0, 1), (0, 2), (0, 3), (0, 4)], [0.6, 0.9, 0.7, 0.8], [0, 1, 1, 1, 1]), [0, 1, 0, 3, 4], 3),
    # all weights equal: the tie rule decides everything
    ((4, [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2)], [0.75] * 5, [0, 1, 0, 1]), [0, 0, 2, 2], 3),
]


def test_hand_cases_with_the_answer_written_out():
    h = _hand_batch([_pairs_frame(*case) for case, _, _ in HAND])
    got = _check(h, 0.5, "hand cases")
    for f, (_, labels, cut) in enumerate(HAND):
        v0 = h.node_ptr[f]
        assert (got["labels"][v0:h.node_ptr[f + 1]] - v0).tolist() == labels and got["cut"][f] == cut, f
    assert got["flags"].tolist() == [0, 0, 0, 0] and got["n_clusters"] == 3 + 1 + 4 + 2


def test_wave_and_block_boundaries_inside_frames_and_degenerate_frames():
    rng = np.random.default_rng(3)
    sizes = [1, 2, 63, 64, 65, 255, 256, 257]
    frames = [_random_frame(rng, n, 5, 3 * n, coarse=(k % 2 == 0), shuffle=(k % 3 == 0)) for k, n in enumerate(sizes)]
    h = _hand_batch(frames)
    got = _check(h, 0.4, "sizes 1 .. 257")
    assert (got["cut"] > 0).sum() >= 3 and got["flags"].sum() == 0
    # a frame with no edges between frames with edges, an empty frame, a frame on one camera
    none = np.zeros(0, np.int64)
    lone = (7, none, none, np.zeros(0, np.float32), np.arange(7) % 3)
    empty = (0, none, none, np.zeros(0, np.float32), np.zeros(0, np.int32))
    h = _hand_batch([frames[2], lone, empty, frames[4], lone])
    got = _check(h, 0.4, "edgeless frames")
    assert got["labels"][63:70].tolist() == list(range(63, 70)) and got["cut"][1] == got["cut"][2] == got["cut"][4] == 0
    # no edge in the whole batch: nothing but the per-frame launch
    h = _hand_batch([lone, empty, lone])
    got = _check(h, 0.5, "E == 0")
    assert got["n_clusters"] == 14 and got["labels"].tolist() == list(range(14))


@pytest.mark.parametrize("n", [64, 65])
def test_block_rungs_a_ring_of_mutual_pairs_as_the_only_frame(n):
    """The size at which the launch changes its block (one wave up to a capacity of 64, 256 threads above): a single frame, so the frame
    itself sizes the launch.  Cameras v % 4: a cluster can hold four neighbours of the ring at most, and at 65 the closing pair (64, 0)
    joins two detections of camera 0."""
    pairs = [(v, (v + 1) % n) if v + 1 < n else (0, v) for v in range(n)]
    weights = [0.55 + ((7 * v) % 16) / 64.0 for v in range(n)]                     # exact in fp32, ties among them
    got = _check(_hand_batch([_pairs_frame(n, pairs, weights, np.arange(n) % 4)]), 0.5, f"ring of {n}")
    assert got["flags"].tolist() == [0] and got["cut"][0] > 0 and n // 4 <= got["n_clusters"] < n
    assert np.bincount(got["labels"]).max() <= 4


def test_edge_cases_of_the_rule():
    # camera ids 0 and 63 in one cluster (mask bit 63), next to a pair that shares camera 63
    f0 = _pairs_frame(4, [(0, 1), (1, 2), (2, 3)], [0.9, 0.8, 0.7], [0, 63, 63, 5])
    # a one-directional edge, a NaN score, a score exactly at the threshold and one ulp below it
    below = np.nextafter(np.float32(0.75), np.float32(0))
    f1 = (5, [0, 1, 1, 2, 2, 3, 0, 3, 4], [1, 0, 2, 1, 3, 2, 3, 4, 3], np.array([0.75, 0.75, 0.75, below, np.nan, 0.9, 0.9, 0.75, 0.8], np.float32),
          [0, 1, 2, 3, 4])
    # same-camera edges in a raw list: never admissible, whatever they weigh
    f2 = _pairs_frame(3, [(0, 1), (1, 2), (0, 2)], [0.99, 0.8, 0.9], [2, 2, 4])
    h = _hand_batch([f0, f1, f2])
    got = _check(h, 0.75, "rule edges")
    assert got["labels"].tolist() == [0, 0, 2, 3, 4, 4, 6, 7, 7, 9, 10, 9]
    assert got["predictions"][h.edge_ptr[1]:h.edge_ptr[2]].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 1]
    assert got["cut"].tolist() == [1, 0, 2] and got["flags"].tolist() == [0, 0, 0]


def test_the_lds_maximum_and_hundreds_of_rounds():
    rng = np.random.default_rng(9)
    big = _random_frame(rng, 4096, 8, 6000)                       # one 4096-node frame: 80 KiB of LDS
    h = _hand_batch([big])
    got = _check(h, 0.3, "4096 nodes")
    assert got["cut"][0] > 0 and 1000 < got["n_clusters"] < 4096
    # a 300-node path with increasing weights: on two alternating cameras (pairs form back to front, one per round) and on 64
    n = 300
    pairs, weights = [(v, v + 1) for v in range(n - 1)], [0.35 + 0.002 * v for v in range(n - 1)]
    h = _hand_batch([_pairs_frame(n, pairs, weights, [v % 2 for v in range(n)]), _pairs_frame(n, pairs, weights, [v % 64 for v in range(n)])])
    got = _check(h, 0.3, "paths")
    assert got["labels"][:n].tolist() == [v - (v % 2) for v in range(n)] and got["cut"][0] == 149
    assert np.unique(got["labels"][n:], return_counts=True)[1].max() == 64


def test_two_runs_give_the_same_bits_and_a_frame_does_not_depend_on_its_batch():
    rng = np.random.default_rng(21)
    frames = [_random_frame(rng, n, 4, 4 * n, coarse=True, shuffle=(k % 2 == 1)) for k, n in enumerate([30, 7, 70, 2, 130, 18])]
    h = _hand_batch(frames)
    first, second = _check(h, 0.5, "whole batch"), _run(h, 0.5)
    _assert_equal(first, second, "second run")
    assert (first["cut"] > 0).sum() >= 3
    rev = _hand_batch(frames[::-1])
    got_rev = _run(rev, 0.5)
    g = len(frames)
    for f in range(g):
        v0, v1, k0, k1 = h.node_ptr[f], h.node_ptr[f + 1], h.edge_ptr[f], h.edge_ptr[f + 1]
        alone = _run(_hand_batch([frames[f]]), 0.5)
        r = g - 1 - f
        for got, w0, e0, cut in ((alone, 0, 0, alone["cut"][0]), (got_rev, rev.node_ptr[r], rev.edge_ptr[r], got_rev["cut"][r])):
            assert np.array_equal(got["labels"][w0:w0 + v1 - v0] - w0, first["labels"][v0:v1] - v0), f
            assert np.array_equal(got["predictions"][e0:e0 + k1 - k0], first["predictions"][k0:k1]) and cut == first["cut"][f], f
    assert got_rev["n_clusters"] == first["n_clusters"]


# ---- the raw entry point: capture, refusals on the device ----------------------------------------------------------------------------------
def _raw(h, th, cam_dev=None, max_n=None):
    """gnncca_post_exclusive_frames on preallocated buffers -> (call, outputs): call() enqueues on the current stream."""
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.frames import _raw_stream
    lib = nat.lib()
    dev = h.ei_dev.device
    g, e = len(h.node_ptr) - 1, h.ei.shape[1]
    nptr, eptr = torch.tensor(h.node_ptr, dtype=torch.int32).cuda(), torch.tensor(h.edge_ptr, dtype=torch.int32).cuda()
    cam_dev = h.cam_dev if cam_dev is None else cam_dev
    max_n = int(np.diff(h.node_ptr).max()) if max_n is None else max_n
    out = {"predictions": torch.empty(e, dtype=torch.int64, device=dev), "labels": torch.empty(h.n, dtype=torch.int32, device=dev),
           "n_clusters": torch.empty(1, dtype=torch.int32, device=dev), "cut": torch.empty(g, dtype=torch.int32, device=dev),
           "flags": torch.empty(g, dtype=torch.int32, device=dev)}
    nbytes = lib.gnncca_post_exclusive_workspace_bytes(h.n, e, g)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        st = lib.gnncca_post_exclusive_frames(h.ei_dev.data_ptr(), h.scores_dev.data_ptr(), h.n, e, cam_dev.data_ptr(), nptr.data_ptr(),
                                              eptr.data_ptr(), g, max_n, th, out["predictions"].data_ptr(), out["labels"].data_ptr(),
                                              out["n_clusters"].data_ptr(), out["cut"].data_ptr(), out["flags"].data_ptr(), ws.data_ptr(), nbytes,
                                              _raw_stream(dev))
        assert st == nat.OK, st
    return call, out, (nptr, eptr, ws, cam_dev)


def test_the_entry_point_replays_from_a_graph():
    rng = np.random.default_rng(4)
    h = _hand_batch([_random_frame(rng, n, 4, 4 * n, coarse=True) for n in (25, 9, 40, 0, 33)])
    call, out, keep = _raw(h, 0.5)
    call()                                        # warm-up: the code object is loaded before the capture
    torch.cuda.synchronize()
    eager = _host(out)
    _assert_equal(eager, oracle.exclusive_oracle(h.ei, h.scores, h.cam, h.node_ptr, h.edge_ptr, 0.5), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                 # one linear stream: plan, plan finish, prepare, clusters
        call()
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(_host(out), eager, "replay")


def test_refusals_on_the_device_and_before_any_launch():
    from gnn_cca_amd.postprocess import exclusive_clusters
    rng = np.random.default_rng(8)
    frames = [_random_frame(rng, n, 4, 4 * n) for n in (12, 9, 28)]
    h = _hand_batch(frames)
    good = _run(h, 0.5)
    # a camera id of 64 in frame 1 reaches the kernel through the raw function: that frame is refused, its neighbours are not
    cam = h.cam.copy()
    cam[h.node_ptr[1] + 3] = 64
    call, out, keep = _raw(h, 0.5, cam_dev=torch.from_numpy(cam).cuda())
    call()
    got = _host(out)
    _assert_equal(got, oracle.exclusive_oracle(h.ei, h.scores, cam, h.node_ptr, h.edge_ptr, 0.5), "camera 64")
    assert got["flags"].tolist() == [0, 1, 0]
    v0, v1, k0, k1 = h.node_ptr[1], h.node_ptr[2], h.edge_ptr[1], h.edge_ptr[2]
    assert got["labels"][v0:v1].tolist() == list(range(v0, v1)) and not got["predictions"][k0:k1].any()
    for a, b in ((0, v0), (v1, h.n)):
        assert np.array_equal(got["labels"][a:b], good["labels"][a:b])
    assert np.array_equal(got["predictions"][:k0], good["predictions"][:k0]) and np.array_equal(got["predictions"][k1:], good["predictions"][k1:])
    assert got["cut"][0] == good["cut"][0] and got["cut"][2] == good["cut"][2]
    # a frame that does not fit the LDS regions sized from the stated maximum (16): refused on the device, that frame alone
    call, out, keep = _raw(h, 0.5, max_n=16)
    call()
    got = _host(out)
    assert got["flags"].tolist() == [0, 0, 2] and got["labels"][h.node_ptr[2]:].tolist() == list(range(h.node_ptr[2], h.n))
    assert np.array_equal(got["labels"][:h.node_ptr[2]], good["labels"][:h.node_ptr[2]]) and not got["predictions"][h.edge_ptr[2]:].any()
    # more than 4096 detections in a frame: ValueError before any launch
    n = 4097
    none = torch.zeros((2, 0), dtype=torch.int64).cuda()
    with pytest.raises(ValueError, match="at most 4096"):
        exclusive_clusters(none, torch.zeros(0).cuda(), torch.zeros(n, dtype=torch.int32).cuda(), n, [0, n], [0, 0])


# ---- random frames through build_graph_batch + the bias-shifted synthetic model ---------------------------------------------------------
def _frames(rng, sizes, cams, node_dim=2048, reid_dim=256):
    sizes = np.asarray(sizes)
    n, g = int(sizes.sum()), len(sizes)
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, node_dim)).astype(np.float32),
                reid=rng.standard_normal((n, reid_dim)).astype(np.float32))


def _args(f):
    return f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"]


def _shift_bias(m, b):
    """Put the decision boundary inside the logits so that decisions vary (as tests/test_gpu_evaluation.py does)."""
    with torch.no_grad():
        med = m(b)["classified_edges"][-1].median()
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= med
        m.load_state_dict(sd)


def _oracle_of(r, th):
    b = r.batch
    return oracle.exclusive_oracle(b.edge_index.cpu().numpy(), r.probs.cpu().numpy(), b.cam_dev.cpu().numpy(), b.node_ptr, b.edge_ptr, th)


@pytest.fixture(scope="module")
def synthetic():
    """Per camera count (3, 4, 6) one batch of 24 frames -- six dense ones of 20-40 detections, ten of 4-10, eight of 2-4 -- and a model
    whose decisions vary; the results of FramePipeline at 0.3 / 0.5 / 0.7 with the oracle's answer for each."""
    import bench
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    rng = np.random.default_rng(17)
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    data = {}
    for cams in (3, 4, 6):
        sizes = np.concatenate([rng.integers(20, 41, size=6), rng.integers(4, 11, size=10), rng.integers(2, 5, size=8)])
        f = _frames(rng, rng.permutation(sizes), cams)
        data[cams] = (f, torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda())
    f, node, reid = data[4]
    _shift_bias(m, build_graph_batch(*_args(f), node, reid))
    runs = []
    for cams, (f, node, reid) in data.items():
        for th in (0.3, 0.5, 0.7):
            r = FramePipeline(m, threshold=th)(*_args(f), node, reid)
            runs.append(types.SimpleNamespace(cams=cams, th=th, r=r, f=f, want=_oracle_of(r, th)))
    return types.SimpleNamespace(model=m, data=data, runs=runs)


def test_pipeline_results_equal_the_oracle_and_nothing_else_moves(synthetic):
    cut_frames = legal_frames = 0
    for run in synthetic.runs:
        r, where = run.r, (run.cams, run.th)
        assert (r._d2h is not None) == (run.th == 0.5)                  # both paths: the one-call chain at 0.5, step by step otherwise
        fin = r.final()
        before = [t.clone() for t in (r.pruned, r.labels, r.triggers, r.probs, r.n_clusters, fin["predictions"], fin["labels"])]
        ex = r.exclusive()
        assert r.exclusive() is ex and sorted(ex) == sorted(KEYS)
        got = _host(ex)
        _assert_equal(got, run.want, where)
        assert oracle.one_per_camera(got["labels"], run.f["id_cam"]), where
        fin2 = r.final()
        after = (r.pruned, r.labels, r.triggers, r.probs, r.n_clusters, fin2["predictions"], fin2["labels"])
        assert fin2 is fin and all(torch.equal(a, b) for a, b in zip(before, after)), where
        # frames that needed no cut: the device chain's partition and pruned predictions, exactly
        labels, pruned = r.labels.cpu().numpy(), r.pruned.cpu().numpy()
        b = r.batch
        for g in range(len(b.node_ptr) - 1):
            if got["cut"][g] == 0:
                legal_frames += 1
                assert np.array_equal(got["labels"][b.node_ptr[g]:b.node_ptr[g + 1]], labels[b.node_ptr[g]:b.node_ptr[g + 1]]), (where, g)
                assert np.array_equal(got["predictions"][b.edge_ptr[g]:b.edge_ptr[g + 1]], pruned[b.edge_ptr[g]:b.edge_ptr[g + 1]]), (where, g)
            else:
                cut_frames += 1
        assert got["flags"].sum() == 0
    print(f"frames with cut > 0: {cut_frames}, with cut == 0: {legal_frames}")
    assert cut_frames >= 20 and legal_frames >= 20, (cut_frames, legal_frames)     # the set is not one-sided (counted from the oracle's cut)


def test_composition_with_evaluation_summaries_and_a_capped_batch(synthetic):
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.tracking import cluster_summaries
    run = next(x for x in synthetic.runs if x.cams == 6 and x.th == 0.5)
    r, ex = run.r, run.r.exclusive()
    rows = evaluate_frames(r.batch, ex["predictions"], ex["labels"])
    want = evaluate_frames(r.batch, torch.from_numpy(run.want["predictions"]).cuda(), torch.from_numpy(run.want["labels"]).cuda())
    assert rows.shape == (24, 16) and np.array_equal(rows.cpu().numpy(), want.cpu().numpy(), equal_nan=True)
    s = cluster_summaries(r.batch, ex["labels"])
    size, n_cams = s.size.cpu().numpy(), s.n_cams.cpu().numpy()
    assert np.array_equal(size, n_cams) and size.sum() == run.f["n"] and int(s.count.sum()) == int(ex["n_clusters"].item())
    plain = cluster_summaries(r.batch, r.labels)                         # (the device chain's clusters are not all legal in this batch)
    assert (plain.size.cpu().numpy() > plain.n_cams.cpu().numpy()).any()
    # a capped batch closed under reversal, and the directed capped list of the one-call path: the oracle on their own edge lists
    f, node, reid = synthetic.data[4]
    for kw in (dict(top_k=3, symmetric="union"), dict(top_k=3)):
        rc = FramePipeline(synthetic.model, **kw)(*_args(f), node, reid)
        got, want = _host(rc.exclusive()), _oracle_of(rc, 0.5)
        _assert_equal(got, want, kw)
        assert rc.batch.edge_index.shape[1] < synthetic.runs[3].r.batch.edge_index.shape[1]
        assert oracle.one_per_camera(got["labels"], f["id_cam"])
