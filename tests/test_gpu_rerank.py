"""gnn_cca_amd.rerank on the GPU against tests/rerank_oracle.py and the goldens of tests/golden/rerank/ (the reference's own
libs.utils.re_ranking, tests/golden/make_golden_rerank.py).

Tolerances, none taken from the code under test:
  * re-ranked values: 4 d_ref against the float64 oracle, d_ref = the largest error of the reference's own float32 result against that
    oracle over the goldens (stored in the fixtures).  Same arithmetic width; the summation order differs and the device expf may differ
    from numpy's by a couple of ulp, which the factor covers.
  * distances: relative error (R + 2) 2^-24 against the float64 oracle, the textbook bound of an fp32 sum of R squares plus a square root.
  * everything discrete (rank prefixes, X(i), the support of V', predictions, lam = 1) is exact.
Frames are clustered embeddings (persons x cameras + noise 0.6, as the goldens); every seeded frame is asserted tie-free where the
reference's unstable sort could otherwise decide."""
import glob
import os
import types

import numpy as np
import pytest
import torch

import rerank_oracle as oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "rerank", "*.npz")))
D_REF = float(np.load(GOLDEN[0])["d_ref"])
TOL = 4 * D_REF
SIZES = (1, 2, 3, 7, 21, 22, 34, 64, 65, 127, 128)
# k1, k2, lam: the default; both directions of the half-to-even rounding; the widest k1; k2 = 1 (step 6 skipped) and k2 > most frames;
# the two ends of lam
PARAMS = ((20, 6, 0.3), (5, 3, 0.3), (7, 1, 0.3), (64, 6, 0.3), (64, 64, 0.3), (20, 6, 0.0), (20, 6, 1.0))


def _embeddings(n, seed, cams=4, width=16):
    rng = np.random.default_rng(seed)
    cam = (np.arange(n) % cams).astype(np.int32)
    person = np.arange(n) // cams
    centres = rng.normal(0, 1, size=(person.max() + 1, width))
    return (centres[person] + 0.6 * rng.normal(0, 1, size=(n, width))).astype(np.float32), cam


_frames, _wants = {}, {}


def _frame(n):
    """One seeded frame of n detections: (D float32 [n, n] symmetric with a zero diagonal, cam)."""
    if n not in _frames:
        x, cam = _embeddings(n, 100 + n)
        _frames[n] = (oracle.frame_distances(x, [0, n], np.float64)[0].astype(np.float32), cam)
    return _frames[n]


def _want(n, k1, k2, lam):
    """(float64 result, the float32 oracle's debug dict) of frame n, computed once."""
    key = (n, k1, k2, lam)
    if key not in _wants:
        D = _frame(n)[0]
        want64 = oracle.rerank(D, k1, k2, lam, np.float64)
        got32, dbg = oracle.rerank(D, k1, k2, lam, np.float32, debug=True)
        head = np.sort(dbg["O"], axis=1)[:, :k1 + 2]
        assert (np.diff(head, axis=1) > 0).all(), f"frame {n}: a tie among the first k1 + 2 values of a row of O"
        dbg["out32"] = got32
        _wants[key] = (want64, dbg)
    return _wants[key]


def _matrices(sizes, device_ptr=True):
    from gnn_cca_amd.rerank import FrameMatrices
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    data = torch.from_numpy(np.concatenate([_frame(n)[0].reshape(-1) for n in sizes])).cuda()
    return FrameMatrices(data, node_ptr, torch.tensor(node_ptr, dtype=torch.int32).cuda() if device_ptr else None)


def _check_rerank(sizes, k1, k2, lam, device_ptr=True):
    from gnn_cca_amd.rerank import rerank_frames
    dist = _matrices(sizes, device_ptr)
    out, dbg = rerank_frames(dist, k1, k2, lam, debug=True)
    plain = rerank_frames(dist, k1, k2, lam)
    assert torch.equal(plain.data, out.data)        # the debug instantiation computes the same bits
    assert out.mat_ptr == dist.mat_ptr == np.concatenate([[0], np.cumsum(np.square(sizes))]).tolist() and out.node_ptr == dist.node_ptr
    rank, expansion, support = dbg["rank"].cpu().numpy(), dbg["expansion"].cpu().numpy(), dbg["support"].cpu().numpy()
    worst = 0.0
    for g, n in enumerate(sizes):
        want64, o = _want(n, k1, k2, lam)
        got = out.frame(g).cpu().numpy()
        assert got.shape == (n, n) and got.dtype == np.float32
        v0 = dist.node_ptr[g]
        p = o["prefix"]
        assert np.array_equal(rank[v0:v0 + n, :p], o["rank"][:, :p]), (n, "rank prefixes")
        assert (rank[v0:v0 + n, p:] == -1).all()
        assert np.array_equal(expansion[v0:v0 + n, :n], o["expansion"]) and not expansion[v0:v0 + n, n:].any(), (n, "X(i)")
        assert np.array_equal(support[v0:v0 + n, :n], o["support"]) and not support[v0:v0 + n, n:].any(), (n, "support of V'")
        err = float(np.abs(got.astype(np.float64) - want64).max())
        worst = max(worst, err)
        print(f"rerank n={n} k1={k1} k2={k2} lam={lam}: max |gpu - fp64 oracle| {err:.3e} (tolerance {TOL:.3e})")
        if lam == 1.0:
            assert np.array_equal(got, o["O"]), (n, "lam = 1 is O bit for bit")
    assert worst <= TOL, (worst, TOL)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_rerank_every_size_alone(n):
    _check_rerank((n,), 20, 6, 0.3, device_ptr=n % 2 == 0)     # (odd sizes: node_ptr goes up through pinned memory)


@pytest.mark.parametrize("k1,k2,lam", PARAMS)
def test_rerank_mixed_batch(k1, k2, lam):
    """All sizes in one batch, large and small frames interleaved: a wrong matrix offset shows here."""
    sizes = (34, 1, 128, 2, 65, 3, 127, 7, 64, 21, 22)
    out = _check_rerank(sizes, k1, k2, lam)
    from gnn_cca_amd.rerank import rerank_frames
    again = rerank_frames(_matrices(sizes), k1, k2, lam)
    assert torch.equal(again.data.view(torch.int32), out.data.view(torch.int32))      # two runs, the same bits


def test_rerank_small_batch_alone_matches_mixed():
    """The LDS stride follows the batch's largest frame; a frame's result does not depend on it."""
    from gnn_cca_amd.rerank import rerank_frames
    small = rerank_frames(_matrices((34, 7)), 20, 6, 0.3)
    mixed = rerank_frames(_matrices((7, 128, 34)), 20, 6, 0.3)
    assert torch.equal(small.frame(0), mixed.frame(2)) and torch.equal(small.frame(1), mixed.frame(0))


def test_degenerate_frames():
    """A single detection and identical embeddings: the column maximum is 0 and O is 0 (the reference: NaN), stated in the docstring."""
    from gnn_cca_amd.rerank import FrameMatrices, rerank_frames
    node_ptr = [0, 1, 4]
    dist = FrameMatrices(torch.zeros(10).cuda(), node_ptr)
    out = rerank_frames(dist, 20, 6, 0.3)
    for g, n in enumerate((1, 3)):
        want = oracle.rerank(np.zeros((n, n), dtype=np.float32), 20, 6, 0.3, np.float64)
        got = out.frame(g).cpu().numpy()
        assert np.isfinite(got).all() and np.abs(got - want).max() <= TOL


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_goldens(path):
    from gnn_cca_amd.rerank import FrameMatrices, rank_predictions, rerank_frames
    z = np.load(path)
    D, cam, k1, k2, lam, off = z["D"], z["cam"], int(z["k1"]), int(z["k2"]), float(z["lam"]), z["offdiag"]
    n = D.shape[0]
    want64, o64 = oracle.rerank(D, k1, k2, lam, np.float64, debug=True)
    dist = FrameMatrices(torch.from_numpy(D.reshape(-1)).cuda(), [0, n])
    out, dbg = rerank_frames(dist, k1, k2, lam, debug=True)
    got = out.frame(0).cpu().numpy()
    err, err_ref = float(np.abs(got.astype(np.float64) - want64).max()), float(np.abs(got.astype(np.float64) - z["ref"])[off].max())
    print(f"{os.path.basename(path)}: max |gpu - fp64 oracle| {err:.3e}, |gpu - reference| {err_ref:.3e} (tolerance {TOL:.3e}, d_ref {D_REF:.3e})")
    p = o64["prefix"]
    assert np.array_equal(dbg["rank"].cpu().numpy()[:, :p], o64["rank"][:, :p])
    assert np.array_equal(dbg["expansion"].cpu().numpy()[:, :n], o64["expansion"])
    assert np.array_equal(dbg["support"].cpu().numpy()[:, :n], o64["support"])
    assert err <= TOL
    assert err_ref <= TOL + D_REF       # (the reference itself is d_ref away from the oracle)
    # rank-R predictions from the GPU's matrix equal the selection from the reference's matrix
    src, dst = np.nonzero(cam[:, None] != cam[None, :])
    ei = np.stack([src, dst]).astype(np.int64)
    batch = types.SimpleNamespace(node_ptr=[0, n], node_ptr_dev=torch.tensor([0, n], dtype=torch.int32).cuda(),
                                  edge_ptr_dev=torch.tensor([0, ei.shape[1]], dtype=torch.int32).cuda(),
                                  cam_dev=torch.from_numpy(cam).cuda(), edge_index=torch.from_numpy(ei).cuda())
    ref = np.where(off, z["ref"], 0)
    for r in z["ranks"].tolist():
        pred = rank_predictions(batch, out, rank=r).cpu().numpy()
        assert np.array_equal(pred, oracle.rank_predictions([ref], [0, n], cam, ei, r)), r


@pytest.mark.parametrize("width", (1, 37, 256, 2048))
def test_frame_distances(width):
    from gnn_cca_amd.rerank import frame_distances
    sizes = (1, 2, 17, 33, 130, 16)      # below, at and across the 16-row tile; one frame above the re-ranking's limit
    node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    rng = np.random.default_rng(width)
    x = rng.standard_normal((node_ptr[-1], width)).astype(np.float32)
    x[40] = x[41]                                            # two identical rows: an exact zero off the diagonal
    batch = types.SimpleNamespace(node_ptr=node_ptr, reid_embeds=torch.from_numpy(x).cuda())
    if width != 37:
        batch.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    dist = frame_distances(batch)
    assert dist.mat_ptr == np.concatenate([[0], np.cumsum(np.square(sizes))]).tolist() and dist.node_ptr == node_ptr
    assert dist.data.dtype == torch.float32 and dist.data.numel() == dist.mat_ptr[-1]
    again = frame_distances(batch)
    assert torch.equal(again.data, dist.data)
    want = oracle.frame_distances(x, node_ptr, np.float64)
    bound = (width + 2) * 2.0 ** -24
    worst = 0.0
    for g, n in enumerate(sizes):
        got = dist.frame(g).cpu().numpy()
        assert got.shape == (n, n)
        assert not got.diagonal().any() and np.array_equal(got, got.T)        # exactly zero, exactly symmetric
        rel = np.abs(got.astype(np.float64) - want[g]) / np.where(want[g] > 0, want[g], 1.0)
        worst = max(worst, float(rel.max()))
        assert rel.max() <= bound, (n, float(rel.max()), bound)
    assert node_ptr[3] <= 40 < 41 < node_ptr[4] and dist.frame(3)[40 - node_ptr[3], 41 - node_ptr[3]] == 0
    print(f"frame_distances R={width}: max relative error {worst:.3e} (bound {bound:.3e})")


def _real_batch(top_k=None, seed=5):
    """A batch as the pipeline makes it: frames of 5, 1, 34, 6 (one camera: no edges), 65 and 128 detections, reid width 37."""
    from gnn_cca_amd.graph_build import build_graph_batch
    sizes = np.array([5, 1, 34, 6, 65, 128])
    rng = np.random.default_rng(seed)
    n = int(sizes.sum())
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    id_cam = np.concatenate([np.arange(s) % 4 for s in sizes])
    id_cam[node_ptr[3]:node_ptr[4]] = 2
    reid = np.concatenate([_embeddings(s, seed + s, width=37)[0] for s in sizes])
    ids = np.concatenate([np.arange(s) // 4 for s in sizes])
    b = build_graph_batch(rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), ids, id_cam, sizes, rng.uniform(10, 90, len(sizes)),
                          torch.from_numpy(rng.standard_normal((n, 32)).astype(np.float32)).cuda(), torch.from_numpy(reid).cuda(), top_k=top_k)
    return b, id_cam


@pytest.fixture(scope="module")
def real():
    from gnn_cca_amd.rerank import frame_distances, rerank_frames
    b, cam = _real_batch()
    dist = frame_distances(b)
    rer = rerank_frames(dist)
    mats = [rer.frame(g).cpu().numpy() for g in range(len(rer))]
    return types.SimpleNamespace(batch=b, cam=cam, dist=dist, rer=rer, mats=mats)


@pytest.mark.parametrize("rank", (1, 2, 1000))
def test_rank_predictions_equal_the_oracle_on_the_gpu_matrix(real, rank):
    from gnn_cca_amd.rerank import rank_predictions
    b = real.batch
    assert b.edge_ptr[3] == b.edge_ptr[4] and b.edge_ptr[1] == b.edge_ptr[2]        # the one-camera frame and the single detection
    pred = rank_predictions(b, real.rer, rank=rank)
    assert pred.dtype == torch.int64 and pred.shape == (b.edge_index.shape[1],)
    ei = b.edge_index.cpu().numpy()
    want = oracle.rank_predictions(real.mats, b.node_ptr, real.cam, ei, rank)
    assert np.array_equal(pred.cpu().numpy(), want)
    if rank == 1000:
        assert want.all()                        # above every degree: every cross-camera pair, and nothing from the same camera
    else:
        assert 0 < want.sum() < len(want)
    where = {(int(a), int(c)): k for k, (a, c) in enumerate(ei.T)}
    back = np.array([where[(int(c), int(a))] for a, c in ei.T])
    assert np.array_equal(want[back], want)      # symmetric by construction


def test_rank_predictions_on_a_capped_batch(real):
    from gnn_cca_amd.rerank import frame_distances, rank_predictions
    b, cam = _real_batch(top_k=3)
    assert b.edge_index.shape[1] < real.batch.edge_index.shape[1]
    dist = frame_distances(b)
    assert torch.equal(dist.data, real.dist.data)
    for rank in (1, 2):
        pred = rank_predictions(b, dist, rank=rank).cpu().numpy()
        mats = [dist.frame(g).cpu().numpy() for g in range(len(dist))]
        want = oracle.rank_predictions(mats, b.node_ptr, cam, b.edge_index.cpu().numpy(), rank)
        assert np.array_equal(pred, want) and 0 < want.sum() < len(want)


def test_exact_ties_go_to_the_smaller_node_id():
    from gnn_cca_amd.rerank import FrameMatrices, rank_predictions
    cam = np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)
    D = np.full((6, 6), 5.0, dtype=np.float32)      # every candidate ties: rank 1 picks the smallest cross-camera id, rank 2 the next
    D[0, 4] = D[4, 0] = 1.0                         # one real winner
    np.fill_diagonal(D, 0)
    src, dst = np.nonzero(cam[:, None] != cam[None, :])
    ei = np.stack([src, dst]).astype(np.int64)
    batch = types.SimpleNamespace(node_ptr=[0, 6], node_ptr_dev=torch.tensor([0, 6], dtype=torch.int32).cuda(),
                                  edge_ptr_dev=torch.tensor([0, ei.shape[1]], dtype=torch.int32).cuda(),
                                  cam_dev=torch.from_numpy(cam).cuda(), edge_index=torch.from_numpy(ei).cuda())
    dist = FrameMatrices(torch.from_numpy(D.reshape(-1)).cuda(), [0, 6])
    sel1 = {0: 4, 1: 2, 2: 0, 3: 0, 4: 0, 5: 0}
    want1 = np.array([int(sel1[a] == c or sel1[c] == a) for a, c in ei.T])
    assert np.array_equal(rank_predictions(batch, dist, rank=1).cpu().numpy(), want1)
    for rank in (1, 2, 3):
        assert np.array_equal(rank_predictions(batch, dist, rank=rank).cpu().numpy(), oracle.rank_predictions([D], [0, 6], cam, ei, rank))
    sel2 = oracle.select(D, cam, 2)
    assert sel2[0].nonzero()[0].tolist() == [2, 4] and sel2[1].nonzero()[0].tolist() == [2, 3] and sel2[5].nonzero()[0].tolist() == [0, 1]


def test_rank_baseline_is_the_chain_and_replays_from_a_graph(real):
    from gnn_cca_amd.evaluation import EvalAccumulator, evaluate_frames
    from gnn_cca_amd.postprocess import prune_and_cluster
    from gnn_cca_amd.rerank import rank_baseline
    b = real.batch
    n = b.node_ptr[-1]
    ei = b.edge_index.cpu().numpy()
    for kw, mats in ((dict(rank=1), real.mats), (dict(rank=2, rerank=False), [real.dist.frame(g).cpu().numpy() for g in range(len(real.dist))])):
        rows = rank_baseline(b, **kw)
        pred = torch.from_numpy(oracle.rank_predictions(mats, b.node_ptr, real.cam, ei, kw["rank"])).cuda()
        post = prune_and_cluster(b.edge_index, pred, n, b.node_ptr_dev, b.edge_ptr_dev)
        assert torch.equal(post["pruned"], pred)          # symmetric predictions: pruning removes nothing
        want = evaluate_frames(b, post["pruned"], post["labels"])
        assert rows.shape == (6, 16) and rows.dtype == torch.float64
        assert torch.equal(rows.view(torch.int64), want.view(torch.int64))
    res = EvalAccumulator().add(rank_baseline(b)).result()
    assert all(np.isfinite(res[k]) for k in ("RI", "MI", "hom", "com", "v"))
    eager = rank_baseline(b)      # warm-up: the LDS attribute and the allocator's blocks exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = rank_baseline(b)
    for _ in range(2):
        static.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static.view(torch.int64), eager.view(torch.int64))
