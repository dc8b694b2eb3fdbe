"""gnn_cca_amd.calibration on the MI355X: the one-pass threshold sweep (csrc/eval_sweep.cuh) against the loop it replaces -- predictions at
the threshold -> prune_and_cluster -> evaluate_frames, one threshold at a time -- bit for bit in all 16 columns, the partitions and the
kept edges included; the reference's own sweep (tests/golden/calibration/reid_sweep.npz: main.py:141-175); SweepAccumulator against EvalAccumulator;
the threshold switch of postprocess.threshold / FramePipeline; and the edges of the domain.  The scoring body of csrc/evaluate.hip was
factored for the sweep: its goldens run here once more."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _frames(rng, sizes, cams=4, node_dim=2048, reid_dim=256):
    sizes = np.asarray(sizes)
    n, g = int(sizes.sum()), len(sizes)
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, node_dim)).astype(np.float32),
                reid=rng.standard_normal((n, reid_dim)).astype(np.float32))


def _args(f):
    return f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"]


def _model(seed=0):
    import bench
    return bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=seed).cuda().eval()


def _shift_bias(m, b):
    """Put the decision boundary inside the logits so that decisions vary (as tests/test_gpu_evaluation.py does)."""
    with torch.no_grad():
        med = m(b)["classified_edges"][-1].median()
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= med
        m.load_state_dict(sd)


def _hand_batch(frames):
    """frames: list of (n, src, dst, lab) with frame-local ids -> a GraphBatch as evaluate_frames takes it."""
    from gnn_cca_amd.sharding import GraphBatch
    node_ptr, edge_ptr, ei, lab = [0], [0], [np.zeros((2, 0), np.int64)], [np.zeros(0, np.float32)]
    for n, src, dst, l in frames:
        v0 = node_ptr[-1]
        ei.append(np.stack([np.asarray(src, np.int64) + v0, np.asarray(dst, np.int64) + v0]).reshape(2, -1))
        lab.append(np.asarray(l, np.float32))
        node_ptr.append(v0 + n)
        edge_ptr.append(edge_ptr[-1] + len(src))
    b = GraphBatch(None, torch.from_numpy(np.concatenate(ei, axis=1)).cuda(), None, edge_ptr, node_ptr)
    b.edge_labels = torch.from_numpy(np.concatenate(lab)).cuda()
    b.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    b.edge_ptr_dev = torch.tensor(edge_ptr, dtype=torch.int32).cuda()
    return b


def _n(b):
    return int(b.node_ptr[-1])


def _loop(b, scores, ths, keep):
    """The loop the sweep replaces: per threshold, the predictions, prune_and_cluster, evaluate_frames."""
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import prune_and_cluster
    s = scores.reshape(-1).double()
    rows, labels, pruned = [], [], []
    for t in ths:
        preds = ((s >= float(t)) if keep == "ge" else (s <= float(t))).to(torch.int64)
        post = prune_and_cluster(b.edge_index, preds, _n(b), b.node_ptr_dev, b.edge_ptr_dev)
        rows.append(evaluate_frames(b, post["pruned"], post["labels"]))
        labels.append(post["labels"])
        pruned.append(post["pruned"])
    return torch.stack(rows).cpu().numpy(), torch.stack(labels).cpu().numpy(), torch.stack(pruned).cpu().numpy()


def _kept_on_host(b, scores, t, keep):
    """The rule restated on the host: active, and the reverse edge of the same frame is active."""
    ei = b.edge_index.cpu().numpy()
    s = scores.reshape(-1).cpu().numpy().astype(np.float64)
    active = (s >= t) if keep == "ge" else (s <= t)
    where = {(int(a), int(c)): k for k, (a, c) in enumerate(ei.T)}
    frame_of = np.searchsorted(np.asarray(b.edge_ptr), np.arange(ei.shape[1]), side="right")
    kept = np.zeros(ei.shape[1], dtype=np.int64)
    for k, (a, c) in enumerate(ei.T):
        r = where.get((int(c), int(a)))
        kept[k] = int(active[k] and r is not None and frame_of[r] == frame_of[k] and active[r])
    return kept


def _assert_sweep_equals_loop(b, scores, ths, keep, where):
    from gnn_cca_amd.calibration import sweep_thresholds
    rows, labels = sweep_thresholds(b, scores, ths, keep=keep, return_labels=True)
    g = len(b.node_ptr) - 1
    assert rows.shape == (len(ths), g, 16) and rows.dtype == torch.float64 and labels.shape == (len(ths), _n(b)) and labels.dtype == torch.int32
    assert torch.equal(rows, sweep_thresholds(b, scores, ths, keep=keep))                     # the same bits without the labels
    rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    want_rows, want_labels, want_pruned = _loop(b, scores, ths, keep)
    ei = b.edge_index.cpu().numpy()
    for t in range(len(ths)):
        bad = np.argwhere(~((rows[t] == want_rows[t]) | (np.isnan(rows[t]) & np.isnan(want_rows[t]))))
        assert np.array_equal(rows[t], want_rows[t], equal_nan=True), (where, t, ths[t], bad[:4])
        assert np.array_equal(labels[t], want_labels[t]), (where, t)
        # the loop's pruned predictions: inside the partition's clusters, and as many per frame as the row counts
        kept = want_pruned[t] == 1
        assert np.array_equal(labels[t][ei[0][kept]], labels[t][ei[1][kept]]), (where, t)
        per_frame = [float(want_pruned[t][b.edge_ptr[f]:b.edge_ptr[f + 1]].sum()) for f in range(g)]
        assert (rows[t][:, 3] + rows[t][:, 4]).tolist() == per_frame, (where, t)
    return rows, labels, want_pruned


@pytest.fixture(scope="module")
def model_batch():
    """Five frames of 0-24 detections on 4 cameras (one empty, one on a single camera), a model whose decisions vary, its probabilities."""
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.postprocess import threshold
    rng = np.random.default_rng(31)
    f = _frames(rng, [17, 0, 24, 9, 13])
    starts = np.concatenate([[0], np.cumsum(f["sizes"])])
    f["id_cam"][starts[3]:starts[4]] = 1                                   # frame 3: one camera, no edge
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    b = build_graph_batch(*_args(f), node, reid)
    m = _model()
    _shift_bias(m, b)
    with torch.no_grad():
        logits = m(b)["classified_edges"][-1]
    probs, _ = threshold(logits)
    return types.SimpleNamespace(f=f, node=node, reid=reid, batch=b, model=m, logits=logits, probs=probs)


def _seven(scores):
    """Seven thresholds: below every score, above every score, a duplicated one, one exactly equal to a score, two ordinary ones."""
    s = np.sort(scores.reshape(-1).cpu().numpy().astype(np.float64))
    exact = float(s[len(s) // 3])
    mid = float((s[len(s) // 2] + s[len(s) // 2 + 1]) / 2)
    return [mid, float(s[0]) - 0.25, exact, float(s[-1]) + 0.25, mid, float(s[(3 * len(s)) // 4]) + 1e-9, float(s[len(s) // 8])]


def test_sweep_equals_the_loop(model_batch):
    mb = model_batch
    b = mb.batch
    ep = b.edge_ptr
    assert ep[2] == ep[1] and ep[4] == ep[3] and b.edge_index.shape[1] > 500
    # (a) the model's probabilities, keep >= t
    ths = _seven(mb.probs)
    assert ths[1] < mb.probs.min().item() and mb.probs.max().item() < ths[3] and ths[2] in mb.probs.double().cpu().numpy()
    rows, _, pruned = _assert_sweep_equals_loop(b, mb.probs, ths, "ge", "probs")
    assert np.array_equal(rows[0], rows[4], equal_nan=True)                                   # the duplicate
    assert rows[3][:, 3].sum() + rows[3][:, 4].sum() == 0                                     # above every score: nothing predicted
    assert rows[1][:, 5].sum() == 0 and rows[1][:, 6].sum() == 0                               # below every score: everything (symmetric list)
    assert len({float(r[:, 3].sum()) for r in rows}) >= 4                                     # the decisions do vary
    for t in (0, 2, 5):
        assert np.array_equal(pruned[t], _kept_on_host(b, mb.probs, ths[t], "ge")), t
    # the thresholded predictions of postprocess.threshold(at=...) are the loop's
    from gnn_cca_amd.postprocess import threshold
    for t in (ths[0], ths[2], ths[6]):
        assert torch.equal(threshold(mb.logits, at=t)[1], (mb.probs.double() >= t).to(torch.int64))
    # (b) a distance column of the edge attributes (a strided view), keep <= t
    dist = b.edge_attr[:, 2]
    assert not dist.is_contiguous()
    ths = _seven(dist)
    rows, _, pruned = _assert_sweep_equals_loop(b, dist, ths, "le", "edge_attr[:, 2]")
    assert rows[1][:, 3].sum() + rows[1][:, 4].sum() == 0 and rows[3][:, 5].sum() + rows[3][:, 6].sum() == 0
    for t in (0, 2):
        assert np.array_equal(pruned[t], _kept_on_host(b, dist, ths[t], "le")), t
    # a score that is not a number is never active, under either comparison
    s = mb.probs.clone()
    s[::7] = float("nan")
    _assert_sweep_equals_loop(b, s, [ths[0], 0.5], "ge", "nan ge")
    _assert_sweep_equals_loop(b, s, [0.5], "le", "nan le")


def test_more_nodes_than_threads_and_many_rounds():
    from gnn_cca_amd.graph_build import build_graph_batch
    rng = np.random.default_rng(5)
    # two frames of 1100 detections, capped at three candidates each: more nodes than a workgroup has threads, a directed list
    f = _frames(rng, [1100, 1100], cams=4, node_dim=8, reid_dim=16)
    b = build_graph_batch(*_args(f), torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda(), top_k=3)
    assert b.edge_index.shape[1] == 2200 * 3
    scores = torch.rand(b.edge_index.shape[1], generator=torch.Generator().manual_seed(1)).cuda()
    rows, labels, _ = _assert_sweep_equals_loop(b, scores, [0.0, 0.35, 0.8], "ge", "1100 x 2, top_k=3")
    assert rows[0][:, 15].max() < 1100 and rows[0][0, 15] < rows[1][0, 15] < rows[2][0, 15] <= 1100

    # a path of 200 nodes (every hop both ways) among inactive edges, its edges in row order and shuffled; and a random frame whose
    # edges are permuted inside the frame (rows no longer sorted: the plan's sorted copy)
    def path(n, shuffle):
        src = np.concatenate([np.arange(n - 1), np.arange(1, n)])
        dst = np.concatenate([np.arange(1, n), np.arange(n - 1)])
        extra = rng.integers(0, n, size=(2, 300))
        extra = extra[:, np.abs(extra[0] - extra[1]) > 1]
        extra = np.unique(np.concatenate([extra, extra[::-1]], axis=1), axis=1)
        s = np.concatenate([np.full(len(src), 0.9), rng.uniform(0.0, 0.4, size=extra.shape[1])])
        src, dst = np.concatenate([src, extra[0]]), np.concatenate([dst, extra[1]])
        order = rng.permutation(len(src)) if shuffle else np.lexsort((dst, src))
        return (n, src[order], dst[order], (rng.random(len(src)) < 0.5).astype(np.float32)), s[order]

    def random_frame(n, e):
        pairs = rng.integers(0, n, size=(2, e))
        pairs = pairs[:, pairs[0] != pairs[1]]
        pairs = np.unique(np.concatenate([pairs, pairs[::-1, : pairs.shape[1] // 2]], axis=1), axis=1)
        order = rng.permutation(pairs.shape[1])
        return (n, pairs[0][order], pairs[1][order], (rng.random(pairs.shape[1]) < 0.4).astype(np.float32)), rng.random(pairs.shape[1])

    (p0, s0), (p1, s1), (r2, s2) = path(200, False), path(200, True), random_frame(70, 400)
    for frames, s, where in (([p0], [s0], "path, rows sorted"), ([p1, r2], [s1, s2], "path shuffled + permuted frame"),
                             ([r2, p0], [s2, s0], "permuted frame + path")):
        b = _hand_batch(frames)
        scores = torch.from_numpy(np.concatenate(s).astype(np.float32)).cuda()
        rows, labels, _ = _assert_sweep_equals_loop(b, scores, [0.5, 0.2, 0.95], "ge", where)
        g = [fr[0] for fr in frames].index(200)
        v0 = b.node_ptr[g]
        assert rows[0][g, 15] == 1 and np.all(labels[0][v0:v0 + 200] == v0), where            # the whole path: one cluster
        assert rows[2][g, 15] == 200 and np.array_equal(labels[2][v0:v0 + 200], np.arange(v0, v0 + 200)), where


def test_golden_reid_sweep():
    from gnn_cca_amd.calibration import SweepAccumulator, sweep_thresholds
    z = np.load(os.path.join(GOLDEN, "calibration", "reid_sweep.npz"))
    ei = z["edge_index"]
    b = _hand_batch([(int(z["n_nodes"]), ei[0], ei[1], z["edge_labels"])])
    ths = z["thresholds"]
    rows = sweep_thresholds(b, torch.from_numpy(z["scores"]).cuda(), ths, keep="le")
    host = rows.cpu().numpy()
    assert host.shape == (100, 1, 16)
    for col, name in ((3, "TP"), (4, "FP"), (5, "FN"), (6, "TN")):
        assert np.array_equal(host[:, 0, col], z[name].astype(np.float64)), name             # exact counts at every threshold
    for col, name in ((0, "P"), (1, "R"), (2, "F")):
        assert np.array_equal(host[:, 0, col], z[name]), name                                 # one frame: the row's P / R / F are the dataset's
    acc = SweepAccumulator(ths).add(rows)
    res = acc.result()
    for key, name in (("P_micro", "P"), ("R_micro", "R"), ("F_micro", "F")):
        assert np.array_equal(res[key], z[name]), name
    assert np.array_equal(acc.best(), np.where(z["F"] == np.max(z["F"]))[0])
    assert np.array_equal(acc.thresholds[acc.best()], ths[np.where(z["F"] == np.max(z["F"]))])


def test_accumulator_equals_eval_accumulator_with_one_synchronisation(model_batch, monkeypatch):
    from gnn_cca_amd.calibration import SweepAccumulator, sweep_thresholds
    from gnn_cca_amd.evaluation import EvalAccumulator
    from gnn_cca_amd.graph_build import build_graph_batch
    mb = model_batch
    rng = np.random.default_rng(77)
    f2 = _frames(rng, [12, 20, 5, 16, 8, 21, 3], node_dim=8, reid_dim=16)
    b2 = build_graph_batch(*_args(f2), torch.from_numpy(f2["node"]).cuda(), torch.from_numpy(f2["reid"]).cuda())
    s2 = torch.rand(b2.edge_index.shape[1], generator=torch.Generator().manual_seed(2)).cuda()
    ths = [0.3, 0.45, 0.5, 0.55, 0.5, 0.9]
    calls = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(1), real_cpu(self, *a, **k))[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        big = torch.randn(2048, 2048, device="cuda")
        for _ in range(20):                                                  # pending work on the stream the sweeps are queued behind
            big = big @ big * 1e-3
        acc = SweepAccumulator(ths)
        r1 = sweep_thresholds(mb.batch, mb.probs, ths)
        acc.add(r1)
        r2 = sweep_thresholds(b2, s2, ths)
        acc.add(r2)
        assert not calls and len(acc) == 12                                  # nothing was copied to the host so far
        res = acc.result()
        assert len(calls) == 1                                               # the one synchronisation
        assert acc.result() is res and len(calls) == 1
    monkeypatch.undo()
    torch.cuda.synchronize()
    for t in range(len(ths)):
        want = EvalAccumulator().add(r1[t]).add(r2[t]).result()
        got = res["aggregates"][t]
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert got[k] == v or (np.isnan(got[k]) and np.isnan(v)), (t, k, got[k], v)         # bit for bit
        assert (res["TP"][t], res["FP"][t], res["FN"][t], res["TN"][t]) == (want["TP"], want["FP"], want["FN"], want["TN"])
        tp, fp, fn = want["TP"], want["FP"], want["FN"]
        p, r = (tp / (tp + fp) if tp + fp else 0), (tp / (tp + fn) if tp + fn else 0)
        assert res["P_micro"][t] == p and res["R_micro"][t] == r and res["F_micro"][t] == (2 * (p * r) / (p + r) if p + r else 0)
    assert res["TP"][2] == res["TP"][4] and res["F_micro"][2] == res["F_micro"][4]          # the duplicated threshold
    assert set(acc.best("F_micro").tolist()) == set(np.where(res["F_micro"] == res["F_micro"].max())[0].tolist())


def test_threshold_switch(model_batch):
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.postprocess import threshold
    mb = model_batch
    x = mb.logits
    p0, d0 = threshold(x)
    p1, d1 = threshold(x, at=0.5)
    assert torch.equal(p0, p1) and torch.equal(d0, d1) and d0.dtype == torch.int64
    p3, d3 = threshold(x, at=0.3)
    assert torch.equal(p3, p0) and torch.equal(d3, (p0.double() >= 0.3).to(torch.int64)) and int(d3.sum()) > int(d0.sum())
    # a threshold that float32 cannot hold: compared in float64 against the widened probability
    at = float(np.nextafter(np.float64(p0[5].item()), 1.0))
    assert int(threshold(x, at=at)[1][5]) == 0 and int(threshold(x, at=p0[5].item())[1][5]) == 1
    args = (*_args(mb.f), mb.node, mb.reid)
    base, same, low = FramePipeline(mb.model), FramePipeline(mb.model, threshold=0.5), FramePipeline(mb.model, threshold=0.3)
    r, s, w = base(*args), same(*args), low(*args)
    assert r._d2h is not None and s._d2h is not None and w._d2h is None                        # 0.5: the one-call path; 0.3: step by step
    for name in ("probs", "preds", "pruned", "flow_out", "flow_in", "labels", "n_clusters", "triggers"):
        assert torch.equal(getattr(r, name), getattr(s, name)), name
    for name in ("x", "edge_index", "edge_attr", "edge_labels"):
        assert torch.equal(getattr(r.batch, name), getattr(s.batch, name)), name
    assert all(torch.equal(a, c) for a, c in zip(r.outputs["classified_edges"], s.outputs["classified_edges"]))
    assert torch.equal(r.evaluate(final=False), s.evaluate(final=False))
    assert torch.equal(w.probs, r.probs) and torch.equal(w.preds, (r.probs.double() >= 0.3).to(torch.int64))
    swept = r.sweep([0.3, 0.5])
    assert swept.shape == (2, 5, 16)
    assert torch.equal(w.evaluate(final=False), swept[0])                                      # bit for bit (NaN-free rows)
    assert torch.equal(r.evaluate(final=False), swept[1])
    assert not torch.equal(swept[0], swept[1])
    for pipe in (base, same, low):
        pipe.close()


def test_edges_of_the_domain(model_batch):
    from gnn_cca_amd.calibration import sweep_thresholds
    from gnn_cca_amd.evaluation import evaluate_frames
    mb = model_batch
    # T = 1
    _assert_sweep_equals_loop(mb.batch, mb.probs, [0.5], "ge", "T = 1")
    # E = 0: frames of three, zero and one node; one cluster per node, as evaluate_frames scores the same partition
    none = np.zeros(0, np.int64)
    b = _hand_batch([(3, none, none, none), (0, none, none, none), (1, none, none, none)])
    rows, labels = sweep_thresholds(b, torch.zeros(0, device="cuda"), [0.1, 0.9], return_labels=True)
    want = evaluate_frames(b, torch.zeros(0, dtype=torch.int64, device="cuda"), torch.arange(4, dtype=torch.int32, device="cuda"))
    assert rows.shape == (2, 3, 16) and torch.equal(rows[0], want) and torch.equal(rows[1], want)
    assert labels.cpu().tolist() == [[0, 1, 2, 3]] * 2 and rows[0][:, 15].cpu().tolist() == [3.0, 0.0, 1.0]
    # G = 0: well-formed empty rows
    empty = types.SimpleNamespace(node_ptr=[0], edge_ptr=[0], edge_index=torch.zeros((2, 0), dtype=torch.int64, device="cuda"),
                                  edge_labels=torch.zeros(0, device="cuda"))
    rows, labels = sweep_thresholds(empty, torch.zeros(0, device="cuda"), [0.1, 0.2, 0.3], return_labels=True)
    assert rows.shape == (3, 0, 16) and rows.dtype == torch.float64 and labels.shape == (3, 0)
    # a frame of one node between two ordinary ones
    b = _hand_batch([(2, [0, 1], [1, 0], [1, 1]), (1, none, none, none), (3, [0, 1, 1, 2], [1, 0, 2, 1], [1, 1, 0, 0])])
    s = torch.tensor([0.9, 0.8, 0.7, 0.6, 0.2, 0.9], device="cuda")
    rows, labels, _ = _assert_sweep_equals_loop(b, s, [0.5, 0.75, 0.1], "ge", "one-node frame")
    assert labels.tolist() == [[0, 0, 2, 3, 3, 5], [0, 0, 2, 3, 4, 5], [0, 0, 2, 3, 3, 3]] and rows[0][1, 15] == 1
    # everything active on complete cross-camera frames: one cluster per connected frame, every node its own where there is no edge
    rows, labels, _ = _assert_sweep_equals_loop(mb.batch, mb.probs, [0.0], "ge", "all active")
    assert rows[0][:, 15].tolist() == [1.0, 0.0, 1.0, 9.0, 1.0] and rows[0][:, 5].sum() == 0 and rows[0][:, 6].sum() == 0
    nptr = mb.batch.node_ptr
    assert np.array_equal(labels[0][nptr[3]:nptr[4]], np.arange(nptr[3], nptr[4])) and np.all(labels[0][:nptr[1]] == 0)


def test_eval_frames_goldens_through_the_factored_body():
    """tests/test_gpu_evaluation.py's fixture check once more (same tolerances: its module docstring has them)."""
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.calibration import sweep_thresholds
    z = np.load(os.path.join(GOLDEN, "post2_eval_frames.npz"))
    nptr, eptr = z["node_ptr"].astype(np.int64), z["edge_ptr"].astype(np.int64)
    b = _hand_batch([(int(nptr[g + 1] - nptr[g]), z["src"][eptr[g]:eptr[g + 1]], z["dst"][eptr[g]:eptr[g + 1]], z["edge_labels"][eptr[g]:eptr[g + 1]])
                     for g in range(len(nptr) - 1)])
    labels = np.concatenate([_smallest(z["id_pred"][nptr[g]:nptr[g + 1]], int(nptr[g])) for g in range(len(nptr) - 1)])
    pred = torch.from_numpy(z["predictions"].astype(np.int64)).cuda()
    rows = evaluate_frames(b, pred, torch.from_numpy(labels).cuda()).cpu().numpy()
    want = z["metrics"]
    tol = {8: 1e-8, 9: 1e-12, 10: 1e-12, 11: 1e-12}
    for q in range(want.shape[1]):
        if q in tol:
            assert np.abs(rows[:, q] - want[:, q]).max() <= tol[q], q
        else:
            assert np.array_equal(rows[:, q], want[:, q]), q
    # and the sweep's counts on the goldens' own predictions used as scores (1 = active): TP + FP can only shrink under pruning
    swept = sweep_thresholds(b, pred.float(), [0.5]).cpu().numpy()[0]
    assert np.all(swept[:, 3] <= rows[:, 3]) and np.all(swept[:, 4] <= rows[:, 4]) and np.all(swept[:, 3] + swept[:, 5] == rows[:, 3] + rows[:, 5])


def _smallest(part, v0):
    first = {}
    for v, c in enumerate(np.asarray(part).tolist()):
        first.setdefault(c, v)
    return np.array([first[c] + v0 for c in np.asarray(part).tolist()], dtype=np.int32)
