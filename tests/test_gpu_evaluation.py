"""gnn_cca_amd.evaluation on the MI355X: the per-frame metrics of inference.py:349-371 (csrc/evaluate.hip) against the reference's goldens
(tests/golden/make_golden_eval.py) and the host restatement (tests/helpers/eval_oracle.py).  Exact: counts, P, R, F, precision0/1, ARI,
the cluster counts and the GT partition; homogeneity / completeness / V within 1e-12, AMI within 1e-8."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import eval_oracle as eo  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = {8: 1e-8, 9: 1e-12, 10: 1e-12, 11: 1e-12}


def _check(got, want, where=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape[0] == want.shape[0], where
    for q in range(want.shape[1]):
        if q in TOL:
            err = np.abs(got[:, q] - want[:, q]).max(initial=0.0)
            assert err <= TOL[q], (where, eo.COLUMNS[q], err)
        else:
            bad = np.flatnonzero(got[:, q] != want[:, q])
            assert bad.size == 0, (where, eo.COLUMNS[q], bad[:5], got[bad[:5], q], want[bad[:5], q])


def _same_partition(a, b):
    pairs = set(zip(np.asarray(a).tolist(), np.asarray(b).tolist()))
    return len(pairs) == len(set(np.asarray(a).tolist())) == len(set(np.asarray(b).tolist()))


def _smallest_id(part, v0=0):
    """Relabel a partition to the pipeline's convention: a node's label is the smallest (global) node id of its cluster."""
    part = np.asarray(part)
    first = {}
    for v, c in enumerate(part.tolist()):
        first.setdefault(c, v)
    return np.array([first[c] + v0 for c in part.tolist()], dtype=np.int32)


def _batch(frames):
    """frames: list of dicts n, src, dst (local), lab, pred, part -> GraphBatch, predictions, labels (device), host arrays."""
    from gnn_cca_amd.sharding import GraphBatch
    node_ptr, edge_ptr, ei, lab, pred, labels = [0], [0], [], [], [], []
    for f in frames:
        v0 = node_ptr[-1]
        ei.append(np.stack([f["src"] + v0, f["dst"] + v0]))
        lab.append(f["lab"])
        pred.append(f["pred"])
        labels.append(_smallest_id(f["part"], v0))
        node_ptr.append(v0 + f["n"])
        edge_ptr.append(edge_ptr[-1] + len(f["src"]))
    ei = np.concatenate(ei, axis=1).astype(np.int64) if ei else np.zeros((2, 0), np.int64)
    lab, pred, labels = np.concatenate(lab).astype(np.float32), np.concatenate(pred).astype(np.int64), np.concatenate(labels)
    b = GraphBatch(None, torch.from_numpy(ei).cuda(), None, edge_ptr, node_ptr)
    b.edge_labels = torch.from_numpy(lab).cuda()
    b.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    b.edge_ptr_dev = torch.tensor(edge_ptr, dtype=torch.int32).cuda()
    return b, torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda(), (ei, lab, pred, labels, node_ptr, edge_ptr)


def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    nptr, eptr = z["node_ptr"].astype(np.int64), z["edge_ptr"].astype(np.int64)
    frames = []
    for g in range(len(nptr) - 1):
        v0, v1, k0, k1 = nptr[g], nptr[g + 1], eptr[g], eptr[g + 1]
        frames.append(dict(n=int(v1 - v0), src=z["src"][k0:k1].astype(np.int64), dst=z["dst"][k0:k1].astype(np.int64),
                           lab=z["edge_labels"][k0:k1], pred=z["predictions"][k0:k1], part=z["id_pred"][v0:v1].astype(np.int64),
                           id_gt=z["id_gt"][v0:v1], metrics=z["metrics"][g]))
    return frames


@pytest.mark.parametrize("fixture", ["post2_eval_frames.npz", "post2_eval_partitions.npz"])
def test_fixtures_as_one_batch_and_as_single_frames(fixture):
    from gnn_cca_amd.evaluation import evaluate_frames
    frames = _fixture(fixture)
    b, pred, labels, _ = _batch(frames)
    rows, gt = evaluate_frames(b, pred, labels, gt_labels=True)
    rows, gt = rows.cpu().numpy(), gt.cpu().numpy()
    want = np.stack([f["metrics"] for f in frames])
    _check(rows[:, :14], want, fixture)
    for g, f in enumerate(frames):
        v0, v1 = b.node_ptr[g], b.node_ptr[g + 1]
        assert _same_partition(gt[v0:v1], f["id_gt"]), g
        assert np.all(gt[v0:v1] >= v0) and np.all(gt[v0:v1] <= np.arange(v0, v1)), g   # smallest-id convention
        assert rows[g, 14] == len(set(f["id_gt"].tolist())) and rows[g, 15] == len(set(f["part"].tolist())), g
    for g, f in enumerate(frames):
        bs, ps, ls, _ = _batch([f])
        one = evaluate_frames(bs, ps, ls).cpu().numpy()
        assert np.array_equal(one[0], rows[g], equal_nan=True), g


def _frames(rng, g, lo=0, hi=24, cams=4):
    sizes = rng.integers(lo, hi, size=g)
    if sizes.sum() == 0:
        sizes[0] = 6
    n = int(sizes.sum())
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, 2048)).astype(np.float32),
                reid=rng.standard_normal((n, 256)).astype(np.float32))


def _model(seed=0):
    import bench
    return bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=seed).cuda().eval()


def _shift_bias(m, f, node, reid):
    """Put the decision boundary inside the logits so that decisions vary (as tests/test_gpu_pipeline.py does)."""
    from gnn_cca_amd.graph_build import build_graph_batch
    b = build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    with torch.no_grad():
        med = m(b)["classified_edges"][-1].median()
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= med
        m.load_state_dict(sd)


def _restated(r, preds, labels):
    b = r.batch
    rows, _ = eo.eval_batch(b.edge_index.cpu().numpy(), b.edge_labels.cpu().numpy(), preds.cpu().numpy(), labels.cpu().numpy(),
                            b.node_ptr, b.edge_ptr)
    return rows


@pytest.mark.parametrize("g,seed", [(1, 2), (7, 3), (64, 1), (200, 4)])
def test_pipeline_evaluate_equals_the_restatement(g, seed):
    from gnn_cca_amd.pipeline import FramePipeline
    rng = np.random.default_rng(seed)
    f = _frames(rng, g, hi=24 if g < 200 else 20)
    m = _model()
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    _shift_bias(m, f, node, reid)
    pipe = FramePipeline(m)
    r = pipe(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    rows = r.evaluate()
    assert rows is r.evaluate() and rows.shape == (g, 16) and rows.dtype == torch.float64
    fin = r.final()
    _check(rows.cpu().numpy(), _restated(r, fin["predictions"], fin["labels"]), "final")
    chain = r.evaluate(final=False)
    _check(chain.cpu().numpy(), _restated(r, r.pruned, r.labels), "chain")
    assert float(rows[:, 3].sum() + rows[:, 4].sum() + rows[:, 5].sum() + rows[:, 6].sum()) == r.batch.edge_index.shape[1]
    pipe.close()


def test_step_by_step_batch_and_zero_edge_frames():
    from gnn_cca_amd.pipeline import FramePipeline
    rng = np.random.default_rng(9)
    m = _model()
    # frames of 0, 1 and single-camera detections (no edges) between ordinary ones
    f = _frames(rng, 12, hi=16)
    f["sizes"][[1, 4, 7]] = [0, 1, 5]
    n = int(f["sizes"].sum())
    f = dict(f, n=n, id_cam=rng.integers(0, 4, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n), yw=rng.uniform(-10, 10, n),
             node=rng.standard_normal((n, 2048)).astype(np.float32), reid=rng.standard_normal((n, 256)).astype(np.float32))
    starts = np.concatenate([[0], np.cumsum(f["sizes"])])
    f["id_cam"][starts[7]:starts[8]] = 2                           # one camera: no cross-camera edge in frame 7
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    _shift_bias(m, f, node, reid)
    pipe = FramePipeline(m)
    r = pipe(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    s = pipe._slow(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    for res in (r, s):
        fin = res.final()
        _check(res.evaluate().cpu().numpy(), _restated(res, fin["predictions"], fin["labels"]), "final")
        _check(res.evaluate(final=False).cpu().numpy(), _restated(res, res.pruned, res.labels), "chain")
    assert torch.equal(r.evaluate(), s.evaluate())
    ep = r.batch.edge_ptr
    assert ep[8] == ep[7] and ep[2] == ep[1]
    # a batch without a single edge still yields rows
    b, pred, labels, _ = _batch([dict(n=3, src=np.zeros(0, np.int64), dst=np.zeros(0, np.int64), lab=np.zeros(0), pred=np.zeros(0),
                                      part=np.array([0, 0, 1])), dict(n=0, src=np.zeros(0, np.int64), dst=np.zeros(0, np.int64),
                                                                       lab=np.zeros(0), pred=np.zeros(0), part=np.zeros(0, np.int64))])
    from gnn_cca_amd.evaluation import evaluate_frames
    rows = evaluate_frames(b, pred, labels).cpu().numpy()
    want = np.stack([eo.eval_frame([], [], [], [], [0, 0, 1], 3)[0], eo.eval_frame([], [], [], [], [], 0)[0]])
    _check(rows, want, "no edges")
    pipe.close()


def _random_batch(rng, sizes, k_frac=0.3, flip=0.2, neg=1.0):
    frames = []
    for n in sizes:
        ident = rng.integers(0, max(int(n * k_frac), 1), size=n)
        part = ident.copy()
        moved = rng.random(n) < flip
        part[moved] = rng.integers(0, n + 1, size=int(moved.sum())) + n
        src, dst, lab = [], [], []
        for c in np.unique(ident):
            mem = np.flatnonzero(ident == c)
            for v in mem[1:]:
                src += [mem[0], v]
                dst += [v, mem[0]]
                lab += [1, 1]
        for _ in range(int(neg * n)):
            a, c = rng.integers(0, n, size=2)
            if ident[a] != ident[c]:
                src += [a, c]
                dst += [c, a]
                lab += [0, 0]
        lab = np.array(lab, np.float32)
        frames.append(dict(n=int(n), src=np.array(src, np.int64), dst=np.array(dst, np.int64), lab=lab,
                           pred=(rng.random(len(lab)) < np.where(lab == 1, 0.8, 0.15)).astype(np.int64), part=part))
    return frames


def test_deterministic_and_graph_capturable():
    from gnn_cca_amd.evaluation import evaluate_frames
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 300, size=24)
    b, pred, labels, host = _batch(_random_batch(rng, sizes))
    a1, a2 = evaluate_frames(b, pred, labels), evaluate_frames(b, pred, labels)
    assert torch.equal(a1, a2)                                            # same bits
    _check(a1.cpu().numpy(), eo.eval_batch(*host)[0], "random")
    # capture on one stream, replay on new inputs of the same shape
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        evaluate_frames(b, pred, labels)                                  # warm-up outside the capture
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            static = evaluate_frames(b, pred, labels)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, a1)
    # new predictions and a new partition of the same nodes (another draw over the same frame sizes)
    _, _, labels2, _ = _batch(_random_batch(np.random.default_rng(4), sizes))
    pred.copy_((torch.rand(pred.shape, device=pred.device) < 0.4).to(torch.int64))
    labels.copy_(labels2)
    graph.replay()
    eager = evaluate_frames(b, pred, labels)
    torch.cuda.synchronize()
    assert torch.equal(static, eager) and not torch.equal(static, a1)
    _check(static.cpu().numpy(), eo.eval_batch(host[0], host[1], pred.cpu().numpy(), labels.cpu().numpy(), host[4], host[5])[0], "replay")


def test_accumulator_equals_main_py_aggregation():
    from gnn_cca_amd.evaluation import EvalAccumulator, evaluate_frames
    rng = np.random.default_rng(8)
    acc, want = EvalAccumulator(), []
    for g in (5, 17, 40):
        b, pred, labels, host = _batch(_random_batch(rng, rng.integers(0, 60, size=g)))
        acc.add(evaluate_frames(b, pred, labels))
        want.append(eo.eval_batch(*host)[0])
    got, ref = acc.result(), eo.aggregate(np.concatenate(want))
    assert sorted(got) == sorted(ref)
    for k, v in ref.items():
        if k in ("TP", "FP", "FN", "TN"):
            assert got[k] == v, k
        else:
            assert abs(got[k] - v) <= (1e-8 if k == "MI" else 1e-12) * max(1.0, abs(v)), k


def test_frame_of_4096_nodes_and_the_cap():
    from gnn_cca_amd.evaluation import evaluate_frames
    rng = np.random.default_rng(12)
    frames = _random_batch(rng, [4096], k_frac=0.1, flip=0.25, neg=0.5) + _random_batch(rng, [4096], k_frac=1.0, flip=0.3, neg=0.2)
    b, pred, labels, host = _batch(frames)
    rows, gt = evaluate_frames(b, pred, labels, gt_labels=True)
    want, want_gt = eo.eval_batch(*host)
    _check(rows.cpu().numpy(), want, "4096")
    assert np.array_equal(gt.cpu().numpy(), want_gt)
    big = _random_batch(rng, [4097], neg=0.1)
    b, pred, labels, _ = _batch(big)
    with pytest.raises(ValueError, match="at most 4096"):
        evaluate_frames(b, pred, labels)
