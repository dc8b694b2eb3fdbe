"""gnn_cca_amd.pipeline.FramePipeline(model, top_k=k, rank_by=...): a batch of frames from detections to identity clusters on a CAPPED
graph in one native call (gnncca_plan_frames_ex + gnncca_frames_forward_topk).  Every output must be BIT FOR BIT what the step-by-step
capped path gives -- graph_build.build_graph_batch(top_k=k) -> MOTMPNet.forward -> postprocess.threshold -> postprocess.prune_and_cluster
-- whose own correctness tests/test_gpu_graph_topk.py (the build, against its numpy definition) and the dense pipeline's tests pin.  No
tolerance anywhere: the same kernels on the same arguments.

In every case the median logit is first taken off the classifier's last bias, as tests/test_gpu_pipeline.py does, so that about half of the
edges are predicted active and the pruning has work to do."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_pipeline import _frames, _model, _same

pytestmark = pytest.mark.gpu
FIELDS = ("pruned", "flow_out", "flow_in", "labels", "n_clusters", "triggers")


def _dev(f):
    return torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()


def _stepwise(m, f, node, reid, **kw):
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.postprocess import prune_and_cluster, threshold
    b = build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid, **kw)
    with torch.no_grad():
        out = m(b)
    probs, preds = threshold(out["classified_edges"][-1])
    post = prune_and_cluster(b.edge_index, preds, b.x.shape[0], b.node_ptr_dev, b.edge_ptr_dev)
    return b, out, probs, preds, post


def _centre(m, f, node, reid, **kw):
    """Puts the decision boundary inside the logits of this batch's (capped) graph; returns the step-by-step result of the centred model."""
    ref = _stepwise(m, f, node, reid, **kw)
    with torch.no_grad():
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= ref[1]["classified_edges"][-1].median()
        m.load_state_dict(sd)
    return _stepwise(m, f, node, reid, **kw)


def _call(pipe, f, node, reid):
    return pipe(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)


def _as_ref(r):
    return r.batch, r.outputs, r.probs, r.preds, {k: getattr(r, k) for k in FIELDS}


def _degrees(f):
    """Cross-camera candidates of every detection in its own frame."""
    deg, v0 = [], 0
    for s in f["sizes"]:
        cam = f["id_cam"][v0:v0 + s]
        deg += [int(s - np.count_nonzero(cam == c)) for c in cam]
        v0 += s
    return np.asarray(deg, dtype=np.int64)


def _max_deg(f):
    return max(int(_degrees(f).max()), 1)


_cases = {}


def _case(g, seed, k, rank_by):
    """A batch, a model centred on its capped graph and the step-by-step capped result: computed once, shared, left unchanged."""
    key = (g, seed, k, rank_by)
    if key not in _cases:
        f = _frames(np.random.default_rng(seed), g)
        m = _model()
        node, reid = _dev(f)
        ref = _centre(m, f, node, reid, top_k=k, rank_by=rank_by)
        torch.cuda.synchronize()
        _cases[key] = dict(f=f, m=m, node=node, reid=reid, ref=ref)
    return _cases[key]


def _mutual_pair_conditions(r):
    """The conditions that keep a comparison from passing on an empty result (g = 64 cases)."""
    ei = r.batch.edge_index.cpu().numpy()
    preds, pruned = r.preds.cpu().numpy().astype(bool), r.pruned.cpu().numpy().astype(bool)
    assert 0 < pruned.sum() < preds.sum()
    index = {(s, d): q for q, (s, d) in enumerate(ei.T.tolist())}
    for s, d in ei.T[pruned].tolist():      # a surviving edge's reverse is in the list and survives too
        assert (d, s) in index and pruned[index[(d, s)]], (s, d)
    one_way = [q for q in np.flatnonzero(preds) if (int(ei[1][q]), int(ei[0][q])) not in index]
    assert len(one_way) >= 1 and not pruned[one_way].any()      # a predicted-active edge without a reverse in the list was pruned away


@pytest.mark.parametrize("g,seed,k,rank_by", [(64, 1, 3, "ground"), (64, 1, 8, "reid"), (1, 2, 1, "reid"), (7, 3, 3, "ground")])
def test_one_call_equals_the_step_by_step_capped_path(g, seed, k, rank_by):
    from gnn_cca_amd.pipeline import FramePipeline
    c = _case(g, seed, k, rank_by)
    b = c["ref"][0]
    deg = _degrees(c["f"])
    assert 0 < b.edge_index.shape[1] == int(np.minimum(deg, k).sum()) < int(deg.sum())      # the cap bites
    pipe = FramePipeline(c["m"], top_k=k, rank_by=rank_by)
    for _ in range(3):                       # repeated calls: staging ring, workspace reuse
        r = _call(pipe, c["f"], c["node"], c["reid"])
    torch.cuda.synchronize()
    assert r._d2h is not None                # the one-call path, not the fallback
    _same(r, c["ref"])
    if g == 64:
        _mutual_pair_conditions(r)


def test_reid_ranking_on_a_ground_only_model():
    """edge_in_dim = 2 with only_dist=True: the reid table is read for the ranking alone."""
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    params = copy.deepcopy(bench.graph_net_params(L=4))
    params["encoder_feats_dict"]["edges"]["edge_in_dim"] = 2
    m = bench.build_model(params, 20, seed=0).cuda().eval()
    f = _frames(np.random.default_rng(3), 7)
    node, reid = _dev(f)
    kw = dict(top_k=3, rank_by="reid", only_dist=True)
    ref = _centre(m, f, node, reid, **kw)
    by_ground = _stepwise(m, f, node, reid, top_k=3, rank_by="ground", only_dist=True)
    assert not torch.equal(ref[0].edge_index, by_ground[0].edge_index)      # the ranking key matters on this batch
    pipe = FramePipeline(m, only_dist=True, top_k=3, rank_by="reid")
    for _ in range(2):
        r = _call(pipe, f, node, reid)
    torch.cuda.synchronize()
    assert r._d2h is not None and r.batch.edge_attr.shape[1] == 2
    _same(r, ref)


@pytest.mark.parametrize("g,seed", [(7, 3), (64, 1)])
def test_a_cap_no_source_reaches_is_the_dense_pipeline(g, seed):
    from gnn_cca_amd.pipeline import FramePipeline
    f = _frames(np.random.default_rng(seed), g)
    m = _model()
    node, reid = _dev(f)
    _centre(m, f, node, reid)
    dense = _call(FramePipeline(m), f, node, reid)
    torch.cuda.synchronize()
    want = _as_ref(dense)
    for k in (_max_deg(f), 10 ** 6):
        for rank_by in ("ground", "reid"):
            r = _call(FramePipeline(m, top_k=k, rank_by=rank_by), f, node, reid)
            torch.cuda.synchronize()
            assert r._d2h is not None
            _same(r, want)


@pytest.mark.parametrize("k,e", [(5, 750), (70, 10500)])
def test_candidates_beyond_one_64_slot_chunk(k, e):
    """One frame of 150 detections on three cameras: 100 candidates per source, two LDS chunks; 15 000 edges dense."""
    from gnn_cca_amd.pipeline import FramePipeline
    rng = np.random.default_rng(11)
    n = 150
    f = dict(sizes=np.array([n]), n=n, id_cam=np.arange(n) % 3, ids=rng.integers(0, 11, size=n), xw=rng.uniform(-20, 20, n),
             yw=rng.uniform(-20, 20, n), max_dist=np.array([60.0]), node=rng.standard_normal((n, 2048)).astype(np.float32),
             reid=rng.standard_normal((n, 256)).astype(np.float32))
    m = _model()
    node, reid = _dev(f)
    ref = _centre(m, f, node, reid, top_k=k)
    assert ref[0].edge_index.shape == (2, e)
    r = _call(FramePipeline(m, top_k=k), f, node, reid)
    torch.cuda.synchronize()
    assert r._d2h is not None
    _same(r, ref)


def _first_frame_on_one_camera():
    f = _frames(np.random.default_rng(8), 6, lo=6, hi=12)
    f["id_cam"] = f["id_cam"].copy()
    f["id_cam"][:int(f["sizes"][0])] = 0      # the first sources (the first waves of the launch) have no candidate
    return f


@pytest.mark.parametrize("batch", ["g7_seed3", "first_frame_on_one_camera"])
def test_stale_counters_are_zeroed_by_the_capped_build(batch, monkeypatch):
    """The chain has no memset: the capped build kernel zeroes flow_out | flow_in | n_clusters | sizes | triggers.  An arena that arrives
    full of ones (then of zeros) must give the step-by-step result -- also where the launch's first waves have no candidate and return early."""
    from gnn_cca_amd.pipeline import FramePipeline
    if batch == "g7_seed3":
        c = _case(7, 3, 3, "ground")
        f, m, node, reid, ref = c["f"], c["m"], c["node"], c["reid"], c["ref"]
    else:
        f = _first_frame_on_one_camera()
        m = _model()
        node, reid = _dev(f)
        ref = _centre(m, f, node, reid, top_k=3)
        assert ref[0].edge_ptr[1] == 0 and ref[0].edge_index.shape[1] > 0
    pipe = FramePipeline(m, top_k=3)
    made = []
    for byte in (0xFF, 0x00):
        def arena(self, nbytes, device, byte=byte):
            made.append(byte)
            return torch.full((nbytes,), byte, dtype=torch.uint8, device=device)
        monkeypatch.setattr(FramePipeline, "_arena", arena)
        r = _call(pipe, f, node, reid)
        torch.cuda.synchronize()
        assert r._d2h is not None
        _same(r, ref)
    assert made == [0xFF, 0x00]


def test_fallbacks_carry_the_cap():
    """More than 4096 detections, a hooked model, a batch without any cross-camera pair and shapes alternating through one pipeline object:
    all with top_k = 3, all equal to the step-by-step capped path; a source with more than 4096 candidates is refused before any launch."""
    from gnn_cca_amd.pipeline import FramePipeline
    rng = np.random.default_rng(9)
    m = _model(seed=1)
    pipe = FramePipeline(m, top_k=3)
    f = _frames(rng, 30)
    node, reid = _dev(f)
    _centre(m, f, node, reid, top_k=3)
    for g in (30, 3, 90, 30):
        f = _frames(rng, g)
        node, reid = _dev(f)
        r = _call(pipe, f, node, reid)
        assert r._d2h is not None
        _same(r, _stepwise(m, f, node, reid, top_k=3))
    # one camera only: no edges
    f = _frames(rng, 5, lo=3, hi=9, cams=1)
    node, reid = _dev(f)
    r = _call(pipe, f, node, reid)
    assert r.batch.edge_index.shape == (2, 0) and int(r.n_clusters.item()) == f["n"]
    _same(r, _stepwise(m, f, node, reid, top_k=3))
    # beyond the one-launch normalisation's 4096 rows
    f = _frames(rng, 260, lo=14, hi=20)
    assert f["n"] > 4096
    node, reid = _dev(f)
    r = _call(pipe, f, node, reid)
    want = _stepwise(m, f, node, reid, top_k=3)
    assert r._d2h is None and r.batch.edge_index.shape[1] == int(np.minimum(_degrees(f), 3).sum())
    _same(r, want)
    # a hooked model
    f = _frames(rng, 12)
    node, reid = _dev(f)
    seen = []
    hook = m.encoder.register_forward_hook(lambda mod, i, o: seen.append(1))
    r = _call(pipe, f, node, reid)
    want = _stepwise(m, f, node, reid, top_k=3)
    hook.remove()
    assert r._d2h is None and len(seen) == 2
    _same(r, want)
    # one source with 4097 candidates
    n = 4098
    cam = np.array([0] + [1] * 4097)
    emb = torch.zeros((n, 2048), device="cuda"), torch.zeros((n, 256), device="cuda")
    with pytest.raises(NotImplementedError):
        pipe(np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64), cam, np.array([n]), np.array([10.0]), *emb)


def test_the_host_pass_and_the_metrics_work_on_the_capped_batch():
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.postprocess import finalize
    from oracle import post_oracle as po
    c = _case(64, 1, 3, "ground")
    pipe = FramePipeline(c["m"], top_k=3)
    r = _call(pipe, c["f"], c["node"], c["reid"])
    got = r.final_async().result()
    b = r.batch
    want = finalize(b.edge_index, r.probs, r.pruned, r.labels, r.n_clusters, r.triggers, b.node_ptr, b.edge_ptr)
    assert np.array_equal(got["predictions"], want["predictions"].cpu().numpy())
    assert np.array_equal(got["labels"], want["labels"].cpu().numpy())
    assert got["n_clusters"] == int(want["n_clusters"].item()) and got["frames_finalized"] == want["frames_finalized"]
    fin = r.final()
    assert fin is r.final()
    assert torch.equal(fin["predictions"], want["predictions"]) and torch.equal(fin["labels"], want["labels"])
    assert int(fin["n_clusters"].item()) == got["n_clusters"]
    # frame by frame: the oracle's restatement of the reference's heuristics on the GPU's own probabilities
    ei, probs = b.edge_index.cpu().numpy(), r.probs.cpu().numpy()
    got_pred, got_lab, trig, pruned = fin["predictions"].cpu().numpy(), fin["labels"].cpu().numpy(), r.triggers.cpu().numpy(), r.pruned.cpu().numpy()
    total = 0
    for q in range(len(b.node_ptr) - 1):
        v0, v1, k0, k1 = b.node_ptr[q], b.node_ptr[q + 1], b.edge_ptr[q], b.edge_ptr[q + 1]
        _, pred_q, ids, k = po.finalize(ei[:, k0:k1] - v0, None, v1 - v0, probs=probs[k0:k1])
        assert np.array_equal(got_pred[k0:k1], pred_q), q
        assert po.same_partition(got_lab[v0:v1], ids), q
        total += k
        assert not (not np.array_equal(pred_q, pruned[k0:k1]) and trig[q] == 0), q      # a frame the heuristics change raises a trigger
    assert int(fin["n_clusters"].item()) == total
    assert fin["frames_finalized"] == [q for q in range(len(trig)) if trig[q]]
    # the metrics score the kept edges
    sb, post = c["ref"][0], c["ref"][4]
    rows = r.evaluate(final=False)
    assert rows.shape == (64, 16) and torch.equal(rows, evaluate_frames(sb, post["pruned"], post["labels"]))
    assert torch.equal(r.evaluate(final=True), evaluate_frames(b, fin["predictions"], fin["labels"]))
    del got, fin, r
    pipe.close()


@pytest.mark.parametrize("route", ["generic_fused", "max_aggregation"])
def test_plan_handover_on_other_forward_routes(route):
    """The pruning reads the CSR plan the forward left in its workspace: carve_generic (node latent 48) and the general step kernel (max
    aggregation) on a capped plan."""
    import bench
    from gnn_cca_amd import MOTMPNet
    from gnn_cca_amd.pipeline import FramePipeline
    params = copy.deepcopy(bench.graph_net_params(L=4))
    if route == "generic_fused":
        params["encoder_feats_dict"]["nodes"]["resnet50"]["node_out_dim"] = 48
        params["node_model_feats_dict"]["fc_dims"] = [48]
    else:
        params["node_agg_fn"] = "max"
    torch.manual_seed(3)
    m = MOTMPNet(copy.deepcopy(params), None, "resnet50")
    with torch.no_grad():
        for p in m.MPNet.node_model.node_mlp.parameters():
            p.mul_(1.0 / 20)
    m = m.cuda().eval()
    f = _frames(np.random.default_rng(5), 24)
    node, reid = _dev(f)
    ref = _centre(m, f, node, reid, top_k=3)
    pipe = FramePipeline(m, top_k=3)
    for _ in range(2):
        r = _call(pipe, f, node, reid)
    torch.cuda.synchronize()
    assert r._d2h is not None
    _same(r, ref)
    assert 0 < int(r.pruned.sum().item()) < r.pruned.numel()


def test_scattered_target_ids_stream_the_columns():
    """A capped list is the first graph built in the package whose target ids per source are not two runs: with column_ranges on, the
    forward must notice (state 1) and give the streaming path's bits."""
    from gnn_cca_amd.pipeline import FramePipeline
    c = _case(64, 1, 3, "ground")
    m = c["m"]
    pipe = FramePipeline(m, top_k=3)
    try:
        m.column_ranges = True
        r = _call(pipe, c["f"], c["node"], c["reid"])
        logits = [t.clone() for t in r.outputs["classified_edges"]]
        state = m.column_ranges_state()
    finally:
        m.column_ranges = False
    r = _call(pipe, c["f"], c["node"], c["reid"])
    torch.cuda.synchronize()
    assert len(logits) == len(r.outputs["classified_edges"])
    for a, b in zip(logits, r.outputs["classified_edges"]):
        assert torch.equal(a, b)
    assert state == 1
    _same(r, c["ref"])
