"""gnn_cca_amd.pipeline.FramePipeline(model, radius=r, radius_unit=...): a batch of frames from detections to identity clusters on a
RADIUS-GATED graph in one native call (gnncca_plan_frames_radius + gnncca_frames_forward_radius).  Every output must be BIT FOR BIT what
the step-by-step gated path gives -- graph_build.build_graph_batch(radius=r) -> MOTMPNet.forward -> postprocess.threshold ->
postprocess.prune_and_cluster -- whose build tests/test_gpu_graph_radius.py pins against the numpy definition.  No tolerance anywhere: the
same kernels on the same arguments.

The batch: 8 consecutive frames of the real-geometry fixture (tests/golden/terrace_geometry.npz: cameras, identities and ground-plane
positions of the EPFL-Terrace annotations) at r = 80, the reference's GEOM_TH for that sequence; embeddings are synthetic.  The median
logit is first taken off the classifier's last bias, as tests/test_gpu_pipeline.py does, so that the pruning has work to do."""
import numpy as np
import pytest
import torch

import graph_radius_oracle as gro
from test_gpu_pipeline import _model, _same
from test_gpu_pipeline_topk import _as_ref, _call, _centre, _dev, _stepwise

pytestmark = pytest.mark.gpu
RADIUS = 80.0
_cases = {}


def terrace_frames(first=500, g=8, seed=0):
    """Frames first .. first + g of the fixture in the shape test_gpu_pipeline._frames gives."""
    t = gro.terrace()
    rng = np.random.default_rng(seed)
    v0, v1 = int(t["node_ptr"][first]), int(t["node_ptr"][first + g])
    n = v1 - v0
    return dict(sizes=t["graph_sizes"][first:first + g].copy(), n=n, id_cam=t["id_cam"][v0:v1].copy(), ids=t["id"][v0:v1].copy(),
                xw=t["xw"][v0:v1].copy(), yw=t["yw"][v0:v1].copy(), max_dist=np.full(g, 100.0),
                node=rng.standard_normal((n, 2048)).astype(np.float32), reid=rng.standard_normal((n, 256)).astype(np.float32))


def case():
    """The batch, a model centred on its gated graph and the step-by-step gated result: computed once, shared, left unchanged."""
    if not _cases:
        f = terrace_frames()
        m = _model()
        node, reid = _dev(f)
        ref = _centre(m, f, node, reid, radius=RADIUS)
        dense = _stepwise(m, f, node, reid)
        torch.cuda.synchronize()
        _cases.update(f=f, m=m, node=node, reid=reid, ref=ref, dense=dense)
    return _cases


@pytest.fixture
def entries(monkeypatch):
    """Records which gnncca_frames_forward* entry a pipeline call reaches."""
    from gnn_cca_amd import _native as nat
    lib, seen = nat.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name.startswith("gnncca_frames_forward"):
                def wrapped(*a, _fn=fn, _name=name):
                    seen.append(_name)
                    return _fn(*a)
                return wrapped
            return fn
    spy = Spy()
    import gnn_cca_amd.pipeline as pl
    monkeypatch.setattr(pl.nat, "lib", lambda: spy)
    return seen


def test_one_call_equals_the_step_by_step_gated_path(entries):
    from gnn_cca_amd.pipeline import FramePipeline
    c = case()
    b, dense = c["ref"][0], c["dense"][0]
    assert 0 < b.edge_index.shape[1] < dense.edge_index.shape[1]      # the gate bites
    pipe = FramePipeline(c["m"], radius=RADIUS)
    for _ in range(3):                       # repeated calls: staging ring, workspace reuse
        r = _call(pipe, c["f"], c["node"], c["reid"])
    torch.cuda.synchronize()
    assert entries == ["gnncca_frames_forward_radius"] * 3 and r._d2h is not None      # the one-call path, through its own entry
    _same(r, c["ref"])
    assert 0 < int(r.pruned.sum().item()) < r.pruned.numel()
    # in the 'max_dist' unit the same gate is 0.8 x max_dist = 100
    r2 = _call(FramePipeline(c["m"], radius=0.8, radius_unit="max_dist"), c["f"], c["node"], c["reid"])
    torch.cuda.synchronize()
    assert entries[-1] == "gnncca_frames_forward_radius"
    _same(r2, c["ref"])


def test_radius_inf_is_the_dense_pipeline():
    from gnn_cca_amd.pipeline import FramePipeline
    c = case()
    dense = _call(FramePipeline(c["m"]), c["f"], c["node"], c["reid"])
    r = _call(FramePipeline(c["m"], radius=float("inf")), c["f"], c["node"], c["reid"])
    torch.cuda.synchronize()
    assert r._d2h is not None
    _same(r, _as_ref(dense))
    _same(r, c["dense"])


def test_stale_counters_are_zeroed_by_the_gated_build(monkeypatch):
    """The chain has no memset: the gated build kernel zeroes flow_out | flow_in | n_clusters | sizes | triggers."""
    from gnn_cca_amd.pipeline import FramePipeline
    c = case()
    pipe = FramePipeline(c["m"], radius=RADIUS)
    for byte in (0xFF, 0x00):
        def arena(self, nbytes, device, byte=byte):
            return torch.full((nbytes,), byte, dtype=torch.uint8, device=device)
        monkeypatch.setattr(FramePipeline, "_arena", arena)
        r = _call(pipe, c["f"], c["node"], c["reid"])
        torch.cuda.synchronize()
        assert r._d2h is not None
        _same(r, c["ref"])


def test_capture_and_replay(monkeypatch):
    """The whole one-call chain inside a HIP graph: nothing on the path waits for the device; replays give the eager bits."""
    from gnn_cca_amd import frames
    from gnn_cca_amd.pipeline import FramePipeline
    c = case()
    monkeypatch.setattr(frames, "_staging", {})      # an event recorded during a capture must not be waited on by a later, eager batch
    node, reid = c["node"].clone(), c["reid"].clone()
    pipe = FramePipeline(c["m"], radius=RADIUS)
    for _ in range(frames._Staging.SLOTS):      # every slot of the ring, the packed weights and the workspace exist before the capture
        _call(pipe, c["f"], node, reid)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _call(pipe, c["f"], node, reid)
    assert static._d2h is not None
    gen = torch.Generator().manual_seed(3)
    for k in range(2):
        if k:
            node.copy_(torch.randn(node.shape, generator=gen))
            reid.copy_(torch.randn(reid.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        got = {name: getattr(static, name).clone() for name in ("probs", "preds", "pruned", "labels", "n_clusters", "triggers")}
        got["logits"] = static.outputs["classified_edges"][-1].clone()
        got["edge_index"], got["edge_attr"] = static.batch.edge_index.clone(), static.batch.edge_attr.clone()
        eager = _call(pipe, c["f"], node, reid)
        torch.cuda.synchronize()
        if k == 0:
            _same(eager, c["ref"])
        want = {name: getattr(eager, name) for name in ("probs", "preds", "pruned", "labels", "n_clusters", "triggers")}
        want["logits"] = eager.outputs["classified_edges"][-1]
        want["edge_index"], want["edge_attr"] = eager.batch.edge_index, eager.batch.edge_attr
        for name in got:
            assert torch.equal(got[name], want[name]), (k, name)


def test_the_result_serves_the_rest_of_the_stack():
    """.final(), .exclusive(), .evaluate(), .evaluate(against='dense'), .sweep(), .rank_metrics() and .identities() on a gated batch."""
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.pipeline import FramePipeline
    c = case()
    f, g, n = c["f"], 8, c["f"]["n"]
    pipe = FramePipeline(c["m"], radius=RADIUS)
    r = _call(pipe, f, c["node"], c["reid"])
    b, e = r.batch, r.batch.edge_index.shape[1]
    fin = r.final()
    assert fin["predictions"].shape == (e,) and fin["labels"].shape == (n,)
    ex = r.exclusive()
    assert ex["predictions"].shape == (e,) and ex["labels"].shape == (n,)
    rows = r.evaluate(final=False)
    assert rows.shape == (g, 16) and torch.equal(rows, evaluate_frames(c["ref"][0], c["ref"][4]["pruned"], c["ref"][4]["labels"]))
    assert torch.equal(r.evaluate(), evaluate_frames(b, fin["predictions"], fin["labels"]))
    assert r.sweep([0.3, 0.5, 0.7]).shape == (3, g, 16) and torch.equal(r.sweep([0.5])[0], rows)
    assert r.rank_metrics().shape[:2] == (1, g)
    ident = r.identities()
    assert ident is r.identities() and ident is not None
    # against='dense': the rows of a dense run whose dropped edges are predicted 0 -- built here from the dense batch
    dense = c["dense"][0]
    ei_d, ei_k = dense.edge_index.cpu().numpy(), b.edge_index.cpu().numpy()
    _, keep = gro.keep_mask(f["xw"], f["yw"], f["id_cam"], f["sizes"], f["max_dist"], RADIUS, ei=ei_d)
    assert np.array_equal(ei_d[:, keep], ei_k)
    where = torch.from_numpy(np.flatnonzero(keep)).cuda()
    for final, preds, labels in ((False, r.pruned, r.labels), (True, fin["predictions"], fin["labels"])):
        as_dense = torch.zeros(ei_d.shape[1], dtype=preds.dtype, device="cuda")
        as_dense[where] = preds
        want = evaluate_frames(dense, as_dense, labels)
        got = r.evaluate(final=final, against="dense")
        torch.cuda.synchronize()
        assert got.shape == (g, 16) and torch.equal(got, want), final
    assert not torch.equal(r.evaluate(final=False, against="dense"), rows)      # the gate dropped a same-identity pair or changed a denominator
    del fin, r
    pipe.close()


def test_a_gate_that_keeps_nothing_and_the_fallbacks():
    """E = 0: empty per-edge outputs and singleton clusters; a hooked model and a non-default threshold take the step-by-step path with the
    gate carried along."""
    from gnn_cca_amd.pipeline import FramePipeline
    c = case()
    f, m = c["f"], c["m"]
    r = _call(FramePipeline(m, radius=1e-9), f, c["node"], c["reid"])
    torch.cuda.synchronize()
    assert r.batch.edge_index.shape == (2, 0) and r.probs.shape == (0,) and r.pruned.shape == (0,) and r.preds.shape == (0,)
    assert int(r.n_clusters.item()) == f["n"] and r.labels.unique().numel() == f["n"]
    assert r.evaluate(final=False).shape == (8, 16)
    _same(r, _stepwise(m, f, c["node"], c["reid"], radius=1e-9))
    seen = []
    hook = m.encoder.register_forward_hook(lambda mod, i, o: seen.append(1))
    try:
        r = _call(FramePipeline(m, radius=RADIUS), f, c["node"], c["reid"])
    finally:
        hook.remove()
    assert r._d2h is None and seen
    _same(r, c["ref"])
    r = _call(FramePipeline(m, radius=RADIUS, threshold=0.4), f, c["node"], c["reid"])
    assert r._d2h is None and torch.equal(r.batch.edge_index, c["ref"][0].edge_index)
