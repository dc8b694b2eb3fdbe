"""gnn_cca_amd.pipeline.FramePipeline(model, top_k=k, symmetric='union' | 'mutual'): the pipeline on a capped graph closed under reversal.
Such a pipeline takes the step-by-step path (E depends on the data), so every output must be BIT FOR BIT what
graph_build.build_graph_batch(top_k=k, symmetric=m) -> MOTMPNet.forward -> postprocess.threshold -> postprocess.prune_and_cluster give;
the build itself is pinned by tests/test_gpu_graph_sym.py."""
import numpy as np
import pytest
import torch

from test_gpu_pipeline import _frames, _model, _same
from test_gpu_pipeline_topk import _call, _centre, _dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["union", "mutual"])
@pytest.mark.parametrize("rank_by", ["ground", "reid"])
def test_pipeline_equals_the_step_by_step_symmetric_path(rank_by, mode):
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    f = _frames(np.random.default_rng(3), 7)
    m = _model()
    node, reid = _dev(f)
    kw = dict(top_k=3, rank_by=rank_by, symmetric=mode)
    ref = _centre(m, f, node, reid, **kw)
    directed = build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid, top_k=3,
                                 rank_by=rank_by).edge_index.shape[1]
    e = ref[0].edge_index.shape[1]
    assert (e > directed) if mode == "union" else (0 < e < directed)      # one-way edges exist: the closure changes the graph
    pipe = FramePipeline(m, **kw)
    for _ in range(2):
        r = _call(pipe, f, node, reid)
    torch.cuda.synchronize()
    assert r._d2h is None      # the step-by-step path
    _same(r, ref)
    # every edge of the batch has its reverse in the batch, so pruning never meets an edge that cannot have an active reverse
    ei = r.batch.edge_index.cpu().numpy()
    have = set(map(tuple, ei.T.tolist()))
    assert all((d, s) in have for s, d in have)
    preds, pruned = r.preds.cpu().numpy().astype(bool), r.pruned.cpu().numpy().astype(bool)
    assert 0 < pruned.sum() <= preds.sum()
    fin = r.final()
    assert fin["predictions"].shape == (e,) and fin["labels"].shape == (len(f["id_cam"]),)
    rows = r.evaluate()
    torch.cuda.synchronize()
    assert rows.shape == (len(f["sizes"]), 16) and bool(torch.isfinite(rows).all())
