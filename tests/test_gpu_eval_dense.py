"""evaluate_frames(against='dense') on the GPU (gnncca_eval_frames_dense, csrc/evaluate.hip): a capped batch scored as the dense graph with
every dropped edge predicted 0 must give the rows of evaluate_frames(dense batch, the capped predictions scattered into the dense edge
list).  Both sides run the same kernel arithmetic on the same counts and the same partitions, so the counts, P, R, F, the two precisions,
ARI and the cluster counts are compared bit for bit; homogeneity / completeness / V within 1e-12 and AMI within 1e-9, the agreements
gnn_cca_amd.evaluation states for its own arithmetic.  The numpy oracle (tests/helpers/graph_sym_oracle.py) pins the scattering itself."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_graph_topk import build, dense
from test_graph_sym_oracle import EVAL_CASES, EVAL_KS, case
from test_graph_topk_oracle import load

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import eval_oracle as eo  # noqa: E402
import graph_sym_oracle as gso  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {8: 1e-9, 9: 1e-12, 10: 1e-12, 11: 1e-12}      # AMI, homogeneity, completeness, V; every other column exactly


def _check(got, want, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, where
    for q in range(want.shape[1]):
        if q in TOL:
            err = np.abs(got[:, q] - want[:, q]).max(initial=0.0)
            print(where, eo.COLUMNS[q], "max abs difference", err)
            assert err <= TOL[q], (where, eo.COLUMNS[q], err)
        else:
            assert np.array_equal(got[:, q], want[:, q]), (where, eo.COLUMNS[q], got[:, q], want[:, q])


@pytest.mark.parametrize("mode", [None, "union"])
@pytest.mark.parametrize("k", EVAL_KS)
@pytest.mark.parametrize("name", EVAL_CASES)
def test_capped_against_dense_equals_the_dense_batch_with_scattered_predictions(name, k, mode):
    from gnn_cca_amd.evaluation import evaluate_frames
    a, c, full = load(name), case(name), dense(name)
    keep = c.keep(k, "ground", mode)
    capped = build(a, top_k=k, rank_by="ground", symmetric=mode)
    assert np.array_equal(capped.edge_index.cpu().numpy(), c.ei[:, keep]) and not keep.all()
    pred, labels = gso.random_outcome(c, keep, seed=7)
    pred_dev, labels_dev = torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda()
    scattered = torch.from_numpy(gso.scatter(keep, pred)).cuda()
    got, got_gt = evaluate_frames(capped, pred_dev, labels_dev, gt_labels=True, against="dense")
    want, want_gt = evaluate_frames(full, scattered, labels_dev, gt_labels=True)
    torch.cuda.synchronize()
    where = f"{name} k={k} {mode}"
    _check(got.cpu().numpy(), want.cpu().numpy(), where)
    assert torch.equal(got_gt, want_gt), where
    # the numpy oracle of the same definition: the exact columns and the partition
    rows, gt = gso.score_against_dense(c, keep, pred, labels)
    exact = [q for q in range(16) if q not in TOL]
    assert np.array_equal(got.cpu().numpy()[:, exact], rows[:, exact]) and np.array_equal(got_gt.cpu().numpy(), gt), where
    # and the default still scores the kept edges alone
    kept = evaluate_frames(capped, pred_dev, labels_dev).cpu().numpy()
    assert np.array_equal(kept[:, [3, 4]], rows[:, [3, 4]]) and kept[:, 5:7].sum() < rows[:, 5:7].sum(), where


@pytest.mark.parametrize("name", EVAL_CASES)
def test_on_a_dense_batch_it_is_the_default(name):
    from gnn_cca_amd.evaluation import evaluate_frames
    c, full = case(name), dense(name)
    pred, labels = gso.random_outcome(c, np.ones(c.ei.shape[1], bool), seed=9)
    pred_dev, labels_dev = torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda()
    a, a_gt = evaluate_frames(full, pred_dev, labels_dev, gt_labels=True)
    b, b_gt = evaluate_frames(full, pred_dev, labels_dev, gt_labels=True, against="dense")
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a_gt, b_gt)
    assert full.person_dev.dtype == torch.int32 and full.person_dev.shape == full.cam_dev.shape == (c.node_ptr[-1],)
    assert np.array_equal(full.cam_dev.cpu().numpy(), np.asarray(c.a["id_cam"]))


def test_frame_result_passes_the_option_through():
    from test_gpu_pipeline import _frames, _model
    from test_gpu_pipeline_topk import _call, _centre, _dev
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.pipeline import FramePipeline
    f = _frames(np.random.default_rng(3), 7)
    m = _model()
    node, reid = _dev(f)
    _centre(m, f, node, reid, top_k=3)
    for kw in (dict(top_k=3), dict(top_k=3, symmetric="union")):      # the one-call path and the step-by-step one
        r = _call(FramePipeline(m, **kw), f, node, reid)
        for final in (False, True):
            pred, labels = (r.final()["predictions"], r.final()["labels"]) if final else (r.pruned, r.labels)
            want = evaluate_frames(r.batch, pred, labels, against="dense")
            got, kept = r.evaluate(final=final, against="dense"), r.evaluate(final=final)
            torch.cuda.synchronize()
            assert torch.equal(got, want) and r.evaluate(final=final, against="dense") is got
            assert torch.equal(kept, evaluate_frames(r.batch, pred, labels)) and not torch.equal(kept, got)
        with pytest.raises(ValueError):
            r.evaluate(against="full")
