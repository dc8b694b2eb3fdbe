#!/usr/bin/env python3
"""Golden vectors for the per-frame scoring of the reference's evaluation loop (inference.py:349-371) -- gnn_cca_amd.evaluation.

As tests/golden/make_golden_post2.py does for the heuristics, this script READS the reference's lines at run time and executes them
unmodified: `compute_P_R_F` (inference.py:23-68) and the loop body from the model call to the appended metrics (inference.py:283-371),
with `mpn_model` a stand-in that returns the case's logits, `data_batch.edge_labels` the ground truth from the case's identities and
`metrics` the installed scikit-learn (1.7.2 when these files were made; the reference pins 0.24.2).  The reference's `libs.utils` is
imported unmodified (cv2 / torch_scatter stand-ins).  Only numbers are stored:

  post2_eval_frames.npz      ~30 frames through the shipped ROUNDING / PRUNING / SPLITTING sequence: per-frame edges, GT edge labels, final
                             predictions, ID_GT, ID_pred and the 14 metric values the loop appends
  post2_eval_partitions.npz  scikit-learn on synthetic partitions (0 / 1 / 2 nodes, no edges, one GT cluster, all-singleton predictions,
                             identical partitions, noisy partitions of 34 ... 4096 nodes); GT = symmetric star edges per identity plus
                             negative edges, so the GT partition comes out of the edges

Build container only:

    python tests/golden/make_golden_eval.py
"""
import os
import sys
import textwrap
import types

import networkx as nx
import numpy as np
import torch
from sklearn import metrics

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_torch_scatter_standin, cross_camera_edges  # noqa: E402

REF_FILE = "/root/reference/inference.py"
PRF_LINES = (23, 68)      # def compute_P_R_F
LOOP_LINES = (283, 371)   # outputs = mpn_model(data_batch) ... TN_list.append(TN)
LISTS = ("rand_index", "precision_1_list", "precision_0_list", "mutual_index", "homogeneity", "completeness", "v_measure", "TP_list",
         "FP_list", "FN_list", "P_list", "R_list", "F_list", "TN_list")
# the 14 values in the order of gnn_cca_amd.evaluation.METRICS[:14]
ORDER = ("P_list", "R_list", "F_list", "TP_list", "FP_list", "FN_list", "TN_list", "rand_index", "mutual_index", "homogeneity",
         "completeness", "v_measure", "precision_0_list", "precision_1_list")


def _lines(first, last):
    with open(REF_FILE) as f:
        return textwrap.dedent("".join(f.readlines()[first - 1:last]))


class Batch:
    pass


def run_reference(utils, n, ei, gt_labels, logits):
    b = Batch()
    b.edge_index = torch.from_numpy(ei)
    b.num_nodes = n
    b.edge_labels = torch.from_numpy(gt_labels.astype(np.float32))
    ns = {"np": np, "torch": torch, "nx": nx, "utils": utils, "metrics": metrics, "data_batch": b,
          "CONFIG": {"ROUNDING": True, "PRUNING": True, "SPLITTING": True},
          "mpn_model": lambda batch: {"classified_edges": [torch.from_numpy(logits).view(-1, 1)]}}
    ns.update({k: [] for k in LISTS})
    exec(compile(_lines(*PRF_LINES), "<reference inference.py:23-68>", "exec"), ns)
    exec(compile(_lines(*LOOP_LINES), "<reference inference.py:283-371>", "exec"), ns)
    pred = ns["predictions"]
    pred = pred.cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
    vals = np.array([float(ns[k][0]) for k in ORDER], dtype=np.float64)
    return pred.astype(np.int64).reshape(-1), np.asarray(ns["ID_GT"]).astype(np.int64), np.asarray(ns["ID_pred"]).astype(np.int64), vals


def frames_fixture(utils):
    cases = []
    for cams, seeds in (([8, 8, 8, 8], range(0, 8)), ([5, 5, 5, 5], range(8, 14)), ([3, 4, 2, 5, 3, 4], range(14, 20)),
                        ([3] * 5, range(20, 25)), ([12, 10, 14, 9], range(25, 30)), ([1, 1], range(30, 31))):
        for s in seeds:
            r = np.random.default_rng(500 + s)
            n, ei = cross_camera_edges(cams)
            ident = r.integers(0, max(n // 3, 2), size=n)
            gt = (ident[ei[0]] == ident[ei[1]]).astype(np.int64)
            lg = (np.where(gt == 1, 2.0, -2.5) + r.normal(0, 1.8, size=ei.shape[1])).astype(np.float32)
            cases.append((n, ei, gt, lg))
    node_ptr, edge_ptr = [0], [0]
    src, dst, lab, pred, id_gt, id_pred, vals = [], [], [], [], [], [], []
    for n, ei, gt, lg in cases:
        p, idg, idp, v = run_reference(utils, n, ei, gt, lg)
        node_ptr.append(node_ptr[-1] + n)
        edge_ptr.append(edge_ptr[-1] + ei.shape[1])
        src.append(ei[0])
        dst.append(ei[1])
        lab.append(gt)
        pred.append(p)
        id_gt.append(idg)
        id_pred.append(idp)
        vals.append(v)
    return dict(node_ptr=np.array(node_ptr, np.int32), edge_ptr=np.array(edge_ptr, np.int32), src=np.concatenate(src).astype(np.int16),
                dst=np.concatenate(dst).astype(np.int16), edge_labels=np.concatenate(lab).astype(np.uint8),
                predictions=np.concatenate(pred).astype(np.uint8), id_gt=np.concatenate(id_gt).astype(np.int16),
                id_pred=np.concatenate(id_pred).astype(np.int16), metrics=np.stack(vals))


def star_edges(ident, rng, n_neg):
    """Symmetric edges from every identity's first member to the others (label 1) plus n_neg random cross-identity pairs (label 0),
    both directions each."""
    src, dst, lab = [], [], []
    for c in np.unique(ident):
        m = np.flatnonzero(ident == c)
        for v in m[1:]:
            src += [m[0], v]
            dst += [v, m[0]]
            lab += [1, 1]
    n = len(ident)
    if n >= 2:
        for _ in range(n_neg):
            a, b = rng.integers(0, n, size=2)
            if ident[a] != ident[b]:
                src += [a, b]
                dst += [b, a]
                lab += [0, 0]
    return np.array(src, np.int64), np.array(dst, np.int64), np.array(lab, np.int64)


def noisy(rng, n, k, flip):
    ident = rng.integers(0, k, size=n)
    pred = ident.copy()
    moved = rng.random(n) < flip
    pred[moved] = rng.integers(0, k + k // 2 + 1, size=int(moved.sum())) + k
    return ident, pred


def partitions_fixture(prf):
    rng = np.random.default_rng(77)
    cases = [("empty", np.zeros(0, np.int64), np.zeros(0, np.int64), 0),
             ("one_node", np.array([0]), np.array([0]), 0),
             ("two_nodes_apart", np.array([0, 1]), np.array([0, 0]), 2),
             ("two_nodes_together", np.array([0, 0]), np.array([0, 1]), 0),
             ("no_edges", np.arange(6), np.array([0, 0, 1, 1, 2, 2]), 0),
             ("gt_one_cluster", np.zeros(40, np.int64), rng.integers(0, 5, size=40), 30),
             ("pred_singletons", rng.integers(0, 9, size=50), np.arange(50), 40),
             ("identical", np.repeat(np.arange(12), 5), np.repeat(np.arange(12), 5), 60)]
    for n, k, flip in ((34, 8, 0.2), (128, 30, 0.15), (1024, 200, 0.1), (4096, 700, 0.1), (4096, 40, 0.3)):
        t, p = noisy(rng, n, k, flip)
        cases.append((f"noisy_{n}_{k}", t, p, n))
    node_ptr, edge_ptr = [0], [0]
    src, dst, lab, pred, ids, preds, vals, names = [], [], [], [], [], [], [], []
    for name, ident, part, n_neg in cases:
        s, d, l = star_edges(ident, rng, n_neg)
        e_pred = (rng.random(len(l)) < np.where(l == 1, 0.8, 0.1)).astype(np.int64)
        G = nx.DiGraph([(int(a), int(b)) for a, b, x in zip(s, d, l) if x == 1])
        sets = list(nx.strongly_connected_components(G))
        id_gt = np.arange(len(ident))           # isolated nodes are singletons
        for q, c in enumerate(sets):
            for v in c:
                id_gt[v] = len(ident) + q
        TP, FP, TN, FN, P, R, F, p0, p1 = prf(e_pred, l.astype(np.float32))
        v = [P, R, F, TP, FP, FN, TN, metrics.adjusted_rand_score(id_gt, part), metrics.adjusted_mutual_info_score(id_gt, part),
             metrics.homogeneity_score(id_gt, part), metrics.completeness_score(id_gt, part), metrics.v_measure_score(id_gt, part),
             np.sum(np.asarray(p0)) / len(p0), np.sum(np.asarray(p1)) / len(p1)]
        node_ptr.append(node_ptr[-1] + len(ident))
        edge_ptr.append(edge_ptr[-1] + len(l))
        src.append(s)
        dst.append(d)
        lab.append(l)
        pred.append(e_pred)
        ids.append(id_gt)
        preds.append(part)
        vals.append(np.array([float(x) for x in v], dtype=np.float64))
        names.append(name)
    return dict(names=np.array(names), node_ptr=np.array(node_ptr, np.int32), edge_ptr=np.array(edge_ptr, np.int32),
                src=np.concatenate(src).astype(np.int16), dst=np.concatenate(dst).astype(np.int16),
                edge_labels=np.concatenate(lab).astype(np.uint8), predictions=np.concatenate(pred).astype(np.uint8),
                id_gt=np.concatenate(ids).astype(np.int16), id_pred=np.concatenate(preds).astype(np.int16), metrics=np.stack(vals))


def main():
    _install_torch_scatter_standin()
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, "/root/reference")
    from libs import utils  # the reference, unmodified

    ns = {"np": np}
    exec(compile(_lines(*PRF_LINES), "<reference inference.py:23-68>", "exec"), ns)
    fr = frames_fixture(utils)
    np.savez_compressed(os.path.join(HERE, "post2_eval_frames.npz"), **fr)
    pa = partitions_fixture(ns["compute_P_R_F"])
    np.savez_compressed(os.path.join(HERE, "post2_eval_partitions.npz"), **pa)
    print(f"frames: {len(fr['node_ptr']) - 1} frames, {fr['node_ptr'][-1]} nodes, {fr['edge_ptr'][-1]} edges")
    print(f"partitions: {', '.join(pa['names'])}")


if __name__ == "__main__":
    main()
