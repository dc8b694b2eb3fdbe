#!/usr/bin/env python3
"""Golden vectors for the joint sweep (gnn_cca_amd.calibration.sweep_joint, gnn_cca_amd.baselines): the reference's position baselines,
geometrical_association and geometrical_appearance_association of inference.py.

Their rule and scoring are inline code of two functions in a module that cannot be imported here.  As make_golden_sweep.py and
make_golden_post2.py do, this script READS the lines from /root/reference at run time, dedents them and executes them unmodified:
  inference.py:896       predictions = logical_and(edge_attr[0] < GEOM_TH / max_dist[0], edge_attr[1] < th)
  inference.py:721-724   predictions = spatial_dist_g < GEOM_TH / max_dist[0]        (the one-condition mode: the rule of :722-724 with
                         the `if CONFIG['NORM_TO_M']:` of :721 that makes it a statement; NORM_TO_M is true here)
  inference.py:899-908   the digraphs of the GT-active and the predicted-active edges, compute_SCC_and_Clusters on both
  inference.py:935-939   adjusted_rand_score ... v_measure_score of (ID_GT, ID_pred)
  libs/utils.py:295-317  compute_SCC_and_Clusters
with networkx and scikit-learn as installed (3.4.2 and 1.7.2 when the fixture was made).  Nothing of the reference's text is stored in
this repository: only numbers (calibration/geom_appearance.npz -- a subdirectory, because tests/conftest.py takes every .npz directly
under tests/golden/ for a forward case).

The case is one frame of four cameras x five detections with every cross-camera ordered pair (300 edges).  Conditions on the case,
asserted below: both scores carry ONE value per unordered pair, so the strongly connected components of the active digraph (the
reference) and the components of the mutual pairs (this repository) coincide; and at both thresholds comparing the float32 scores in
float32 and in float64 gives the same predictions (torch compares a float32 tensor with a Python scalar in float32; the sweep compares
in float64).  Build container only:

    python tests/golden/make_golden_geom.py
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
from make_golden import cross_camera_edges  # noqa: E402

REF_INFERENCE = "/root/reference/inference.py"
REF_UTILS = "/root/reference/libs/utils.py"
JOINT_RULE, GEOM_RULE, CLUSTERING, SCORING, SCC = (896, 896), (721, 724), (899, 908), (935, 939), (295, 317)


def reference_statements(path, span):
    with open(path) as f:
        lines = f.readlines()[span[0] - 1:span[1]]
    return textwrap.dedent("".join(lines))


def run(rule, ns):
    """One of the two rules, then the clustering and the scoring statements -> (predictions, ID_GT, ID_pred, the five scores)."""
    ns = dict(ns, rand_index=[], mutual_index=[], homogeneity=[], completeness=[], v_measure=[])
    for span in (rule, CLUSTERING, SCORING):
        exec(compile(reference_statements(REF_INFERENCE, span), f"<reference inference.py:{span[0]}-{span[1]}>", "exec"), ns)
    pred = ns["predictions"].numpy().astype(np.int64).reshape(-1)
    scores = [ns[k][0] for k in ("rand_index", "mutual_index", "homogeneity", "completeness", "v_measure")]
    return pred, np.asarray(ns["ID_GT"], dtype=np.int64), np.asarray(ns["ID_pred"], dtype=np.int64), np.array(scores, dtype=np.float64)


def main():
    scc = {"nx": nx, "np": np}
    exec(compile(reference_statements(REF_UTILS, SCC), "<reference libs/utils.py:295-317>", "exec"), scc)
    utils = types.SimpleNamespace(compute_SCC_and_Clusters=scc["compute_SCC_and_Clusters"])

    rng = np.random.default_rng(41)
    n, ei = cross_camera_edges([5, 5, 5, 5])
    ident = rng.integers(0, 6, size=n)
    centre = rng.uniform(-8.0, 8.0, size=(6, 2))
    pos = centre[ident] + rng.normal(0.0, 0.9, size=(n, 2))       # a person's detections lie within a metre or two of each other
    max_dist, geom_th, reid_th = 25.0, 2.4, 0.45
    same = ident[ei[0]] == ident[ei[1]]
    metres = np.sqrt(((pos[ei[0]] - pos[ei[1]]) ** 2).sum(axis=1))   # (a - b)^2 == (b - a)^2: one value per unordered pair
    geom = (metres / max_dist).astype(np.float32)
    pair, reid = {}, np.zeros(ei.shape[1], dtype=np.float32)
    for k, (a, b) in enumerate(ei.T.tolist()):
        key = (min(a, b), max(a, b))
        if key not in pair:   # same-identity pairs are closer in appearance, with overlap
            pair[key] = np.float32(rng.uniform(0.1, 0.55) if same[k] else rng.uniform(0.3, 1.0))
        reid[k] = pair[key]
    labels = same.astype(np.float32)

    # the conditions on the case
    where = {(int(a), int(b)): k for k, (a, b) in enumerate(ei.T)}
    back = np.array([where[(int(b), int(a))] for a, b in ei.T])
    assert np.array_equal(geom[back], geom) and np.array_equal(reid[back], reid) and np.array_equal(labels[back], labels)
    th_geom = geom_th / max_dist
    assert np.array_equal(geom < np.float32(th_geom), geom.astype(np.float64) < th_geom)
    assert np.array_equal(reid < np.float32(reid_th), reid.astype(np.float64) < reid_th)

    batch = types.SimpleNamespace(edge_index=torch.from_numpy(ei), num_nodes=n)
    ns = {"np": np, "torch": torch, "nx": nx, "utils": utils, "metrics": metrics, "data_batch": batch,
          "labels_edges_GT": torch.from_numpy(labels), "max_dist": [max_dist], "th": reid_th,
          "CONFIG": {"GEOM_TH": {"case": geom_th}, "DATASET_VAL": {"NAME": "case"}, "NORM_TO_M": True},
          "edge_attr": torch.from_numpy(np.stack([geom, reid])), "spatial_dist_g": torch.from_numpy(geom).view(-1, 1)}
    pred_j, gt_j, id_j, sc_j = run(JOINT_RULE, ns)
    pred_g, gt_g, id_g, sc_g = run(GEOM_RULE, ns)
    assert np.array_equal(gt_j, gt_g)
    assert np.array_equal(pred_j, ((geom.astype(np.float64) < th_geom) & (reid.astype(np.float64) < reid_th)).astype(np.int64))
    assert np.array_equal(pred_g, (geom.astype(np.float64) < th_geom).astype(np.int64))
    assert 0 < pred_j.sum() < pred_g.sum() < ei.shape[1] and len(set(id_j.tolist())) > len(set(id_g.tolist())) > 1

    out = dict(n_nodes=np.int64(n), edge_index=ei, geom=geom, reid=reid, edge_labels=labels, geom_th=np.float64(geom_th),
               max_dist=np.float64(max_dist), reid_th=np.float64(reid_th), id_gt=gt_j, pred_joint=pred_j, id_pred_joint=id_j,
               scores_joint=sc_j, pred_geom=pred_g, id_pred_geom=id_g, scores_geom=sc_g)
    os.makedirs(os.path.join(HERE, "calibration"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "calibration", "geom_appearance.npz"), **out)
    print(f"N={n} E={ei.shape[1]} label-1 edges {int(labels.sum())}; active: geometry {int(pred_g.sum())}, joint {int(pred_j.sum())}; "
          f"clusters: GT {len(set(gt_j.tolist()))}, geometry {len(set(id_g.tolist()))}, joint {len(set(id_j.tolist()))}; "
          f"ARI geometry {sc_g[0]:.4f} joint {sc_j[0]:.4f}")


if __name__ == "__main__":
    main()
