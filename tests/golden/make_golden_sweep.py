#!/usr/bin/env python3
"""Golden vectors for the threshold sweep (gnn_cca_amd.calibration): the reference's ReID calibration, main.py:141-175 -- normalise the
distances by their maximum, 100 thresholds `np.arange(0.01, 1.01, 0.01)`, `preds = (dist <= t) * 1`, `compute_P_R_F` at each.

Those statements are inline code of main.py under `if CONFIG['MODE'] == 'REID':`, in a script that cannot be imported here.  As
make_golden_post2.py does for inference.py, this script READS those lines from /root/reference/main.py at run time, dedents them and
executes them unmodified -- `reid_dists_l2` / `labels` the synthetic case below, the result lists empty, and `compute_P_R_F` the
reference's own (inference.py:23-68, read and executed the same way: the module cannot be imported either).  Nothing of the reference's
text is stored in this repository: only numbers (calibration/reid_sweep.npz, a subdirectory: tests/conftest.py takes every .npz directly
under tests/golden/ without a known prefix for a forward case) -- the inputs, the thresholds and the TP / FP / FN / TN / P / R / F lists.

The case is one frame of four cameras x five detections with every cross-camera ordered pair (300 edges); a pair's two directions carry
the same distance, so pruning single-direction edges changes nothing and the sweep's per-threshold counts are the reference's.
Condition on the inputs, asserted below: comparing the float32 distances with a threshold in float32 and in float64 gives the same
predictions at every threshold (the reference's pinned numpy and a current one promote a float32 array against a float64 scalar
differently; the sweep compares in float64).  Build container only:

    python tests/golden/make_golden_sweep.py
"""
import os
import sys
import textwrap

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import cross_camera_edges  # noqa: E402

REF_MAIN, SWEEP_FIRST, SWEEP_LAST = "/root/reference/main.py", 141, 175
REF_INFERENCE, PRF_FIRST, PRF_LAST = "/root/reference/inference.py", 23, 68


def reference_statements(path, first, last):
    with open(path) as f:
        lines = f.readlines()[first - 1:last]
    return textwrap.dedent("".join(lines))


def main():
    ns = {"np": np}
    exec(compile(reference_statements(REF_INFERENCE, PRF_FIRST, PRF_LAST), "<reference inference.py:23-68>", "exec"), ns)

    rng = np.random.default_rng(23)
    n, ei = cross_camera_edges([5, 5, 5, 5])
    ident = rng.integers(0, 6, size=n)
    same = ident[ei[0]] == ident[ei[1]]
    pair = {}
    dist = np.zeros(ei.shape[1], dtype=np.float32)
    for k, (a, b) in enumerate(ei.T.tolist()):
        key = (min(a, b), max(a, b))
        if key not in pair:   # one distance per unordered pair; same-identity pairs are closer, with overlap
            pair[key] = np.float32(rng.uniform(2.0, 14.0) if same[k] else rng.uniform(6.0, 24.0))
        dist[k] = pair[key]
    labels = same.astype(np.float32)

    ns.update(reid_dists_l2=dist, labels=labels, precisions=[], precisions_1=[], precisions_0=[], P_list=[], R_list=[], TP_list=[],
              FP_list=[], FN_list=[], TN_list=[], F_list=[])
    exec(compile(reference_statements(REF_MAIN, SWEEP_FIRST, SWEEP_LAST), "<reference main.py:141-175>", "exec"), ns)

    scores, ths = ns["reid_distances_norm"], np.asarray(ns["ths"], dtype=np.float64)
    assert scores.dtype == np.float32 and len(ths) == 100
    for t in ths:   # the condition on the inputs
        assert np.array_equal(scores <= np.float32(t), scores.astype(np.float64) <= np.float64(t)), t
    out = dict(n_nodes=np.int64(n), edge_index=ei, dists=dist, scores=scores, edge_labels=labels, thresholds=ths,
               TP=np.asarray(ns["TP_list"], dtype=np.int64), FP=np.asarray(ns["FP_list"], dtype=np.int64),
               FN=np.asarray(ns["FN_list"], dtype=np.int64), TN=np.asarray(ns["TN_list"], dtype=np.int64),
               P=np.asarray(ns["P_list"], dtype=np.float64), R=np.asarray(ns["R_list"], dtype=np.float64),
               F=np.asarray(ns["F_list"], dtype=np.float64))
    assert np.all(out["TP"] + out["FP"] + out["FN"] + out["TN"] == ei.shape[1])
    os.makedirs(os.path.join(HERE, "calibration"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "calibration", "reid_sweep.npz"), **out)
    best = np.where(out["F"] == out["F"].max())[0]
    print(f"N={n} E={ei.shape[1]} label-1 edges {int(labels.sum())}; max F {out['F'].max():.4f} at thresholds {ths[best]}; "
          f"TP at 0.25 / 0.5 / 1.0: {out['TP'][24]} / {out['TP'][49]} / {out['TP'][99]}")


if __name__ == "__main__":
    main()
