"""Numpy restatement of the symmetric capped graph build (build_graph_batch(top_k=k, rank_by=..., symmetric='union' | 'mutual')) and of
evaluate_frames(against='dense'), written from their definitions, not from the kernels.  TEST INFRASTRUCTURE.

Build: D = the directed capped selection of tests/helpers/graph_topk_oracle.py (keep_dir, a mask of the dense edge list); rev[e] = the
position of dense edge e's reverse (the dense graph holds every cross-camera pair in both directions); 'union' keeps keep_dir |
keep_dir[rev], 'mutual' keeps keep_dir & keep_dir[rev].  keep_dir[rev[e]] is the decision the DESTINATION of e made with its own keys
(the 'reid' key of (j, i) is F.pairwise_distance(reid[j], reid[i]), not the key of (i, j): the eps goes to a - b).

Scoring against the dense truth: scatter the capped predictions into the dense edge list (every dropped edge predicted 0) and score that
with tests/helpers/eval_oracle.py.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_oracle as eo  # noqa: E402
import graph_topk_oracle as gto  # noqa: E402

MODES = ["union", "mutual"]


def reverse_index(ei):
    """rev [E]: ei[:, rev[e]] == (ei[1, e], ei[0, e]).  Raises if an edge has no reverse (the dense list always has it)."""
    n = int(ei.max()) + 1 if ei.size else 1
    code = ei[0].astype(np.int64) * n + ei[1]
    order = np.argsort(code, kind="stable")
    back = ei[1].astype(np.int64) * n + ei[0]
    pos = np.searchsorted(code[order], back)
    assert np.all(pos < code.size) and np.array_equal(code[order][pos], back), "an edge without its reverse"
    return order[pos]


def close(ei, keep_dir, mode):
    rev = reverse_index(ei)
    if mode == "union":
        return keep_dir | keep_dir[rev]
    if mode == "mutual":
        return keep_dir & keep_dir[rev]
    raise ValueError(mode)


class Case:
    """The dense build and both keys of a fixture-shaped dict, computed once."""

    def __init__(self, a):
        self.a = a
        self.reid_n = gto.graph_oracle.normalize_columns(a["reid_embeds_raw"])
        self.ei, self.attr, self.lab = gto.dense(a, self.reid_n)
        self.key = {r: gto.keys(a, self.ei, r, self.reid_n) for r in ("ground", "reid")}
        self.node_ptr = np.concatenate([[0], np.cumsum(np.asarray(a["graph_sizes"], np.int64))])
        self._dir = {}

    def keep_dir(self, k, rank_by):
        if (k, rank_by) not in self._dir:
            self._dir[(k, rank_by)] = gto.select(self.ei, self.key[rank_by], k)
        return self._dir[(k, rank_by)]

    def keep(self, k, rank_by, mode):
        """bool [E_dense]: the kept edges; mode None: the directed selection."""
        d = self.keep_dir(k, rank_by)
        return d if mode is None else close(self.ei, d, mode)

    def build(self, k, rank_by, mode):
        keep = self.keep(k, rank_by, mode)
        return self.ei[:, keep], self.attr[keep], self.lab[keep], keep

    def edge_ptr(self, keep):
        """Per-frame edge ranges [G + 1] of a mask of the dense edge list (edges are emitted frame by frame)."""
        frame_of = np.searchsorted(self.node_ptr, self.ei[0], side="right") - 1
        counts = np.bincount(frame_of[keep], minlength=len(self.node_ptr) - 1)
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def random_outcome(case, keep, seed):
    """Predictions int64 [E_kept] (0/1) and a predicted partition int32 [N] in the smallest-global-id convention, from a fixed seed."""
    rng = np.random.default_rng(seed)
    pred = rng.integers(0, 2, int(keep.sum())).astype(np.int64)
    labels = np.empty(case.node_ptr[-1], np.int32)
    for v0, v1 in zip(case.node_ptr[:-1], case.node_ptr[1:]):
        part = rng.integers(0, max((v1 - v0) // 2, 1), v1 - v0)
        first = {}
        for v, c in enumerate(part.tolist()):
            first.setdefault(c, v)
        labels[v0:v1] = [first[c] + v0 for c in part.tolist()]
    return pred, labels


def scatter(keep, pred_kept):
    """The capped predictions in the dense edge list, every dropped edge predicted 0."""
    out = np.zeros(keep.size, np.int64)
    out[keep] = pred_kept
    return out


def score_against_dense(case, keep, pred_kept, labels):
    """rows [G, 16] and ID_GT [N] of the dense graph scored with the scattered predictions (eval_oracle.eval_batch)."""
    return eo.eval_batch(case.ei, case.lab, scatter(keep, pred_kept), labels, case.node_ptr, case.edge_ptr(np.ones(keep.size, bool)))


def score_kept(case, keep, pred_kept, labels):
    """The default scoring: the kept edges alone."""
    return eo.eval_batch(case.ei[:, keep], case.lab[keep], pred_kept, labels, case.node_ptr, case.edge_ptr(keep))


def dense_truth_by_definition(case, keep, pred_kept):
    """What evaluate_frames(against='dense') is defined to feed the formulas, from the person ids and cameras alone: per frame
    (TP, FP, FN, TN) and ID_GT [N] (smallest-global-id convention).  FN / TN of the kept edges plus the dropped ordered cross-camera pairs
    with the same / a different id; all detections of an identity seen on at least two cameras form one component."""
    a = case.a
    ids, cams = np.asarray(a["id"]), np.asarray(a["id_cam"])
    ei_k, lab_k = case.ei[:, keep], case.lab[keep]
    frame_of = np.searchsorted(case.node_ptr, ei_k[0], side="right") - 1
    counts, gt = [], np.arange(case.node_ptr[-1], dtype=np.int64)
    for g, (v0, v1) in enumerate(zip(case.node_ptr[:-1], case.node_ptr[1:])):
        here = frame_of == g
        lab, pred = lab_k[here], pred_kept[here]
        tp, fp = int(((lab == 1) & (pred == 1)).sum()), int(((lab == 0) & (pred == 1)).sum())
        fn, tn = int(((lab == 1) & (pred == 0)).sum()), int(((lab == 0) & (pred == 0)).sum())
        i, c = ids[v0:v1], cams[v0:v1]
        cross = c[:, None] != c[None, :]
        same = i[:, None] == i[None, :]
        fn += int((cross & same).sum()) - int((lab == 1).sum())
        tn += int((cross & ~same).sum()) - int((lab == 0).sum())
        counts.append((tp, fp, fn, tn))
        for v in range(v1 - v0):
            if (cross[v] & same[v]).any():
                gt[v0 + v] = v0 + int(np.flatnonzero(same[v])[0])
    return np.asarray(counts, np.int64), gt
