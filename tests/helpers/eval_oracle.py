"""numpy float64 restatement of the per-frame scoring of the reference's evaluation loop (inference.py:349-371) and of main.py:335-348's
aggregation -- the checker of gnn_cca_amd.evaluation.  No scikit-learn and no reference import (the GPU host has neither): the formulas and
special cases are restated from scikit-learn 1.7.2 (metrics/cluster/_supervised.py, _expected_mutual_info_fast.pyx) and pinned against it
by tests/test_eval_oracle.py (the goldens of tests/golden/make_golden_eval.py and, where it is installed, live scikit-learn).

    row = eval_frame(src, dst, edge_labels, predictions, pred_partition, n)    # 16 floats, columns gnn_cca_amd.evaluation.METRICS
    rows = eval_batch(edge_index, edge_labels, predictions, labels, node_ptr, edge_ptr)
"""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])
COLUMNS = ("P", "R", "F", "TP", "FP", "FN", "TN", "rand_index", "mutual_index", "homogeneity", "completeness", "v_measure",
           "precision0", "precision1", "n_clusters_gt", "n_clusters_pred")
EXACT = ("P", "R", "F", "TP", "FP", "FN", "TN", "rand_index", "precision0", "precision1", "n_clusters_gt", "n_clusters_pred")


def p_r_f(pred, lab):
    """compute_P_R_F (inference.py:23-68): TP, FP, TN, FN, P, R, F, precision0, precision1 as float64."""
    pred, lab = np.asarray(pred), np.asarray(lab)
    one, zero = lab == 1, lab == 0
    tp, fn = int(np.sum(pred[one] == 1)), int(np.sum(pred[one] == 0))
    fp, tn = int(np.sum(pred[zero] == 1)), int(np.sum(pred[zero] == 0))
    c1, c0 = int(one.sum()), int(zero.sum())
    P = np.float64(tp) / np.float64(tp + fp) if tp + fp else 0.0
    R = np.float64(tp) / np.float64(tp + fn) if tp + fn else 0.0
    F = 2 * (P * R) / (P + R) if P + R != 0 else 0.0
    prec1 = (np.float64(tp) / np.float64(c1)) * 100.0 if tp else 0.0
    prec0 = (np.float64(tn) / np.float64(c0)) * 100.0 if tn else 0.0
    return tp, fp, tn, fn, float(P), float(R), float(F), float(prec0), float(prec1)


def components(n, src, dst, active):
    """Connected components of the active edges (both endpoints in [0, n)): labels[v] = smallest node id of v's component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, on in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(active).tolist()):
        if on and 0 <= a < n and 0 <= b < n:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(n)], dtype=np.int64)


def _contingency(t, p):
    _, ti = np.unique(t, return_inverse=True)
    _, pi = np.unique(p, return_inverse=True)
    cells = {}
    for a, b in zip(ti.tolist(), pi.tolist()):
        cells[(a, b)] = cells.get((a, b), 0) + 1
    a_sizes = np.bincount(ti).astype(np.int64)
    b_sizes = np.bincount(pi).astype(np.int64)
    keys = sorted(cells)
    return a_sizes, b_sizes, np.array([k[0] for k in keys], dtype=np.int64), np.array([k[1] for k in keys], dtype=np.int64), \
        np.array([cells[k] for k in keys], dtype=np.int64)


def adjusted_rand(t, p):
    n = len(t)
    a, b, _, _, nij = _contingency(t, p) if n else (np.zeros(0, np.int64),) * 5
    ssq = int((nij * nij).sum())
    c11, c01, c10 = ssq - n, int((b * b).sum()) - ssq, int((a * a).sum()) - ssq
    c00 = n * n - c01 - c10 - ssq
    tn, fp, fn, tp = c00, c01, c10, c11
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def entropy(sizes):
    if sizes.sum() == 0:
        return 1.0
    if sizes.size == 1:
        return 0.0
    pi = sizes.astype(np.float64)
    s = pi.sum()
    return float(-np.sum((pi / s) * (np.log(pi) - math.log(s))))


def mutual_info(a, b, nij_rows, nij_cols, nij):
    if a.size == 1 or b.size == 1:
        return 0.0
    n = int(a.sum())
    cnm = nij / n
    outer = a[nij_rows] * b[nij_cols]
    log_outer = -np.log(outer) + math.log(n) + math.log(n)
    mi = cnm * (np.log(nij) - math.log(n)) + cnm * log_outer
    mi = np.where(np.abs(mi) < EPS, 0.0, mi)
    return float(np.clip(mi.sum(), 0.0, None))


def expected_mutual_info(a, b, n):
    """sklearn's EMI, its (i, j) double sum grouped by DISTINCT sizes (the term of a pair depends on the two sizes alone)."""
    if a.size == 1 or b.size == 1:
        return 0.0
    sa, ma = np.unique(a, return_counts=True)
    sb, mb = np.unique(b, return_counts=True)
    emi = 0.0
    gammaln = _lgamma
    lgn1 = math.lgamma(n + 1)
    for ai, wa in zip(sa.tolist(), ma.tolist()):
        for bj, wb in zip(sb.tolist(), mb.tolist()):
            nij = np.arange(max(1, ai - n + bj), min(ai, bj) + 1, dtype=np.float64)
            if nij.size == 0:
                continue
            term1 = nij / n
            term2 = (math.log(n) + np.log(nij)) - math.log(ai) - math.log(bj)
            gln = (gammaln(ai + 1) + gammaln(bj + 1) + gammaln(n - ai + 1) + gammaln(n - bj + 1) - (gammaln(nij + 1) + lgn1)
                   - gammaln(ai - nij + 1) - gammaln(bj - nij + 1) - gammaln(n - ai - bj + nij + 1))
            emi += wa * wb * float(np.sum(term1 * term2 * np.exp(gln)))
    return emi


def cluster_scores(t, p):
    """(ARI, AMI, homogeneity, completeness, V) of scikit-learn 1.7.2 for two labellings of the same nodes."""
    t, p = np.asarray(t), np.asarray(p)
    n = len(t)
    ari = adjusted_rand(t, p)
    if n == 0:
        return ari, 1.0, 1.0, 1.0, 1.0
    a, b, rows, cols, nij = _contingency(t, p)
    hc, hk = entropy(a), entropy(b)
    mi = mutual_info(a, b, rows, cols, nij)
    h = mi / hc if hc else 1.0
    c = mi / hk if hk else 1.0
    v = 0.0 if h + c == 0.0 else 2.0 * h * c / (h + c)
    if a.size == b.size == 1:
        ami = 1.0
    elif a.size == 1 or b.size == 1:
        ami = 0.0
    else:
        emi = expected_mutual_info(a, b, n)
        den = (hc + hk) / 2.0 - emi
        den = min(den, -EPS) if den < 0 else max(den, EPS)
        num = mi - emi
        num = min(num, -EPS) if num < 0 else max(num, EPS)
        ami = num / den
    return ari, ami, h, c, v


def eval_frame(src, dst, edge_labels, predictions, pred_partition, n, n_clusters_pred=None):
    """One frame: src / dst local ids, edge_labels 0/1, predictions 0/1, pred_partition [n] any labelling.  n_clusters_pred defaults to
    the number of distinct labels.  Returns (row of 16 floats, GT labels in the smallest-id convention)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    inside = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    lab, pred = np.asarray(edge_labels)[inside], np.asarray(predictions)[inside]
    tp, fp, tn, fn, P, R, F, prec0, prec1 = p_r_f(pred, lab)
    gt = components(n, src[inside], dst[inside], lab == 1)
    pp = np.asarray(pred_partition)
    ari, ami, h, c, v = cluster_scores(gt, pp)
    k_pred = len(np.unique(pp)) if n_clusters_pred is None else n_clusters_pred
    row = [P, R, F, tp, fp, fn, tn, ari, ami, h, c, v, prec0, prec1, len(np.unique(gt)), k_pred]
    return np.array(row, dtype=np.float64), gt


def eval_batch(edge_index, edge_labels, predictions, labels, node_ptr, edge_ptr):
    """Every frame of a batch (host arrays; labels in the smallest batch-global id convention) -> (rows [G, 16], GT labels [N] global)."""
    edge_index, labels = np.asarray(edge_index), np.asarray(labels)
    rows, gts = [], []
    for g in range(len(node_ptr) - 1):
        v0, v1, k0, k1 = int(node_ptr[g]), int(node_ptr[g + 1]), int(edge_ptr[g]), int(edge_ptr[g + 1])
        lab = labels[v0:v1]
        row, gt = eval_frame(edge_index[0, k0:k1] - v0, edge_index[1, k0:k1] - v0, edge_labels[k0:k1], predictions[k0:k1], lab, v1 - v0,
                             n_clusters_pred=int(np.sum(lab == np.arange(v0, v1))))
        rows.append(row)
        gts.append(gt + v0)
    return np.array(rows, dtype=np.float64).reshape(-1, 16), (np.concatenate(gts) if gts else np.zeros(0, np.int64))


def aggregate(rows):
    """main.py:335-348 over per-frame rows: means of P, R, F, RI, MI, hom, com, v, prec0, prec1; sums of TP, FP, FN, TN."""
    rows = np.asarray(rows, dtype=np.float64)
    mean = {"P": 0, "R": 1, "F": 2, "RI": 7, "MI": 8, "hom": 9, "com": 10, "v": 11, "prec0": 12, "prec1": 13}
    out = {k: float(np.mean(rows[:, c])) for k, c in mean.items()}
    out.update({k: int(np.sum(rows[:, c])) for k, c in {"TP": 3, "FP": 4, "FN": 5, "TN": 6}.items()})
    return out
