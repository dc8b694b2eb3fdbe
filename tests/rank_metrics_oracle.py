"""The ranking rules of include/gnncca_mpn.h (gnncca_rank_metrics, gnncca_rank_rows_accumulate, gnncca_rank_pool_add) restated in numpy:
what the device must equal bit for bit.  Every float64 operation below is one IEEE operation of numpy (no fused multiply-add), every
count a Python or numpy integer.

AP's order of additions, restated: the samples sorted by key descending; a group's term stands at the position of the group's LAST
sample, every other position holds +0; lane q of 256 adds the positions q, q + 256, ... ascending onto +0; within each block of 64 lanes
six butterfly steps v[q] = v[q] + v[q ^ o], o = 32, 16, 8, 4, 2, 1; AP = ((v[0] + v[64]) + v[128]) + v[192]."""
import numpy as np

COLUMNS = ("n_pos", "n_neg", "n_distinct", "n_nan", "AUROC", "AP", "best_F", "best_cut")
LANES = 256


def keys(scores, low):
    """fp32 scores (no NaN) -> uint32 keys, monotone: the score exactly negated when `low`, -0 taken as +0, then u | 0x80000000 for a
    non-negative score and ~u for a negative one."""
    s = np.asarray(scores, dtype=np.float32)
    if low:
        s = -s
    s = np.where(s == 0, np.float32(0.0), s).astype(np.float32)
    u = s.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ap_sum(terms):
    """The 256-lane sum of the per-position terms, in the header's order."""
    m = len(terms)
    padded = np.zeros((m + LANES - 1) // LANES * LANES if m else LANES, dtype=np.float64)
    padded[:m] = terms
    lanes = np.zeros(LANES, dtype=np.float64)
    for row in padded.reshape(-1, LANES):          # lane q: positions q, q + 256, ... ascending
        lanes = lanes + row
    v = lanes.reshape(LANES // 64, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ o]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def rank_row(scores, labels, low=False):
    """One frame, one score -> float64 [8], COLUMNS."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    labels = np.asarray(labels, dtype=np.float32).reshape(-1)
    sample = (labels == 1) | (labels == 0)
    s, pos = scores[sample], labels[sample] == 1
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    isnan = np.isnan(s)
    n_nan = int(isnan.sum())
    s, pos = s[~isnan], pos[~isnan]
    k = keys(s, low)
    order = np.argsort(-k.astype(np.int64), kind="stable")     # from the most positive key
    k, s, pos = k[order], s[order], pos[order]
    m = len(k)
    end = np.concatenate([k[1:] != k[:-1], [True]]) if m else np.zeros(0, dtype=bool)
    row = np.full(8, np.nan)
    row[:4] = n_pos, n_neg, int(end.sum()), n_nan
    if n_nan or n_pos == 0:
        return row
    at = np.nonzero(end)[0]
    TP = np.cumsum(pos.astype(np.int64))[at]
    FP = (at + 1) - TP
    p = TP - np.concatenate([[0], TP[:-1]])
    n = FP - np.concatenate([[0], FP[:-1]])
    if n_neg:
        num = sum(int(a) * (2 * (n_neg - int(b)) + int(c)) for a, b, c in zip(p, FP, n))      # an exact integer
        row[4] = num / (2 * n_pos * n_neg)                                                      # ... and one correctly rounded division
    terms = np.zeros(m, dtype=np.float64)
    has = p > 0
    terms[at[has]] = (p[has].astype(np.float64) / np.float64(n_pos)) * (TP[has].astype(np.float64) / (TP[has] + FP[has]).astype(np.float64))
    row[5] = ap_sum(terms)
    # compute_P_R_F at every cut (inference.py:53-66): TP + FP > 0 and TP + FN = n_pos > 0 at each
    P = TP.astype(np.float64) / (TP + FP).astype(np.float64)
    R = TP.astype(np.float64) / np.float64(n_pos)
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where((P + R) != 0, 2 * (P * R) / (P + R), 0.0)
    best = int(np.argmax(F))                                    # the first cut that reaches the maximum
    row[6] = F[best]
    row[7] = np.float64(s[at[best]]) + 0.0                      # the un-negated score, widened; a zero is +0
    return row


def rank_rows(score_list, labels, edge_ptr, low_list):
    """-> float64 [K, G, 8]."""
    g = len(edge_ptr) - 1
    out = np.empty((len(score_list), g, 8))
    for q, (sc, low) in enumerate(zip(score_list, low_list)):
        for f in range(g):
            a, b = edge_ptr[f], edge_ptr[f + 1]
            out[q, f] = rank_row(np.asarray(sc)[a:b], np.asarray(labels)[a:b], low)
    return out


def meter_fold(batches):
    """RankMeter's state after add(rows) for every rows float64 [K, G, 8] of `batches`: per score and column the frames one by one
    onto the running sum, a NaN skipped -> (sums float64 [K, 8], counts int64 [K, 8])."""
    k = batches[0].shape[0]
    sums, counts = np.zeros((k, 8)), np.zeros((k, 8), dtype=np.int64)
    for rows in batches:
        for f in range(rows.shape[1]):
            r = rows[:, f, :]
            ok = ~np.isnan(r)
            sums = np.where(ok, sums + np.where(ok, r, 0.0), sums)
            counts = counts + ok
    return sums, counts


def pooled_histograms(scores, labels, thresholds, keep):
    """-> (int64 [2, T + 1]: row 0 the negatives, row 1 the positives; the (negatives, positives) with a NaN score).  The bucket of a
    sample: keep='le' the number of thresholds < the widened score, keep='ge' the number <= it."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1).astype(np.float64)
    labels = np.asarray(labels, dtype=np.float32).reshape(-1)
    th = np.asarray(thresholds, dtype=np.float64)
    hist = np.zeros((2, len(th) + 1), dtype=np.int64)
    nans = []
    for cls in (0, 1):
        v = s[labels == cls]
        nans.append(int(np.isnan(v).sum()))
        v = v[~np.isnan(v)]
        b = np.searchsorted(th, v, side="left" if keep == "le" else "right")
        hist[cls] = np.bincount(b, minlength=len(th) + 1)
    return hist, tuple(nans)


def pooled_rows(hist, keep):
    """Per threshold TP, FP, FN, TN and compute_P_R_F's P, R, F on them; AUROC and AP of the quantised score: the non-empty buckets
    are the tie groups, from the most positive one (keep='le': bucket 0 upwards; 'ge': bucket T downwards), AP's terms added one by
    one in that order."""
    neg, pos = hist[0], hist[1]
    t = len(pos) - 1
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    out = {k: [] for k in ("TP", "FP", "FN", "TN", "P", "R", "F")}
    cpos, cneg = np.cumsum(pos), np.cumsum(neg)
    for i in range(t):
        # the buckets predicted 1 at thresholds[i]: keep='le' the buckets 0 ... i, keep='ge' the buckets i + 1 ... T
        TP, FP = (cpos[i], cneg[i]) if keep == "le" else (cpos[t] - cpos[i], cneg[t] - cneg[i])
        FN, TN = n_pos - TP, n_neg - FP
        P = TP / (TP + FP) if (TP + FP) != 0 else 0
        R = TP / (TP + FN) if (TP + FN) != 0 else 0
        F = 2 * (P * R) / (P + R) if (P + R) != 0 else 0
        for k, v in zip(("TP", "FP", "FN", "TN", "P", "R", "F"), (TP, FP, FN, TN, P, R, F)):
            out[k].append(v)
    res = {k: np.array(out[k], dtype=np.int64) for k in ("TP", "FP", "FN", "TN")}
    res.update({k: np.array(out[k], dtype=np.float64) for k in ("P", "R", "F")})
    buckets = [b for b in (range(t + 1) if keep == "le" else range(t, -1, -1)) if pos[b] + neg[b] > 0]
    num, tp, fp, ap = 0, 0, 0, np.float64(0.0)
    for b in buckets:
        p, n = int(pos[b]), int(neg[b])
        tp, fp = tp + p, fp + n
        num += p * (2 * (n_neg - fp) + n)
        if p:
            ap = ap + (np.float64(p) / np.float64(n_pos)) * (np.float64(tp) / np.float64(tp + fp))
    res["AUROC"] = num / (2 * n_pos * n_neg) if n_pos and n_neg else float("nan")
    res["AP"] = float(ap) if n_pos else float("nan")
    res["n_pos"], res["n_neg"] = n_pos, n_neg
    return res
