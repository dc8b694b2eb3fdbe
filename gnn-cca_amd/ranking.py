"""Which score orders the edges better?  Threshold-free ranking scores per frame, and the reference's pooled sweep over a data set.

calibration.py judges a score AT a threshold.  To compare the GNN's probabilities with the ground distance, the ReID distance or a
re-ranked distance one wants the area under the ROC curve and the average precision; and the reference's own calibration (main.py:124-319,
MODE REID) does not score frames at all: it pools every raw edge distance of the data set (`validate_REID`, inference.py:70-141), applies
`preds = dist <= t` for 100 thresholds and runs `compute_P_R_F` on the pooled vector -- no pruning, no clustering.

    rows = rank_metrics(batch, [probs, batch.edge_attr[:, 2]], ['high', 'low'])   # float64 [K, G, 8] on the device, RANK_COLUMNS
    rows = r.rank_metrics()                                                       # r: a pipeline.FrameResult, its probabilities
    meter = RankMeter(); meter.add(rows) ...                                      # one launch per call, no synchronisation
    res = meter.result()                                                          # one synchronisation: means over defined frames
    curve = PooledCurve(np.arange(0.01, 1.01, 0.01), keep='le')
    curve.add(batch, batch.edge_attr[:, 2]) ...                                   # one launch per call, nothing of the batch kept
    res = curve.result(); th = curve.thresholds[curve.best('F')]                  # one synchronisation; main.py:190

The rule (include/gnncca_mpn.h has it in full; tests/rank_metrics_oracle.py restates it in numpy, and the device equals that bit for
bit): samples are a frame's directed edges with a label of exactly 1 or 0; the ranking key is the float32 score (positive='low': exactly
negated) with -0 taken as +0; equal keys are ONE tie group; AUROC = sum over groups of p (2 neg_ranked_below + n) / (2 n_pos n_neg), an
exact integer over an exact integer; AP = sum over groups of (p / n_pos) (TP / (TP + FP)) in a fixed order of float64 additions;
best_F the maximum of compute_P_R_F's F over all cuts, best_cut the score of the first cut that reaches it.  A NaN score is counted in
n_nan and makes the frame's AUROC, AP, best_F and best_cut NaN; so does a frame without positives (AUROC: or without negatives).

* A capped batch (top_k=k) is ranked on its kept edges, like the sweeps.
* A frame holds at most 16384 edges here (it is sorted in the LDS of one compute unit); PooledCurve has no such limit.
* Nothing here says which score is better: no trained model exists in this repository."""
import numpy as np
import torch

from . import _native as nat
from .evaluation import _dev_i32
from .frames import _on, _raw_stream

RANK_COLUMNS = ("n_pos", "n_neg", "n_distinct", "n_nan", "AUROC", "AP", "best_F", "best_cut")
MAX_SCORES = nat.RANK_MAX_SCORES
MAX_RANK_FRAME_EDGES = nat.RANK_MAX_FRAME_EDGES
MAX_POOL_THRESHOLDS = nat.RANK_POOL_MAX_THRESHOLDS
POSITIVE = ("high", "low")
KEEP = ("le", "ge")
_NO_GPU = "gnn_cca_amd.ranking runs on MI355X only (no CPU fallback)"


def _scores(scores, e):
    """-> the K score tensors of a call, each [E] or [E, 1] (checked, not yet flattened)."""
    if torch.is_tensor(scores):
        scores = [scores]
    try:
        scores = list(scores)
    except TypeError:
        raise ValueError("scores must be a tensor [E] or a sequence of 1 to 4 of them") from None
    if not 1 <= len(scores) <= MAX_SCORES:
        raise ValueError(f"{len(scores)} scores; one call ranks 1 to {MAX_SCORES}")
    for k, s in enumerate(scores):
        if not torch.is_tensor(s) or not (s.dim() == 1 or (s.dim() == 2 and s.shape[1] == 1)) or s.numel() != e:
            shape = list(s.shape) if torch.is_tensor(s) else type(s).__name__
            raise ValueError(f"scores[{k}] ({shape}) does not match the batch: [E] or [E, 1] with E={e}")
    return scores


def _flat(s, e):
    """[E] float32 with a positive stride: a view where the caller's tensor allows one (edge_attr[:, k] is read in place)."""
    s = s.reshape(-1)
    if s.dtype != torch.float32:
        s = s.float()
    if e > 1 and s.stride(0) < 1:
        s = s.contiguous()
    return s


def rank_metrics(batch, scores, positive="high"):
    """Ranks every frame of `batch` (a GraphBatch as evaluate_frames takes it) by each of K scores: `scores` one device tensor [E] or
    [E, 1] or a sequence of 1 to 4 -- float32 views with a stride, such as batch.edge_attr[:, 2], are read in place; `positive` 'high'
    (a high score speaks for label 1: probabilities) or 'low' (distances), or a sequence with one per score.  One launch on the current
    stream, nothing waits for the GPU.  Returns float64 [K, G, 8] on the device, columns RANK_COLUMNS (the module's docstring has the
    rule).  Every argument is checked on the host (ValueError) before the GPU is touched; a frame of more than 16384 edges is refused
    there, by the host's batch.edge_ptr."""
    edge_ptr = np.asarray(batch.edge_ptr, dtype=np.int64)
    g = len(edge_ptr) - 1
    e = int(batch.edge_index.shape[1])
    sl = _scores(scores, e)
    k = len(sl)
    if isinstance(positive, str):
        positive = [positive] * k
    try:
        positive = list(positive)
    except TypeError:
        raise ValueError(f"positive must be 'high' or 'low', or a sequence of {k} of them, not {positive!r}") from None
    if len(positive) != k or any(not isinstance(p, str) or p not in POSITIVE for p in positive):
        raise ValueError(f"positive must be 'high' or 'low', or a sequence of {k} of them, not {positive!r}")
    if batch.edge_labels.numel() != e:
        raise ValueError(f"edge_labels [{batch.edge_labels.numel()}] do not match the batch (E={e})")
    max_e = int(np.diff(edge_ptr).max()) if g > 0 else 0
    if max_e > MAX_RANK_FRAME_EDGES:
        raise ValueError(f"a frame has {max_e} edges; rank_metrics ranks frames of at most {MAX_RANK_FRAME_EDGES} (PooledCurve has no limit)")
    if not all(s.is_cuda for s in sl) or not batch.edge_labels.is_cuda:
        raise RuntimeError(_NO_GPU)
    dev = sl[0].device
    if any(s.device != dev for s in sl):
        raise ValueError("the scores of one call must be on one device")
    with _on(dev):
        flat = [_flat(s, e) for s in sl]
        el = batch.edge_labels.reshape(-1)
        if el.dtype != torch.float32 or not el.is_contiguous():
            el = el.float().contiguous()
        rows = torch.empty((k, g, 8), dtype=torch.float64, device=dev)
        if g > 0:
            eptr = _dev_i32(batch.edge_ptr_dev, flat[0])
            ptrs = (nat.C.c_void_p * k)(*[s.data_ptr() if e else None for s in flat])
            strides = (nat.C.c_int64 * k)(*[max(int(s.stride(0)), 1) if e else 1 for s in flat])
            low = (nat.C.c_int32 * k)(*[int(p == "low") for p in positive])
            st = nat.lib().gnncca_rank_metrics(el.data_ptr() if e else None, ptrs, strides, low, k, e, eptr.data_ptr(), g, max_e, rows.data_ptr(),
                                               _raw_stream(dev))
            if st:
                nat.check(st, "gnncca_rank_metrics")
    return rows


class RankMeter:
    """The running means of many batches' rank_metrics rows (the same K scores in every call).  `add(rows)` makes one launch
    (gnncca_rank_rows_accumulate) and keeps nothing of the batch; no synchronisation before `result()`, which makes one.  Per score and
    column it keeps the sum over the frames where the column is defined (not NaN) and their number.  The order of the sums is part of
    the contract: the frames are added one by one onto the running value, in the order they were added (within a batch: ascending
    frame) -- ((s + r0) + r1) + ... in float64, a NaN skipped."""

    def __init__(self):
        self._state = None      # [K * 16] 8-byte words on the device: float64 sums [K, 8], then int64 counts [K, 8]
        self._k = None
        self._res = None

    def add(self, rows):
        if not torch.is_tensor(rows) or rows.dim() != 3 or rows.shape[2] != 8 or rows.dtype != torch.float64 or not 1 <= rows.shape[0] <= MAX_SCORES:
            raise ValueError("RankMeter.add expects the float64 [K, G, 8] rows of rank_metrics")
        k, g = int(rows.shape[0]), int(rows.shape[1])
        if self._k is not None and k != self._k:
            raise ValueError(f"RankMeter.add: rows of {k} scores after rows of {self._k}")
        if not rows.is_cuda:
            raise RuntimeError(_NO_GPU)
        with _on(rows.device):
            rows = rows.contiguous()
            if self._state is None:
                self._state, self._k = torch.zeros(k * 16, dtype=torch.float64, device=rows.device), k
            elif self._state.device != rows.device:
                raise ValueError("RankMeter.add: rows of another device than the earlier ones")
            st = nat.lib().gnncca_rank_rows_accumulate(rows.data_ptr() if g else None, k, g, self._state.data_ptr(),
                                                       self._state.data_ptr() + 8 * k * 8, _raw_stream(rows.device))
            if st:
                nat.check(st, "gnncca_rank_rows_accumulate")
        self._res = None
        return self

    def result(self):
        """-> dict(sums float64 [K, 8], frames int64 [K, 8] (the frames where each column is defined), means float64 [K, 8] (sum /
        frames, divided on the host; NaN where no frame defines the column), columns RANK_COLUMNS); the arrays are on the host."""
        if self._res is not None:
            return self._res
        if self._state is None:
            raise ValueError("RankMeter.result: no rows were added")
        host = self._state.cpu().numpy()    # the one synchronisation
        k = self._k
        sums, frames = host[:k * 8].reshape(k, 8).copy(), host[k * 8:].view(np.int64).reshape(k, 8).copy()
        means = np.full((k, 8), np.nan)
        np.divide(sums, frames.astype(np.float64), out=means, where=frames > 0)
        self._res = {"columns": RANK_COLUMNS, "sums": sums, "frames": frames, "means": means}
        return self._res


def _pool_thresholds(thresholds):
    try:
        th = np.array(thresholds, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"thresholds must be a sequence of real numbers ({exc})") from None
    if th.ndim != 1 or th.size < 1:
        raise ValueError("thresholds must be a non-empty one-dimensional sequence")
    if th.size > MAX_POOL_THRESHOLDS:
        raise ValueError(f"{th.size} thresholds; a pooled curve takes at most {MAX_POOL_THRESHOLDS}")
    if not np.isfinite(th).all():
        raise ValueError("thresholds must be finite")
    if not (np.diff(th) > 0).all():
        raise ValueError("thresholds must strictly increase")
    return th


def curve_from_histograms(hist, keep):
    """The rows of a pooled curve from its two histograms (int64 [2, T + 1]: row 0 the negatives, row 1 the positives; bucket b as
    gnncca_rank_pool_add defines it) -> dict(TP, FP, FN, TN int64 [T]; P, R, F float64 [T] by compute_P_R_F's expressions
    (inference.py:53-66) on numpy int64 counts; AUROC, AP of the score as the thresholds quantise it: the non-empty buckets are the tie
    groups, visited from the most positive one (keep='le': bucket 0 upwards, keep='ge': bucket T downwards), the AUROC numerator a
    Python integer, AP's terms added one by one in visiting order; n_pos, n_neg)."""
    hist = np.asarray(hist, dtype=np.int64)
    neg, pos = hist[0], hist[1]
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    if keep == "le":
        TP, FP = np.cumsum(pos)[:-1], np.cumsum(neg)[:-1]
    else:
        TP, FP = n_pos - np.cumsum(pos)[:-1], n_neg - np.cumsum(neg)[:-1]
    FN, TN = n_pos - TP, n_neg - FP
    p, r, f = [], [], []
    for tp, fp, fn in zip(TP, FP, FN):   # compute_P_R_F, expression for expression (numpy int64 counts)
        P = tp / (tp + fp) if (tp + fp) != 0 else 0
        R = tp / (tp + fn) if (tp + fn) != 0 else 0
        F = 2 * (P * R) / (P + R) if (P + R) != 0 else 0
        p.append(P), r.append(R), f.append(F)
    order = range(len(pos)) if keep == "le" else range(len(pos) - 1, -1, -1)
    num, tp, fp, ap = 0, 0, 0, np.float64(0.0)
    for b in order:
        gp, gn = int(pos[b]), int(neg[b])
        if gp + gn == 0:
            continue
        tp, fp = tp + gp, fp + gn
        num += gp * (2 * (n_neg - fp) + gn)
        if gp and n_pos:
            ap = ap + (np.float64(gp) / np.float64(n_pos)) * (np.float64(tp) / np.float64(tp + fp))
    auroc = num / (2 * n_pos * n_neg) if n_pos and n_neg else float("nan")
    return {"TP": TP.astype(np.int64), "FP": FP.astype(np.int64), "FN": FN.astype(np.int64), "TN": TN.astype(np.int64),
            "P": np.array(p, dtype=np.float64), "R": np.array(r, dtype=np.float64), "F": np.array(f, dtype=np.float64),
            "AUROC": float(auroc), "AP": float(ap) if n_pos else float("nan"), "n_pos": n_pos, "n_neg": n_neg}


class PooledCurve:
    """The reference's pooled sweep (main.py:124-319, MODE REID) accumulated over a data set: `thresholds` a host sequence of 1 to
    65536 finite reals that strictly increase; keep='le' predicts score <= t (distances, the reference's own), keep='ge' score >= t.
    `add(batch, scores)` / `add_raw(scores, labels)` enqueue one launch each (gnncca_rank_pool_add): a sample's bucket among the
    thresholds is found by binary search -- thresholds compared in float64 against the float32 score widened -- and two int64
    histograms are bumped with integer atomics, so any split of a data set into calls gives the same state.  The thresholds go up once,
    through pinned memory; nothing waits for the GPU and nothing of a batch is kept; a frame may have any size.  `result()`
    synchronises once."""

    def __init__(self, thresholds, keep="le"):
        if not isinstance(keep, str) or keep not in KEEP:
            raise ValueError(f"keep must be 'le' or 'ge', not {keep!r}")
        self.thresholds = _pool_thresholds(thresholds)
        self.keep = keep
        self.n_nan = None       # (negatives, positives) with a NaN score, known after result()
        self._state = None      # int64 [2 * (T + 1) + 2] on the device: the histograms, then the NaN counts
        self._th_dev = None
        self._res = None

    def add_raw(self, scores, labels):
        """`scores` [S] or [S, 1] (float32 views with a stride are read in place), `labels` [S] float32 with 1 / 0 (a sample with any
        other label is skipped, as gnncca_eval_frames skips it), both on the device."""
        if not torch.is_tensor(scores) or not torch.is_tensor(labels) or not (scores.dim() == 1 or (scores.dim() == 2 and scores.shape[1] == 1)):
            raise ValueError("PooledCurve.add_raw expects scores [S] or [S, 1] and labels [S]")
        s = int(scores.numel())
        if labels.numel() != s:
            raise ValueError(f"scores [{s}] and labels [{labels.numel()}] do not match")
        if not scores.is_cuda or not labels.is_cuda:
            raise RuntimeError(_NO_GPU)
        dev = scores.device
        t = int(self.thresholds.size)
        with _on(dev):
            if self._state is None:
                staged = torch.empty(t, dtype=torch.float64, pin_memory=True)
                staged.copy_(torch.from_numpy(self.thresholds))
                self._th_dev = staged.to(dev, non_blocking=True)
                self._state = torch.zeros(2 * (t + 1) + 2, dtype=torch.int64, device=dev)
            elif self._state.device != dev:
                raise ValueError("PooledCurve.add: scores of another device than the earlier ones")
            sc = _flat(scores, s)
            lab = labels.reshape(-1)
            if lab.dtype != torch.float32 or not lab.is_contiguous():
                lab = lab.float().contiguous()
            st = nat.lib().gnncca_rank_pool_add(sc.data_ptr() if s else None, max(int(sc.stride(0)), 1) if s else 1, lab.data_ptr() if s else None, s,
                                                self._th_dev.data_ptr(), t, int(self.keep == "le"), self._state.data_ptr(),
                                                self._state.data_ptr() + 16 * (t + 1), _raw_stream(dev))
            if st:
                nat.check(st, "gnncca_rank_pool_add")
        self._res = None
        return self

    def add(self, batch, scores):
        """Every edge of `batch` with its label (batch.edge_labels) and `scores` [E] or [E, 1]."""
        e = int(batch.edge_index.shape[1])
        if not torch.is_tensor(scores) or scores.numel() != e or batch.edge_labels.numel() != e:
            n = scores.numel() if torch.is_tensor(scores) else type(scores).__name__
            raise ValueError(f"scores [{n}] / edge_labels [{batch.edge_labels.numel()}] do not match the batch (E={e})")
        return self.add_raw(scores, batch.edge_labels)

    def histograms(self):
        """-> (int64 [2, T + 1], the (negatives, positives) with a NaN score) on the host; synchronises."""
        if self._state is None:
            raise ValueError("PooledCurve: nothing was added")
        host = self._state.cpu().numpy()
        t = int(self.thresholds.size)
        return host[:2 * (t + 1)].reshape(2, t + 1).copy(), (int(host[-2]), int(host[-1]))

    def result(self):
        """-> dict(thresholds float64 [T], and curve_from_histograms' entries: TP / FP / FN / TN int64 [T] (exact), P / R / F float64
        [T], AUROC, AP, n_pos, n_neg); the arrays are on the host.  Raises ValueError if a score was NaN (their number is in the
        message and in `n_nan`): the reference's comparisons would silently predict 0 for them."""
        if self._res is not None:
            return self._res
        hist, self.n_nan = self.histograms()    # the one synchronisation
        if self.n_nan[0] + self.n_nan[1]:
            raise ValueError(f"PooledCurve.result: {self.n_nan[1]} positive and {self.n_nan[0]} negative samples had a NaN score")
        out = {"thresholds": self.thresholds.copy()}
        out.update(curve_from_histograms(hist, self.keep))
        self._res = out
        return out

    def best(self, metric="F"):
        """Indices of ALL thresholds at which `metric` (P, R, F, TP, FP, FN or TN) equals its maximum -- main.py:190's
        np.where(F_list == np.max(F_list))."""
        res = self.result()
        if metric not in ("P", "R", "F", "TP", "FP", "FN", "TN"):
            raise ValueError(f"unknown metric {metric!r}")
        return np.where(res[metric] == np.max(res[metric]))[0]


__all__ = ["RANK_COLUMNS", "MAX_RANK_FRAME_EDGES", "MAX_POOL_THRESHOLDS", "rank_metrics", "RankMeter", "PooledCurve", "curve_from_histograms"]
