"""Which threshold should the association run at?  Every operating point of a batch scored in one pass on the GPU.

The reference calibrates its comparison methods by sweeping thresholds on the host (main.py:124-319, MODE REID: 100 thresholds over the
ReID L2 and cosine distances, `compute_P_R_F` at each, the threshold of maximal F; the OPT_TH / GEOM_TH tables of config_inference.yaml
are the results of such sweeps).  With `threshold` -> `prune_and_cluster` -> `evaluate_frames` that is a Python loop of five or more
launches and one int64 [E] prediction vector per threshold; `sweep_thresholds` is four launches whatever the number of thresholds
(csrc/eval_sweep.cuh) and returns, bit for bit, the rows that loop returns.

    rows = sweep_thresholds(batch, scores, thresholds)             # float64 [T, G, 16] on the device, columns evaluation.METRICS
    rows = r.sweep(thresholds)                                     # r: a pipeline.FrameResult, its probabilities, keep='ge'
    rows = r.sweep(thresholds, partition='exclusive')              # the operating points of r.exclusive(), not of the components
    acc = SweepAccumulator(thresholds); acc.add(rows) ...          # no synchronisation
    res = acc.result()                                             # one synchronisation
    th = acc.thresholds[acc.best('F_micro')]                       # every threshold of maximal F (main.py:190)
    pipe = FramePipeline(model, threshold=float(th[0]))            # ... applied

The rule for threshold t (include/gnncca_mpn.h has it in full): an edge is active iff its score >= thresholds[t] (keep='le': <=, for
distances); it is kept iff its reverse edge is active too; the partition is the connected components of the kept edges; the row is
evaluate_frames' for those predictions and that partition.  With partition='exclusive' the partition is the camera-exclusive one of
postprocess.exclusive_clusters at thresholds[t] and the predictions are its predictions (one pass as well: a pair's place in the rule's
order does not depend on the threshold).

* A threshold is compared in float64 against the float32 score widened to float64.  `scores <= t` in numpy or torch may round t to
  float32 first: only at a threshold that lies within a float32 rounding of a score can the two differ.
* Normalising a score is the caller's business: main.py:141 divides the distances by the maximum of the whole dataset before it sweeps
  0.01 ... 1.00.
* A capped batch (top_k=k) is swept against its kept edges only (`evaluate_frames(against='kept')`); there is no dense form.
* Nothing here says which threshold is right: no trained model exists in this repository, and a threshold chosen on random weights
  means nothing."""
import numpy as np
import torch

from . import _native as nat
from .evaluation import MAX_FRAME_NODES, METRICS, _aggregates, _dev_i32, _reduce_rows
from .frames import _on, _raw_stream
from .postprocess import check_cameras, check_threshold

MAX_THRESHOLDS = nat.SWEEP_MAX_THRESHOLDS
KEEP = ("ge", "le")
PARTITIONS = ("components", "exclusive")
MICRO = ("P_micro", "R_micro", "F_micro")


def _thresholds(thresholds):
    try:
        th = np.array(thresholds, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"thresholds must be a sequence of real numbers ({exc})") from None
    if th.ndim != 1 or th.size < 1:
        raise ValueError("thresholds must be a non-empty one-dimensional sequence")
    if th.size > MAX_THRESHOLDS:
        raise ValueError(f"{th.size} thresholds; one sweep takes at most {MAX_THRESHOLDS}")
    if not np.isfinite(th).all():
        raise ValueError("thresholds must be finite")
    return th


def sweep_thresholds(batch, scores, thresholds, keep="ge", return_labels=False, partition="components", cam=None):
    """Scores every frame of `batch` (a GraphBatch as evaluate_frames takes it) at every threshold: `scores` float32 [E] or [E, 1] on the
    device, any per-edge score; `thresholds` a host sequence of finite reals (at most 1024; any order, duplicates allowed); keep='ge'
    keeps score >= t (probabilities), keep='le' keeps score <= t (distances).  Enqueued on the current stream without a wait (the
    thresholds go up through pinned memory); returns float64 [T, G, 16] on the device, rows[t] bit for bit
    evaluate_frames(batch, post['pruned'], post['labels']) with post = prune_and_cluster(..., predictions at thresholds[t], ...), and with
    return_labels=True also int32 [T, N], the partitions (a node's label the smallest node id of its cluster).

    partition='exclusive' sweeps the CAMERA-EXCLUSIVE partition instead (csrc/eval_sweep_exclusive.cuh): rows[t] bit for bit
    evaluate_frames(batch, ex['predictions'], ex['labels']) with ex = postprocess.exclusive_clusters(..., at=thresholds[t]), the labels
    ex['labels'] -- the threshold of FrameResult.exclusive() is calibrated on this partition, not on the components.  `cam`: int32 [N]
    camera ids on the device (default: batch.cam_dev).  Its domain is exclusive_clusters': every threshold strictly inside (0, 1),
    keep='ge' only (the rule needs positive weights), camera ids in [0, 64) (judged on the host where batch.cam_host or a host `cam`
    exists; an id that reaches the device makes its frame "every node its own cluster"), frames of at most 4096 detections."""
    if keep not in KEEP:
        raise ValueError(f"keep must be 'ge' or 'le', not {keep!r}")
    if not isinstance(partition, str) or partition not in PARTITIONS:
        raise ValueError(f"partition must be 'components' or 'exclusive', not {partition!r}")
    exclusive = partition == "exclusive"
    if exclusive and keep != "ge":
        raise ValueError("partition='exclusive' takes keep='ge' only: the camera-exclusive rule orders pairs by a positive weight")
    th = _thresholds(thresholds)
    if exclusive:
        for v in th.tolist():
            check_threshold(v)
    node_ptr = np.asarray(batch.node_ptr, dtype=np.int64)
    g = len(node_ptr) - 1
    n = int(node_ptr[-1]) if g > 0 else 0
    e = int(batch.edge_index.shape[1])
    max_n = int(np.diff(node_ptr).max()) if g > 0 else 0
    if max_n > MAX_FRAME_NODES:
        raise ValueError(f"a frame has {max_n} detections; sweep_thresholds scores frames of at most {MAX_FRAME_NODES}")
    if scores.numel() != e or batch.edge_labels.numel() != e:
        raise ValueError(f"scores [{scores.numel()}] / edge_labels [{batch.edge_labels.numel()}] do not match the batch (E={e})")
    if exclusive:
        if cam is None:
            cam = getattr(batch, "cam_dev", None)
            if cam is None:
                raise ValueError("partition='exclusive' needs camera ids: pass cam (int32 [N] on the device) or a batch with cam_dev")
            if getattr(batch, "cam_host", None) is not None:
                check_cameras(batch.cam_host)
        if not torch.is_tensor(cam) or cam.numel() != n:
            raise ValueError(f"cam [{cam.numel() if torch.is_tensor(cam) else type(cam).__name__}] does not match the batch (N={n})")
        if not cam.is_cuda:   # a host tensor can be judged here; it is refused below like any other host input
            check_cameras(cam.numpy())
    if not scores.is_cuda or (exclusive and not cam.is_cuda):
        raise RuntimeError("gnn_cca_amd.calibration runs on MI355X only (no CPU fallback)")
    dev = scores.device
    t = int(th.size)
    lib = nat.lib()
    with _on(dev):
        sc = scores.reshape(-1)
        if sc.dtype != torch.float32 or not sc.is_contiguous():
            sc = sc.float().contiguous()
        ei = batch.edge_index.contiguous()
        el = batch.edge_labels.contiguous()
        rows = torch.empty((t, g, 16), dtype=torch.float64, device=dev)
        labels = torch.empty((t, n), dtype=torch.int32, device=dev) if return_labels else None
        if g > 0:
            nptr, eptr = _dev_i32(batch.node_ptr_dev, sc), _dev_i32(batch.edge_ptr_dev, sc)
            staged = torch.empty(t, dtype=torch.float64, pin_memory=True)
            staged.copy_(torch.from_numpy(th))
            th_dev = staged.to(dev, non_blocking=True)
            lab_ptr = labels.data_ptr() if return_labels and n else None
            if exclusive:
                cm = _dev_i32(cam.reshape(-1), sc)
                ws_bytes = lib.gnncca_eval_sweep_exclusive_workspace_bytes(n, e, g, t)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                st = lib.gnncca_eval_sweep_exclusive(ei.data_ptr() if e else None, el.data_ptr() if e else None, sc.data_ptr() if e else None,
                                                     cm.data_ptr() if n else None, n, e, nptr.data_ptr(), eptr.data_ptr(), g, max_n,
                                                     th_dev.data_ptr(), t, rows.data_ptr(), lab_ptr, ws.data_ptr(), ws_bytes, _raw_stream(dev))
                if st:
                    nat.check(st, "gnncca_eval_sweep_exclusive")
            else:
                ws_bytes = lib.gnncca_eval_sweep_workspace_bytes(n, e, g, t)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
                st = lib.gnncca_eval_sweep(ei.data_ptr() if e else None, el.data_ptr() if e else None, sc.data_ptr() if e else None, n, e,
                                           nptr.data_ptr(), eptr.data_ptr(), g, max_n, th_dev.data_ptr(), t, int(keep == "le"), rows.data_ptr(),
                                           lab_ptr, ws.data_ptr(), ws_bytes, _raw_stream(dev))
                if st:
                    nat.check(st, "gnncca_eval_sweep")
            # workspace and thresholds are freed by the caching allocator in stream order (allocated on this stream): nothing to keep
    return (rows, labels) if return_labels else rows


class SweepAccumulator:
    """Collects the device rows of many batches' sweeps over the SAME thresholds (`add`, no synchronisation) and reduces them once
    (`result`, one synchronisation).  Per threshold: main.py:335-348's aggregates, reduced by EvalAccumulator's own reduction (threshold t
    gets exactly what an EvalAccumulator fed rows[t] of the same batches in the same order returns); the summed TP / FP / FN / TN; and
    P_micro / R_micro / F_micro, `compute_P_R_F`'s expressions (inference.py:53-66) on the summed counts, which is how main.py:167 scores
    a threshold over the whole dataset."""

    def __init__(self, thresholds):
        self.thresholds = _thresholds(thresholds)
        self._rows = []
        self._res = None

    def add(self, rows):
        if rows.dim() != 3 or rows.shape[0] != self.thresholds.size or rows.shape[2] != len(METRICS) or rows.dtype != torch.float64:
            raise ValueError(f"SweepAccumulator.add expects the float64 [{self.thresholds.size}, G, 16] rows of sweep_thresholds")
        self._rows.append(rows)
        self._res = None
        return self

    def __len__(self):
        return sum(int(r.shape[1]) for r in self._rows)

    def result(self):
        """-> dict(thresholds float64 [T], aggregates: list of T dicts as EvalAccumulator.result() returns them, TP / FP / FN / TN int64
        [T], P_micro / R_micro / F_micro float64 [T]); the arrays are on the host."""
        if self._res is not None:
            return self._res
        if not self._rows:
            raise ValueError("SweepAccumulator.result: no rows were added")
        red = []
        for t in range(self.thresholds.size):   # EvalAccumulator's tensors, threshold by threshold: the same reduction, the same bits
            allr = torch.cat([r[t] for r in self._rows]) if len(self._rows) > 1 else self._rows[0][t]
            red.append(_reduce_rows(allr))
        host = torch.stack(red).cpu().numpy()    # the one synchronisation
        agg = [_aggregates(h) for h in host]
        out = {"thresholds": self.thresholds.copy(), "aggregates": agg}
        for name in ("TP", "FP", "FN", "TN"):
            out[name] = np.array([a[name] for a in agg], dtype=np.int64)
        p, r, f = [], [], []
        for TP, FP, FN in zip(out["TP"], out["FP"], out["FN"]):   # compute_P_R_F, expression for expression (numpy int64 counts)
            P = TP / (TP + FP) if (TP + FP) != 0 else 0
            R = TP / (TP + FN) if (TP + FN) != 0 else 0
            F = 2 * (P * R) / (P + R) if (P + R) != 0 else 0
            p.append(P), r.append(R), f.append(F)
        out["P_micro"], out["R_micro"], out["F_micro"] = (np.array(v, dtype=np.float64) for v in (p, r, f))
        self._res = out
        return out

    def best(self, metric="F_micro"):
        """Indices of ALL thresholds at which `metric` equals its maximum -- main.py:190's np.where(F_list == np.max(F_list)).  `metric`:
        P_micro / R_micro / F_micro, or one of the aggregates' names (P, R, F, TP, ..., prec1)."""
        res = self.result()
        if metric in MICRO:
            vals = res[metric]
        elif metric in res["aggregates"][0]:
            vals = np.array([a[metric] for a in res["aggregates"]], dtype=np.float64)
        else:
            raise ValueError(f"unknown metric {metric!r}")
        return np.where(vals == np.max(vals))[0]


__all__ = ["MAX_THRESHOLDS", "sweep_thresholds", "SweepAccumulator"]
