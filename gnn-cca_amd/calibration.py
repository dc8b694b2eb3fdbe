"""Which threshold should the association run at?  Every operating point of a batch scored in one pass on the GPU.

The reference calibrates its comparison methods by sweeping thresholds on the host (main.py:124-319, MODE REID: 100 thresholds over the
ReID L2 and cosine distances, `compute_P_R_F` at each, the threshold of maximal F; the OPT_TH / GEOM_TH tables of config_inference.yaml
are the results of such sweeps).  With `threshold` -> `prune_and_cluster` -> `evaluate_frames` that is a Python loop of five or more
launches and one int64 [E] prediction vector per threshold; `sweep_thresholds` is four launches whatever the number of thresholds
(csrc/eval_sweep.cuh) and returns, bit for bit, the rows that loop returns.

    rows = sweep_thresholds(batch, scores, thresholds)             # float64 [T, G, 16] on the device, columns evaluation.METRICS
    rows = r.sweep(thresholds)                                     # r: a pipeline.FrameResult, its probabilities, keep='ge'
    rows = r.sweep(thresholds, partition='exclusive')              # the operating points of r.exclusive(), not of the components
    rows = r.sweep(thresholds, partition='strong')                 # ... of a pipeline with pruning=False: strongly connected clusters
    acc = SweepAccumulator(thresholds); acc.add(rows) ...          # no synchronisation
    res = acc.result()                                             # one synchronisation
    th = acc.thresholds[acc.best('F_micro')]                       # every threshold of maximal F (main.py:190)
    pipe = FramePipeline(model, threshold=float(th[0]))            # ... applied

The rule for threshold t (include/gnncca_mpn.h has it in full): an edge is active iff its score >= thresholds[t] (keep='le': <=, for
distances); it is kept iff its reverse edge is active too; the partition is the connected components of the kept edges; the row is
evaluate_frames' for those predictions and that partition.  With partition='exclusive' the partition is the camera-exclusive one of
postprocess.exclusive_clusters at thresholds[t] and the predictions are its predictions (one pass as well: a pair's place in the rule's
order does not depend on the threshold).  With partition='strong' nothing is pruned and the partition is the strongly connected
components of the active edges (postprocess.strong_clusters at thresholds[t]; two launches, csrc/eval_sweep_strong.cuh).

Several scores at once (csrc/eval_sweep_joint.cuh): the reference's position baselines keep an edge iff its ground distance AND its ReID
distance pass (inference.py:722-724, :896), and their tables were swept one axis at a time.  partition='strong' in either call is the
reference's own clustering for them: no pruning, strongly connected components.

    rows = sweep_joint(batch, [attr[:, 0], attr[:, 2]], points, ['lt', 'lt'], frame_div=div)   # points host [T, 2]; float64 [T, G, 16]
    rows = sweep_grid(batch, [attr[:, 0], attr[:, 2]], [axis0, axis1], ['lt', 'lt'])           # ... viewed [T0, T1, G, 16]
    acc = JointSweepAccumulator(grid_points([axis0, axis1])[0]); acc.add(rows) ...             # one launch, nothing of the batch kept
    best = acc.points[acc.best('F_micro')]                                                     # one synchronisation

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
from .evaluation import AGGREGATES, MAX_FRAME_NODES, METRICS, _aggregates, _dev_i32, _reduce_rows
from .frames import _on, _raw_stream
from .postprocess import check_cameras, check_threshold, widest_frame

MAX_THRESHOLDS = nat.SWEEP_MAX_THRESHOLDS
KEEP = ("ge", "le")
PARTITIONS = ("components", "exclusive")            # the partitions built from mutual pairs (the pruning rule)
SWEEP_PARTITIONS = PARTITIONS + ("strong",)         # every partition sweep_thresholds takes: 'strong' prunes nothing
JOINT_PARTITIONS = ("components", "strong")   # the camera-exclusive partition is not swept jointly
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


def _batch_dims(batch):
    """-> (g, n, e, max_n): the frames, nodes and edges of a GraphBatch and the detections of its widest frame."""
    node_ptr = np.asarray(batch.node_ptr, dtype=np.int64)
    g = len(node_ptr) - 1
    return g, int(node_ptr[-1]) if g > 0 else 0, int(batch.edge_index.shape[1]), widest_frame(node_ptr)


def _stage(host, dev):
    """A flat host float64 array -> (the pinned staging tensor, its copy on the device), without a wait.  The caller holds the pinned
    tensor until its launches are enqueued: freeing it makes the host allocator record an event on the stream, and that marker belongs
    behind the sweep's kernels, not between the copy and the first of them."""
    staged = torch.empty(host.size, dtype=torch.float64, pin_memory=True)
    staged.copy_(torch.from_numpy(host))
    return staged, staged.to(dev, non_blocking=True)


def _outputs(t, g, n, return_labels, dev):
    """-> (rows float64 [T, G, 16], labels int32 [T, N] or None, the labels' pointer as the entries take it); nothing is initialised."""
    rows = torch.empty((t, g, 16), dtype=torch.float64, device=dev)
    labels = torch.empty((t, n), dtype=torch.int32, device=dev) if return_labels else None
    return rows, labels, labels.data_ptr() if return_labels and n else None


_ENTRIES = {}   # name -> (`name`_workspace_bytes, `name`) of the loaded library: looked up once, not per sweep


def _run(name, size_args, dev, *args):
    """Calls the sweep entry `name` on the current stream: `args`, then a workspace of `name`_workspace_bytes(*size_args) bytes (allocated
    on this stream, so freed in stream order: nothing to keep) and the stream; raises on a bad status."""
    fns = _ENTRIES.get(name)
    if fns is None:
        fns = _ENTRIES[name] = (getattr(nat.lib(), name + "_workspace_bytes"), getattr(nat.lib(), name))
    ws_bytes = fns[0](*size_args)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = fns[1](*args, ws.data_ptr(), ws_bytes, _raw_stream(dev))
    if st:
        nat.check(st, name)


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
    exists; an id that reaches the device makes its frame "every node its own cluster"), frames of at most 4096 detections.

    partition='strong' sweeps the STRONGLY CONNECTED clusters of the unpruned edges (csrc/eval_sweep_strong.cuh), the reference's rule
    with PRUNING off: rows[t] bit for bit evaluate_frames(batch, pred_t, strong_clusters(batch.edge_index, pred_t, ...)['labels']) with
    pred_t the active edges at thresholds[t], nothing pruned -- the threshold of a FramePipeline(pruning=False, splitting=False) is
    calibrated on this partition.  Both `keep` values and any finite thresholds are allowed; `cam` is ignored; frames of at most 1024
    detections (a frame's reachability matrix lives in LDS).  Two launches whatever the number of thresholds."""
    if keep not in KEEP:
        raise ValueError(f"keep must be 'ge' or 'le', not {keep!r}")
    if not isinstance(partition, str) or partition not in SWEEP_PARTITIONS:
        raise ValueError(f"partition must be one of {SWEEP_PARTITIONS}, not {partition!r}")
    if partition == "strong":   # the K = 1 case of the joint form (csrc/eval_sweep_strong.cuh): the same entry, the same host checks
        th = _thresholds(thresholds)
        if not torch.is_tensor(scores) or scores.numel() != int(batch.edge_index.shape[1]):
            size = scores.numel() if torch.is_tensor(scores) else type(scores).__name__
            raise ValueError(f"scores [{size}] do not match the batch (E={int(batch.edge_index.shape[1])})")
        return sweep_joint(batch, [scores.reshape(-1)], th.reshape(-1, 1), [keep], return_labels=return_labels, partition="strong")
    exclusive = partition == "exclusive"
    if exclusive and keep != "ge":
        raise ValueError("partition='exclusive' takes keep='ge' only: the camera-exclusive rule orders pairs by a positive weight")
    th = _thresholds(thresholds)
    if exclusive:
        for v in th.tolist():
            check_threshold(v)
    g, n, e, max_n = _batch_dims(batch)
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
    with _on(dev):
        sc = scores.reshape(-1)
        if sc.dtype != torch.float32 or not sc.is_contiguous():
            sc = sc.float().contiguous()
        ei = batch.edge_index.contiguous()
        el = batch.edge_labels.contiguous()
        rows, labels, lab_ptr = _outputs(t, g, n, return_labels, dev)
        if g > 0:
            nptr, eptr = _dev_i32(batch.node_ptr_dev, sc), _dev_i32(batch.edge_ptr_dev, sc)
            pinned, th_dev = _stage(th, dev)
            ei_ptr, el_ptr, sc_ptr = (ei.data_ptr(), el.data_ptr(), sc.data_ptr()) if e else (None, None, None)
            if exclusive:
                cm = _dev_i32(cam.reshape(-1), sc)
                _run("gnncca_eval_sweep_exclusive", (n, e, g, t), dev, ei_ptr, el_ptr, sc_ptr, cm.data_ptr() if n else None, n, e, nptr.data_ptr(),
                     eptr.data_ptr(), g, max_n, th_dev.data_ptr(), t, rows.data_ptr(), lab_ptr)
            else:
                _run("gnncca_eval_sweep", (n, e, g, t), dev, ei_ptr, el_ptr, sc_ptr, n, e, nptr.data_ptr(), eptr.data_ptr(), g, max_n,
                     th_dev.data_ptr(), t, int(keep == "le"), rows.data_ptr(), lab_ptr)
    return (rows, labels) if return_labels else rows


def _micro_prf(out):
    """Completes an accumulator's result `out` (it holds 'aggregates', one dict per operating point) with the summed TP / FP / FN / TN as
    int64 arrays and P_micro / R_micro / F_micro, `compute_P_R_F`'s expressions (inference.py:53-66) on those sums."""
    for name in ("TP", "FP", "FN", "TN"):
        out[name] = np.array([a[name] for a in out["aggregates"]], dtype=np.int64)
    p, r, f = [], [], []
    for TP, FP, FN in zip(out["TP"], out["FP"], out["FN"]):   # compute_P_R_F, expression for expression (numpy int64 counts)
        P = TP / (TP + FP) if (TP + FP) != 0 else 0
        R = TP / (TP + FN) if (TP + FN) != 0 else 0
        F = 2 * (P * R) / (P + R) if (P + R) != 0 else 0
        p.append(P), r.append(R), f.append(F)
    out["P_micro"], out["R_micro"], out["F_micro"] = (np.array(v, dtype=np.float64) for v in (p, r, f))
    return out


def _best(res, metric):
    """Indices of ALL operating points of an accumulator's result at which `metric` equals its maximum."""
    if metric in MICRO:
        vals = res[metric]
    elif metric in res["aggregates"][0]:
        vals = np.array([a[metric] for a in res["aggregates"]], dtype=np.float64)
    else:
        raise ValueError(f"unknown metric {metric!r}")
    return np.where(vals == np.max(vals))[0]


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
        self._res = _micro_prf({"thresholds": self.thresholds.copy(), "aggregates": agg})
        return self._res

    def best(self, metric="F_micro"):
        """Indices of ALL thresholds at which `metric` equals its maximum -- main.py:190's np.where(F_list == np.max(F_list)).  `metric`:
        P_micro / R_micro / F_micro, or one of the aggregates' names (P, R, F, TP, ..., prec1)."""
        return _best(self.result(), metric)


MAX_POINTS = nat.JOINT_MAX_POINTS
MAX_SCORES = nat.JOINT_MAX_SCORES
COMPARATORS = tuple(nat.CMP)


def _points(points, k):
    try:
        pts = np.array(points, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"points must be a [T, {k}] array of real numbers ({exc})") from None
    if pts.ndim != 2 or pts.shape[0] < 1 or pts.shape[1] != k:
        raise ValueError(f"points must be a non-empty [T, {k}] array (one column per score), not {list(pts.shape)}")
    if pts.shape[0] > MAX_POINTS:
        raise ValueError(f"{pts.shape[0]} points; one joint sweep takes at most {MAX_POINTS}")
    if not np.isfinite(pts).all():
        raise ValueError("points must be finite")
    return np.ascontiguousarray(pts)


def _score_list(scores, e):
    """-> the K score tensors of a joint sweep, each [E] (a view where the caller's tensor allows one)."""
    if torch.is_tensor(scores):
        if scores.dim() != 2:
            raise ValueError("scores must be a sequence of K tensors [E] or [E, 1], or one [K, E] tensor")
        scores = list(scores.unbind(0))
    try:
        scores = list(scores)
    except TypeError:
        raise ValueError("scores must be a sequence of K tensors [E] or [E, 1], or one [K, E] tensor") from None
    if not 1 <= len(scores) <= MAX_SCORES:
        raise ValueError(f"{len(scores)} scores; a joint sweep takes 1 to {MAX_SCORES}")
    out = []
    for k, s in enumerate(scores):
        if not torch.is_tensor(s) or not (s.dim() == 1 or (s.dim() == 2 and s.shape[1] == 1)) or s.numel() != e:
            shape = list(s.shape) if torch.is_tensor(s) else type(s).__name__
            raise ValueError(f"scores[{k}] ({shape}) does not match the batch: [E] or [E, 1] with E={e}")
        out.append(s)
    return out


def sweep_joint(batch, scores, points, keep, frame_div=None, return_labels=False, partition="components"):
    """Scores every frame of `batch` at every point of a CONJUNCTION of K conditions (csrc/eval_sweep_joint.cuh): the rule of the
    reference's position baselines (inference.py:722-724, :896).  `scores`: a sequence of K (1 to 4) device tensors [E] or [E, 1] --
    float32 views with a stride, such as batch.edge_attr[:, 0], are read in place, not copied -- or one [K, E] tensor; `points`: host
    [T, K], finite, at most 16384 rows, any order, duplicates allowed; `keep`: K names out of 'ge', 'gt', 'le', 'lt' (the reference's
    geometric rules are strict 'lt'); `frame_div`: host [K, G] (or [G] when K = 1), finite and > 0, or None.

    At point t in frame g the threshold of condition k is points[t, k] / frame_div[k, g] (one float64 division; points[t, k] itself
    without frame_div: GEOM_TH / max_dist[g], the table value in metres against an attribute that was divided by the frame's max_dist);
    an edge is active iff EVERY condition holds, score_k[e] compared in float64 after widening the float32 score (a NaN score is never
    active); from there on sweep_thresholds' rule: kept iff the reverse edge is active too, the partition the connected components of
    the kept edges, the row evaluate_frames'.  With K = 1, no frame_div and 'ge' / 'le' it returns sweep_thresholds' bits.

    Every argument is checked on the host (ValueError) before the GPU is touched; points and divisors go up through pinned memory
    without a wait; four launches whatever T and K are.  Returns float64 [T, G, 16] on the device, and with return_labels=True also
    int32 [T, N].

    partition='strong': the reference's own rule for these baselines (inference.py:733-738, 904-908) -- nothing is pruned, no reverse
    edge is consulted, and the partition is the strongly connected components of the active edges (csrc/eval_sweep_strong.cuh): rows[t]
    bit for bit evaluate_frames(batch, pred_t, strong_clusters(batch.edge_index, pred_t, ...)['labels']) for the int64 vector pred_t of
    active edges.  Two launches; frames of at most 1024 detections.  partition='exclusive' is a ValueError: the camera-exclusive
    partition is swept for a single score only (sweep_thresholds)."""
    if not isinstance(partition, str) or partition not in JOINT_PARTITIONS:
        raise ValueError(f"partition must be one of {JOINT_PARTITIONS} in a joint sweep (the camera-exclusive partition is swept by "
                         f"sweep_thresholds only), not {partition!r}")
    strong = partition == "strong"
    g, n, e, max_n = _batch_dims(batch)
    sl = _score_list(scores, e)
    k = len(sl)
    if isinstance(keep, str) or keep is None:
        raise ValueError(f"keep must be a sequence of {k} names out of {COMPARATORS}, one per score, not {keep!r}")
    try:
        keep = list(keep)
    except TypeError:
        raise ValueError(f"keep must be a sequence of {k} names out of {COMPARATORS}, one per score, not {keep!r}") from None
    if len(keep) != k or any(not isinstance(c, str) or c not in nat.CMP for c in keep):
        raise ValueError(f"keep must be a sequence of {k} names out of {COMPARATORS}, one per score, not {keep!r}")
    pts = _points(points, k)
    div = None
    if frame_div is not None:
        try:
            div = np.array(frame_div, dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"frame_div must be a [{k}, {g}] array of real numbers ({exc})") from None
        if div.ndim == 1 and k == 1:
            div = div.reshape(1, -1)
        if div.shape != (k, g):
            raise ValueError(f"frame_div must be [{k}, {g}] (one row per score, one column per frame), not {list(div.shape)}")
        if not (np.isfinite(div).all() and (div > 0).all()):
            raise ValueError("frame_div must be finite and > 0")
        div = np.ascontiguousarray(div)
    limit = nat.STRONG_MAX_FRAME_NODES if strong else MAX_FRAME_NODES
    if max_n > limit:
        raise ValueError(f"a frame has {max_n} detections; sweep_joint(partition={partition!r}) scores frames of at most {limit}")
    if batch.edge_labels.numel() != e:
        raise ValueError(f"edge_labels [{batch.edge_labels.numel()}] do not match the batch (E={e})")
    if not all(s.is_cuda for s in sl):
        raise RuntimeError("gnn_cca_amd.calibration runs on MI355X only (no CPU fallback)")
    dev = sl[0].device
    if any(s.device != dev for s in sl):
        raise ValueError("the scores of a joint sweep must be on one device")
    t = int(pts.shape[0])
    with _on(dev):
        flat = []
        for s in sl:
            s = s.reshape(-1)          # ([E, 1] with a row stride: still a view)
            if s.dtype != torch.float32:
                s = s.float()
            if e > 1 and s.stride(0) < 1:
                s = s.contiguous()
            flat.append(s)
        ei = batch.edge_index.contiguous()
        el = batch.edge_labels.contiguous()
        rows, labels, lab_ptr = _outputs(t, g, n, return_labels, dev)
        if g > 0:
            nptr, eptr = _dev_i32(batch.node_ptr_dev, flat[0]), _dev_i32(batch.edge_ptr_dev, flat[0])
            pinned, up = _stage(np.concatenate([pts.reshape(-1)] + ([div.reshape(-1)] if div is not None else [])), dev)   # (one copy for both)
            div_ptr = up.data_ptr() + 8 * t * k if div is not None else None
            ptrs = (nat.C.c_void_p * k)(*[s.data_ptr() if e else None for s in flat])
            strides = (nat.C.c_int64 * k)(*[max(int(s.stride(0)), 1) if e else 1 for s in flat])
            cmps = (nat.C.c_int32 * k)(*[nat.CMP[c] for c in keep])
            _run("gnncca_eval_sweep_strong" if strong else "gnncca_eval_sweep_joint", (n, e, g), dev,   # (one argument list)
                 ei.data_ptr() if e else None, el.data_ptr() if e else None, ptrs, strides, cmps, k, n, e, nptr.data_ptr(), eptr.data_ptr(), g,
                 max_n, up.data_ptr(), t, div_ptr, rows.data_ptr(), lab_ptr)
    return (rows, labels) if return_labels else rows


def grid_points(axes):
    """The Cartesian product of K host sequences in C order (the last axis varies fastest) -> (points float64 [T1 * ... * TK, K], the
    shape (T1, ..., TK)): the points sweep_grid sweeps, for a JointSweepAccumulator over them."""
    try:
        axes = [np.array(a, dtype=np.float64) for a in axes]
    except (TypeError, ValueError) as exc:
        raise ValueError(f"axes must be K sequences of real numbers ({exc})") from None
    if not 1 <= len(axes) <= MAX_SCORES or any(a.ndim != 1 or a.size < 1 for a in axes):
        raise ValueError(f"axes must be 1 to {MAX_SCORES} non-empty one-dimensional sequences, one per score")
    shape = tuple(int(a.size) for a in axes)
    total = int(np.prod(shape, dtype=np.int64))
    if total > MAX_POINTS:
        raise ValueError(f"the grid {' x '.join(map(str, shape))} has {total} points; one joint sweep takes at most {MAX_POINTS}")
    return np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")], axis=1), shape


def sweep_grid(batch, scores, axes, keep, frame_div=None, return_labels=False, partition="components"):
    """sweep_joint over the Cartesian product of K host sequences `axes` (C order: the last axis varies fastest) -- main.py's own 0.01
    step on two axes is 100 x 100 points in one call.  Rows come back viewed as [T1, ..., TK, G, 16] (labels as [T1, ..., TK, N]); a
    product above 16384 points is a ValueError.  `partition`: sweep_joint's ('components' or 'strong')."""
    pts, shape = grid_points(axes)
    out = sweep_joint(batch, scores, pts, keep, frame_div=frame_div, return_labels=return_labels, partition=partition)
    if return_labels:
        rows, labels = out
        return rows.view(*shape, *rows.shape[1:]), labels.view(*shape, labels.shape[1])
    return out.view(*shape, *out.shape[1:])


_COUNT_COLUMNS = tuple(col for _, col, how in AGGREGATES if how == "sum")


class JointSweepAccumulator:
    """The running sums of many batches' sweep_joint / sweep_grid rows over the SAME points.  `add(rows)` makes one launch
    (gnncca_eval_rows_accumulate) and keeps nothing of the batch: the device state is T x 16 doubles and a frame count, whatever the
    data set's size (SweepAccumulator keeps every batch's rows until result(): 82 MB per batch at 10,000 points x 64 frames).  No
    synchronisation before `result()`, which makes one.

    The order of the sums is part of the contract: for every point and column the frames are added one by one onto the running value,
    in the order they were added (within a batch: ascending frame) -- ((s + r0) + r1) + ... in float64.  SweepAccumulator sums with
    torch's reduction, in another order: the means of the two agree within the rounding of a recursive sum, the counts exactly.  A NaN
    row propagates into its point's sums, as it does there."""

    def __init__(self, points):
        try:
            pts = np.array(points, dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"points must be a [T, K] array of real numbers ({exc})") from None
        if pts.ndim != 2 or not 1 <= pts.shape[1] <= MAX_SCORES:
            raise ValueError(f"points must be a [T, K] array with K from 1 to {MAX_SCORES}, not {list(pts.shape)}")
        self.points = _points(pts, pts.shape[1])
        self._state = None      # float64 [T * 16 + 1] on the device: the sums, then the frame count (an int64 in the last 8 bytes)
        self._res = None

    def add(self, rows):
        t = self.points.shape[0]
        if rows.dim() < 3 or rows.shape[-1] != len(METRICS) or rows.dtype != torch.float64 or rows.numel() != t * rows.shape[-2] * 16:
            raise ValueError(f"JointSweepAccumulator.add expects the float64 [{t}, G, 16] rows of sweep_joint (or sweep_grid's view of them)")
        if not rows.is_cuda:
            raise RuntimeError("gnn_cca_amd.calibration runs on MI355X only (no CPU fallback)")
        g = int(rows.shape[-2])
        with _on(rows.device):
            rows = rows.reshape(t, g, 16).contiguous()
            if self._state is None:
                self._state = torch.zeros(t * 16 + 1, dtype=torch.float64, device=rows.device)
            elif self._state.device != rows.device:
                raise ValueError("JointSweepAccumulator.add: rows of another device than the earlier ones")
            st = nat.lib().gnncca_eval_rows_accumulate(rows.data_ptr() if g else None, t, g, self._state.data_ptr(),
                                                       self._state.data_ptr() + 8 * t * 16, _raw_stream(rows.device))
            if st:
                nat.check(st, "gnncca_eval_rows_accumulate")
        self._res = None
        return self

    def result(self):
        """-> dict(points float64 [T, K], frames int, sums float64 [T, 16], aggregates: list of T dicts as EvalAccumulator.result()
        returns them (means = sum / frames, divided on the host in float64; the count columns as int), TP / FP / FN / TN int64 [T],
        P_micro / R_micro / F_micro float64 [T] by SweepAccumulator's expressions); the arrays are on the host."""
        if self._res is not None:
            return self._res
        if self._state is None:
            raise ValueError("JointSweepAccumulator.result: no rows were added")
        host = self._state.cpu().numpy()    # the one synchronisation
        t = self.points.shape[0]
        sums, frames = host[:t * 16].reshape(t, 16).copy(), int(host[t * 16:].view(np.int64)[0])
        if frames == 0:
            raise ValueError("JointSweepAccumulator.result: the rows added hold no frame")
        red = sums / np.float64(frames)
        red[:, _COUNT_COLUMNS] = sums[:, _COUNT_COLUMNS]
        agg = [_aggregates(h) for h in red]
        self._res = _micro_prf({"points": self.points.copy(), "frames": frames, "sums": sums, "aggregates": agg})
        return self._res

    def best(self, metric="F_micro"):
        """Indices of ALL points at which `metric` equals its maximum (SweepAccumulator.best's rule and names)."""
        return _best(self.result(), metric)


__all__ = ["MAX_THRESHOLDS", "MAX_POINTS", "sweep_thresholds", "SweepAccumulator", "sweep_joint", "sweep_grid", "grid_points", "JointSweepAccumulator"]
