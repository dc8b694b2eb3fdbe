"""Per-frame association metrics of a batch on the GPU: the scoring at the end of the reference's evaluation loop (inference.py:349-371)
and the aggregation main.py:335-348 makes of it, without copying frames to the host or calling scikit-learn per frame.

    rows = evaluate_frames(batch, predictions, labels)       # float64 [G, 16] on the device, columns METRICS; one launch, no sync
    rows = r.evaluate()                                      # r: a pipeline.FrameResult (its final() predictions / labels)
    rows = evaluate_frames(batch, predictions, labels, against='dense')   # a capped batch (top_k=k) scored as the dense graph, every
    rows = r.evaluate(against='dense')                                    # dropped edge predicted 0: comparable with a dense run
    acc = EvalAccumulator(); acc.add(rows) ...; acc.result() # {'P': ..., 'R': ..., 'TP': ..., 'RI': ..., 'MI': ...} as main.py prints them

Per frame (csrc/evaluate.hip, one workgroup each): TP / FP / FN / TN, P, R, F and the two per-class precisions exactly as
`compute_P_R_F` (inference.py:23-68) writes them; ID_GT = connected components of the edges with label 1 (the reference's strongly
connected components of that symmetric edge set, inference.py:296-299); ARI, AMI (arithmetic normaliser), homogeneity, completeness and
V-measure between ID_GT and the predicted partition; and the two cluster counts.  The counts, P, R, F, the precisions and ARI are bit for
bit the reference's expressions; homogeneity / completeness / V agree to ~1e-12 and AMI to ~1e-9 (its expected mutual information is
summed over distinct cluster sizes, in another order).

The formulas and special cases are scikit-learn 1.7.2's, which produced the goldens (tests/golden/make_golden_eval.py); the reference pins
scikit-learn 0.24.2 (env_gnn.yml:106).  Known differences of 0.24.2 from 1.7.2 in the degenerate cases: its adjusted_rand_score computes
the same pair counts but in numpy int64 rather than Python integers (the same values below 2^53, as here); its adjusted_mutual_info_score
returns 1.0 for two one-cluster (or empty) labellings as 1.7.2 does, but divides the unclamped MI - EMI (1.7.2 also keeps the numerator
at least eps away from zero), and its mutual_info_score does not zero the per-cell terms below eps: the two can differ by ~1e-16 on frames
whose MI equals its expectation.  (These come from the scikit-learn changelogs, not from a run of 0.24.2.)
Frames of more than 4096 detections are refused (ValueError)."""
import numpy as np
import torch

from . import _native as nat
from .frames import _on, _raw_stream

METRICS = ("P", "R", "F", "TP", "FP", "FN", "TN", "rand_index", "mutual_index", "homogeneity", "completeness", "v_measure",
           "precision0", "precision1", "n_clusters_gt", "n_clusters_pred")
MAX_FRAME_NODES = 4096
# main.py:335-348: (name, column, reduction)
AGGREGATES = (("P", 0, "mean"), ("R", 1, "mean"), ("F", 2, "mean"), ("TP", 3, "sum"), ("FP", 4, "sum"), ("FN", 5, "sum"), ("TN", 6, "sum"),
              ("RI", 7, "mean"), ("MI", 8, "mean"), ("hom", 9, "mean"), ("com", 10, "mean"), ("v", 11, "mean"), ("prec0", 12, "mean"),
              ("prec1", 13, "mean"))


def _dev_i32(t, like):
    return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(device=like.device, dtype=torch.int32).contiguous()


AGAINST = ("kept", "dense")


def evaluate_frames(batch, predictions, labels, gt_labels=False, against="kept"):
    """Scores every frame of `batch` (a GraphBatch with edge_index, edge_labels, host node_ptr / edge_ptr and device node_ptr_dev /
    edge_ptr_dev, as graph_build.build_graph_batch and pipeline.FramePipeline make it) against `predictions` int64 [E] (0/1) and
    `labels` int32 [N] (the predicted partition, a node's label the smallest node id of its cluster).  Enqueued on the current stream;
    returns float64 [G, 16] (columns METRICS) on the device, and with gt_labels=True also ID_GT as int32 [N] in the same convention.

    against='kept' (the default) scores the batch's own edges: on a capped batch (top_k=k) a same-identity pair the cap dropped is
    neither a hit nor a miss, and ID_GT is made of the kept label-1 edges.  against='dense' scores a capped batch as the DENSE graph would
    have been scored with every dropped edge predicted 0 (no counterpart in the reference, which has no capped graph): TP and FP as
    before; FN grows by the dropped label-1 ordered pairs and TN by the dropped label-0 ones (counted from the per-frame person ids and
    cameras: ordered cross-camera pairs with the same / a different id, minus the kept ones); ID_GT is the dense graph's -- all
    detections of an identity seen on at least two cameras form one component, every other detection its own; P, R, F, the class
    precisions and the clustering scores are the same expressions on those inputs.  It needs batch.person_dev / batch.cam_dev (int32 [N]
    on the device: build_graph_batch and FramePipeline provide them), runs in the same one-workgroup-per-frame launch and does not
    synchronise; on a dense batch it returns the default's rows."""
    if against not in AGAINST:
        raise ValueError(f"against must be 'kept' or 'dense', not {against!r}")
    dense = against == "dense"
    if dense and (getattr(batch, "person_dev", None) is None or getattr(batch, "cam_dev", None) is None):
        raise ValueError("evaluate_frames(against='dense') needs batch.person_dev and batch.cam_dev (int32 [N] on the device)")
    node_ptr = np.asarray(batch.node_ptr, dtype=np.int64)
    g = len(node_ptr) - 1
    n = int(node_ptr[-1]) if g > 0 else 0
    e = int(batch.edge_index.shape[1])
    max_n = int(np.diff(node_ptr).max()) if g > 0 else 0
    if max_n > MAX_FRAME_NODES:
        raise ValueError(f"a frame has {max_n} detections; evaluate_frames scores frames of at most {MAX_FRAME_NODES}")
    dev = labels.device
    if not labels.is_cuda:
        raise RuntimeError("gnn_cca_amd.evaluation runs on MI355X only (no CPU fallback)")
    if labels.numel() != n or predictions.numel() != e or batch.edge_labels.numel() != e:
        raise ValueError(f"predictions [{predictions.numel()}] / labels [{labels.numel()}] do not match the batch (E={e}, N={n})")
    lib = nat.lib()
    with _on(dev):
        ei = batch.edge_index.contiguous()
        el = batch.edge_labels.contiguous()
        pr = predictions.to(torch.int64).contiguous()
        lb = labels.to(torch.int32).contiguous()
        nptr, eptr = _dev_i32(batch.node_ptr_dev, lb), _dev_i32(batch.edge_ptr_dev, lb)
        out = torch.empty((g, 16), dtype=torch.float64, device=dev)
        gt = torch.empty(n, dtype=torch.int32, device=dev) if gt_labels else None
        ws_bytes = lib.gnncca_eval_workspace_bytes(n, e, g)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        if dense:
            person, cam = _dev_i32(batch.person_dev, lb), _dev_i32(batch.cam_dev, lb)
            if person.numel() != n or cam.numel() != n:
                raise ValueError(f"batch.person_dev [{person.numel()}] / batch.cam_dev [{cam.numel()}] do not match the batch (N={n})")
            st = lib.gnncca_eval_frames_dense(ei.data_ptr() if e else None, el.data_ptr() if e else None, pr.data_ptr() if e else None,
                                              lb.data_ptr() if n else None, person.data_ptr() if n else None, cam.data_ptr() if n else None,
                                              n, e, nptr.data_ptr(), eptr.data_ptr(), g, max_n, gt.data_ptr() if gt_labels and n else None,
                                              out.data_ptr(), ws.data_ptr(), ws_bytes, _raw_stream(dev))
        else:
            st = lib.gnncca_eval_frames(ei.data_ptr() if e else None, el.data_ptr() if e else None, pr.data_ptr() if e else None,
                                        lb.data_ptr() if n else None, n, e, nptr.data_ptr(), eptr.data_ptr(), g, max_n,
                                        gt.data_ptr() if gt_labels and n else None, out.data_ptr(), ws.data_ptr(), ws_bytes, _raw_stream(dev))
        if st:
            nat.check(st, "gnncca_eval_frames")
        # the workspace is freed by the caching allocator in stream order (it was allocated on this stream): nothing to keep
    return (out, gt) if gt_labels else out


def _reduce_rows(allr):
    """The ONE definition of main.py:335-348's reduction of float64 [F, 16] rows: sums of the count columns, means of the others, in
    float64 and in a fixed order (torch's sum over one contiguous tensor) -> float64 [16] on the device, no synchronisation.
    EvalAccumulator and calibration.SweepAccumulator both reduce with it."""
    sums = allr.sum(dim=0)
    return torch.where(torch.tensor([0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1], dtype=torch.bool, device=allr.device),
                       sums, sums / allr.shape[0])


def _aggregates(host):
    """A reduced row on the host -> {'P': ..., 'TP': ...} as main.py prints them."""
    return {name: (int(host[col]) if how == "sum" else float(host[col])) for name, col, how in AGGREGATES}


class EvalAccumulator:
    """Collects the device rows of many batches (`add`, no synchronisation) and reduces them ONCE (`result`): the aggregates main.py:335-348
    prints -- means of P, R, F, RI, MI, hom, com, v, prec0, prec1 and sums of TP, FP, FN, TN over all frames -- in float64, in a fixed
    order (torch's sum over one concatenated tensor), with one synchronisation."""

    def __init__(self):
        self._rows = []

    def add(self, rows):
        if rows.dim() != 2 or rows.shape[1] != len(METRICS) or rows.dtype != torch.float64:
            raise ValueError("EvalAccumulator.add expects the float64 [G, 16] rows of evaluate_frames")
        self._rows.append(rows)
        return self

    def __len__(self):
        return sum(int(r.shape[0]) for r in self._rows)

    def result(self):
        if not self._rows:
            raise ValueError("EvalAccumulator.result: no rows were added")
        allr = torch.cat(self._rows) if len(self._rows) > 1 else self._rows[0]
        host = _reduce_rows(allr).cpu().numpy()       # the one synchronisation
        return _aggregates(host)


__all__ = ["METRICS", "MAX_FRAME_NODES", "evaluate_frames", "EvalAccumulator"]
