"""The training loss of the reference and the statistics it logs, on the GPU: `compute_loss_acc` (train.py:51-208), the per-step,
per-class mean probabilities (train.py:460-469) and the six `AverageMeter`s (train.py:472-479), without a host round trip.

    loss_fn = EdgeLoss('BCE_weighted', pos_weight=4.5, meters=TrainMeters(capacity=len(loader), n_steps=S))
    step = GraphedTrainStep(model, optimizer, loss_fn)           # the loss_fn slot, unchanged
    for data, labels in loader:
        step(data, labels)                                       # every replay appends one row to the meters, on the device
    stats = loss_fn.meters.result(batch_size=B)                  # one synchronisation per epoch
    loss_fn.meters.reset()

`EdgeLoss(outputs, labels)` returns the scalar loss (fp32, differentiable); the forward is two launches over the [S, E] logits (per-edge
terms in fp32, fp64 sums in a fixed order) and the backward one elementwise launch (csrc/loss.hip).  The criteria are those of
main_training.py:258-268: 'BCE', 'BCE_weighted' (pos_weight) and 'Focal' (utils.FocalLoss_binary: its focal factor is applied to the
step's MEAN BCE for the loss and to every edge's BCE for the per-class losses).  mode='validate' uses plain BCE with logits whatever the
criterion, as compute_loss_acc does.
"""
import numpy as np
import torch

from . import _native as nat
from .frames import _on, _raw_stream

CRITERIA = {"BCE": 0, "BCE_weighted": 1, "Focal": 2}
MODES = ("train", "validate")
FIELDS = ("loss", "loss_class1", "loss_class0", "precision1", "precision0", "precision", "n_pos", "n_neg")
METERS = ("loss", "loss_class1", "loss_class0", "precision1", "precision0", "precision")   # train.py:472-479, in that order
MAX_STEPS = 64


def record_len(n_steps):
    """fp64 words of one record: FIELDS, mean_prob [S][2] (class 0, class 1), coef [S] (d loss / d mean BCE of each step)."""
    return len(FIELDS) + 3 * int(n_steps)


class LossRecord:
    """One call's statistics as device tensors (views of `record`, fp64): FIELDS as 0-d tensors, mean_prob [S, 2], coef [S]."""

    def __init__(self, record, n_steps):
        self.record = record
        for q, name in enumerate(FIELDS):
            setattr(self, name, record[q])
        k = len(FIELDS)
        self.mean_prob = record[k:k + 2 * n_steps].view(n_steps, 2)
        self.coef = record[k + 2 * n_steps:k + 3 * n_steps]


def _steps_tensor(ce):
    """The [S, E, 1] tensor whose unbind(0) `ce` is (no copy), else the stacked steps as [S, E]."""
    t0 = ce[0]
    base = t0._base if torch.is_tensor(t0) else None
    if base is not None and base.dim() == 3 and base.shape[0] == len(ce) and base.shape[2] == 1 and base.is_contiguous():
        e = base.shape[1]
        if all(torch.is_tensor(t) and t._base is base and tuple(t.shape) == (e, 1)
               and t.storage_offset() == base.storage_offset() + s * e for s, t in enumerate(ce)):
            return base
    shapes = {tuple(t.shape) for t in ce}
    if any(t.numel() != ce[0].numel() for t in ce):
        raise ValueError(f"EdgeLoss: the classified steps differ in length ({sorted(shapes)})")
    return torch.stack([t.reshape(-1) for t in ce])


class _EdgeLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, owner):
        s = int(logits.shape[0])
        e = int(logits.shape[1])
        lib = nat.lib()
        dev = logits.device
        with _on(dev):
            x = logits.detach()
            loss = torch.empty((), dtype=torch.float32, device=dev)
            record = torch.empty(record_len(s), dtype=torch.float64, device=dev)
            ws_bytes = lib.gnncca_edge_loss_workspace_bytes(s, e)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            m = owner.meters
            hist, cap, cur = (m.history.data_ptr(), m.capacity, m.cursor.data_ptr()) if m is not None else (None, 0, None)
            st = lib.gnncca_edge_loss_forward(x.data_ptr() if e else None, labels.data_ptr() if e else None, s, e, owner._crit,
                                              owner._validate, owner._pw, owner._gamma, owner._alpha, loss.data_ptr(), record.data_ptr(),
                                              hist, cap, cur, ws.data_ptr(), ws_bytes, _raw_stream(dev))
            if st:
                nat.check(st, "gnncca_edge_loss_forward")
        ctx.owner = owner
        ctx.save_for_backward(x, labels, record)
        owner.last = LossRecord(record, s)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, labels, record = ctx.saved_tensors
        owner = ctx.owner
        s, e = int(x.shape[0]), int(x.shape[1])
        dev = x.device
        with _on(dev):
            g = g.to(torch.float32).contiguous()
            grad = torch.empty_like(x)
            st = nat.lib().gnncca_edge_loss_backward(x.data_ptr() if e else None, labels.data_ptr() if e else None, s, e, owner._crit,
                                                     owner._validate, owner._pw, g.data_ptr(), record.data_ptr(),
                                                     grad.data_ptr() if e else None, _raw_stream(dev))
            if st:
                nat.check(st, "gnncca_edge_loss_backward")
        return grad, None, None


class EdgeLoss:
    """compute_loss_acc's loss and statistics as one callable: `loss = EdgeLoss(...)(outputs, labels)`, outputs the dict the MPN returns
    ({'classified_edges': [Tensor[E, 1], ...]}), labels fp32 [E] (batch.edge_labels).  `.last` holds the LossRecord of the latest call
    (device tensors; for a call captured into a graph, the tensors that every replay rewrites).  With `meters` (a TrainMeters), every
    call -- eager or replayed -- appends its record on the device."""

    def __init__(self, criterion="BCE", pos_weight=None, focusing_param=5, balance_param=0.9, mode="train", meters=None):
        if criterion not in CRITERIA:
            raise ValueError(f"EdgeLoss: criterion must be one of {sorted(CRITERIA)}, not {criterion!r}")
        if mode not in MODES:
            raise ValueError(f"EdgeLoss: mode must be 'train' or 'validate', not {mode!r}")
        if criterion == "BCE_weighted":
            if pos_weight is None or not float(pos_weight) > 0.0:
                raise ValueError("EdgeLoss: 'BCE_weighted' needs pos_weight > 0 (POSITIVE_WEIGHT of the dataset)")
        self.criterion, self.mode, self.meters = criterion, mode, meters
        self.pos_weight = None if pos_weight is None else float(pos_weight)
        self.focusing_param, self.balance_param = float(focusing_param), float(balance_param)
        self._crit, self._validate = CRITERIA[criterion], int(mode == "validate")
        self._pw = self.pos_weight if criterion == "BCE_weighted" else 1.0
        self._gamma, self._alpha = self.focusing_param, self.balance_param
        self.last = None

    def __call__(self, outputs, labels):
        ce = outputs["classified_edges"] if isinstance(outputs, dict) else outputs
        if len(ce) == 0:
            raise ValueError("EdgeLoss: no classified steps")
        if len(ce) > MAX_STEPS:
            raise ValueError(f"EdgeLoss: at most {MAX_STEPS} classified steps")
        if not (all(t.is_cuda for t in ce) and labels.is_cuda):
            raise RuntimeError("gnn_cca_amd.loss runs on MI355X only (no CPU fallback): logits and labels must be on the GPU")
        logits = _steps_tensor(ce)
        if logits.dtype != torch.float32 or labels.dtype != torch.float32:
            raise ValueError(f"EdgeLoss: logits and labels must be float32 (got {logits.dtype}, {labels.dtype})")
        if logits.device != labels.device:
            raise ValueError("EdgeLoss: logits and labels are on different devices")
        e = int(logits.shape[1])
        if labels.numel() != e:
            raise ValueError(f"EdgeLoss: {labels.numel()} labels for {e} edges")
        if self.meters is not None:
            if self.meters.n_steps != len(ce):
                raise ValueError(f"EdgeLoss: the meters hold {self.meters.n_steps} steps, the outputs have {len(ce)}")
            if self.meters.history.device != logits.device:
                raise ValueError("EdgeLoss: the meters live on another device")
        return _EdgeLossFunction.apply(logits, labels.detach().reshape(-1).contiguous(), self)


def average_meter(values, n):
    """libs/utils.py's AverageMeter fed `values` in order with weight n: (val, sum, count, avg), Python floats reduced sequentially."""
    val, total, count, avg = 0, 0, 0, 0
    for v in values:
        val = v
        total += v * n
        count += n
        avg = total / count
    return val, total, count, avg


def reduce_history(rows, n_steps, batch_size=1):
    """The host side of TrainMeters.result(): rows float64 [K, record_len(S)] in iteration order -> per quantity the per-iteration values
    as the reference's meters receive them (the losses as the fp32 `.item()`s, the precisions in float64) and the AverageMeter state;
    the mean probabilities per iteration (float32, as torch.mean returns them) and their epoch entry (np.mean over the iterations, the
    list_mean_probs_history entry of train.py:508-514)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, record_len(n_steps))
    out = {"iterations": int(rows.shape[0])}
    for q, name in enumerate(METERS):
        col = rows[:, q]
        vals = [float(np.float32(v)) for v in col] if q < 3 else [float(v) for v in col]
        val, total, count, avg = average_meter(vals, batch_size)
        out[name] = {"values": vals, "val": val, "sum": total, "count": count, "avg": avg}
    out["n_pos"] = rows[:, 6].astype(np.int64)
    out["n_neg"] = rows[:, 7].astype(np.int64)
    k = len(FIELDS)
    probs = rows[:, k:k + 2 * n_steps].reshape(-1, n_steps, 2).astype(np.float32)
    out["mean_probs"] = {c: {f"step{s}": probs[:, s, int(c)].copy() for s in range(n_steps)} for c in ("0", "1")}
    out["mean_probs_epoch"] = {c: {f"step{s}": (np.mean(probs[:, s, int(c)]) if len(probs) else np.float32(np.nan))
                                   for s in range(n_steps)} for c in ("0", "1")}
    return out


class TrainMeters:
    """The device history EdgeLoss appends to: fp64 [capacity, record_len(n_steps)] plus a cursor word and an overflow word, both written
    by the kernel (so a replayed graph fills successive rows).  `result(batch_size)` synchronises once and reduces on the host
    (reduce_history); `reset()` starts a new epoch in place, so graphs that captured these buffers stay valid."""

    def __init__(self, capacity, n_steps, device=None):
        if int(capacity) < 1 or not 1 <= int(n_steps) <= MAX_STEPS:
            raise ValueError(f"TrainMeters: capacity >= 1 and 1 <= n_steps <= {MAX_STEPS}")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("gnn_cca_amd.loss.TrainMeters runs on MI355X only (no CPU fallback)")
        self.capacity, self.n_steps = int(capacity), int(n_steps)
        self.history = torch.zeros((self.capacity, record_len(n_steps)), dtype=torch.float64, device=dev)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=dev)   # [next row, overflow]

    def reset(self):
        self.cursor.zero_()
        return self

    def rows(self):
        """(rows float64 [K, record_len] on the host, overflow flag) with one synchronisation."""
        with _on(self.history.device):
            h = torch.empty(self.history.shape, dtype=self.history.dtype, pin_memory=True)
            c = torch.empty(2, dtype=torch.int64, pin_memory=True)
            h.copy_(self.history, non_blocking=True)
            c.copy_(self.cursor, non_blocking=True)
            torch.cuda.current_stream(self.history.device).synchronize()
        k, overflow = int(c[0]), bool(c[1])
        return h[:k].numpy().copy(), overflow

    def result(self, batch_size=1):
        rows, overflow = self.rows()
        if overflow:
            raise RuntimeError(f"TrainMeters: more than {self.capacity} iterations since reset(); the rows past capacity were dropped")
        return reduce_history(rows, self.n_steps, batch_size)


__all__ = ["CRITERIA", "FIELDS", "METERS", "EdgeLoss", "LossRecord", "TrainMeters", "average_meter", "reduce_history", "record_len"]
