"""`optimizer.step()` of the reference's training loop (train.py:492-494) in one HIP launch per parameter group (csrc/optim.hip), for the
two optimizers main_training.py:220-256, 349-370 builds:

    optimizer = FusedSGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)      # torch.optim.SGD's arguments
    optimizer = FusedAdam(model.parameters(), lr=1e-3)                                      # torch.optim.Adam's

Both are `torch.optim.Optimizer`s: `param_groups[0]['lr'] = x`, `torch.optim.lr_scheduler.*`, `zero_grad`, `state_dict()` /
`load_state_dict()` (interchangeable with the torch classes' in both directions) work as on the torch optimizers.  What differs is where
the hyperparameters live: the kernel reads `lr`, `momentum`, ... and every step count from a small device block, so a training step
captured into a HIP graph (`GraphedTrainStep`) keeps following a learning-rate schedule -- `torch.optim.SGD` freezes the Python numbers of
the capture into the graph.  `sync_hyperparameters()` uploads a group's values when they differ from what the block holds; `step()`
calls it in eager mode, `GraphedTrainStep` before every replay.
"""
import ctypes as C

import torch

from . import _native as nat
from .frames import _on, _raw_stream

_REFUSED = ("maximize", "differentiable", "decoupled_weight_decay")


class _FusedOptimizer(torch.optim.Optimizer):
    _RULE = None
    _STATE_KEYS = ()

    def __init__(self, params, defaults):
        self._blocks = []      # per parameter group: the device block (uint8 tensor) or None until the group's first use
        self._uploaded = []    # per parameter group: the hyperparameter tuple the block holds
        super().__init__(params, defaults)

    # -- what this optimizer refuses ---------------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
        except Exception:
            self.param_groups.pop()
            raise
        self._blocks.append(None)
        self._uploaded.append(None)

    def _check_group(self, group):
        name = type(self).__name__
        for key in _REFUSED:
            if group.get(key, False):
                raise ValueError(f"{name} does not implement {key}=True (use torch.optim for it)")
        for p in group["params"]:
            if not p.is_cuda:
                raise ValueError(f"{name} runs on MI355X only: move the model to the GPU before building the optimizer "
                                 f"(got a parameter on {p.device}; there is no CPU fallback)")
            if p.dtype != torch.float32:
                raise TypeError(f"{name} updates float32 parameters only, got {p.dtype}")
            if p.is_sparse or p.layout != torch.strided:
                raise TypeError(f"{name} updates dense parameters only")
        devices = {p.device for p in group["params"]}
        if len(devices) > 1:
            raise ValueError(f"{name}: the parameters of one group live on several devices ({sorted(map(str, devices))})")

    def _hyper(self, group):
        """(lr, weight_decay, a, b, c, flag) of gnncca_optim_set_hyper for a group, as Python numbers."""
        raise NotImplementedError

    # -- the device block --------------------------------------------------------------------------------------------------------
    def _block(self, gi):
        while len(self._blocks) < len(self.param_groups):   # (groups restored by load_state_dict / __setstate__)
            self._blocks.append(None)
            self._uploaded.append(None)
        blk = self._blocks[gi]
        if blk is None:
            params = self.param_groups[gi]["params"]
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: call sync_hyperparameters() (or take one eager step) before capturing a "
                                   "step into a graph: the device block of the hyperparameters cannot be created inside a capture")
            dev = params[0].device
            with _on(dev):
                blk = torch.zeros(nat.lib().gnncca_optim_block_bytes(len(params)), dtype=torch.uint8, device=dev)
            self._blocks[gi] = blk
        return blk

    def _steps(self, gi):
        """The group's step counts: an int32 view of its block, one entry per parameter of the group."""
        n = len(self.param_groups[gi]["params"])
        o = nat.OPTIM_BLOCK_STEPS_OFFSET
        return self._block(gi)[o:o + 4 * n].view(torch.int32)

    def sync_hyperparameters(self):
        """Enqueue, on the current stream, the upload of every group's hyperparameters that differ from what its device block holds;
        nothing otherwise.  Inside a stream capture nothing is enqueued (the values would be frozen into the graph): sync before the
        capture and before every replay, as GraphedTrainStep does."""
        if torch.cuda.is_current_stream_capturing():
            return
        for gi, group in enumerate(self.param_groups):
            if not group["params"]:
                continue
            for key in _REFUSED:
                if group.get(key, False):
                    raise ValueError(f"{type(self).__name__} does not implement {key}=True (use torch.optim for it)")
            h = self._hyper(group)
            blk = self._block(gi)
            if self._uploaded[gi] == h:
                continue
            lr, wd, a, b, c, flag = h
            dev = blk.device
            with _on(dev):
                st = nat.lib().gnncca_optim_set_hyper(blk.data_ptr(), self._RULE, lr, wd, a, b, c, int(flag), _raw_stream(dev))
            if st == nat.ERR_INVALID_ARG:
                raise ValueError(f"{type(self).__name__}: illegal hyperparameters in group {gi}: "
                                 f"{ {k: v for k, v in group.items() if k != 'params'} }")
            nat.check(st, "gnncca_optim_set_hyper")
            self._uploaded[gi] = h

    # -- the step ----------------------------------------------------------------------------------------------------------------
    def _new_state(self, group, p):
        """Creates the state tensors a parameter needs for its group's settings (no-op where they exist) -> (s0, s1, s2) or Nones."""
        raise NotImplementedError

    def _launch(self, lib, blk, n_slots, n, pp, gp, s, ne, sl, stream):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.sync_hyperparameters()
        lib = nat.lib()
        for gi, group in enumerate(self.param_groups):
            todo = []
            for slot, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.layout != torch.strided:
                    raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise RuntimeError(f"{type(self).__name__}: gradient {g.dtype} {tuple(g.shape)} on {g.device} does not match its "
                                       f"float32 parameter {tuple(p.shape)} on {p.device}")
                if not p.is_contiguous():
                    raise RuntimeError(f"{type(self).__name__} needs contiguous parameters")
                todo.append((slot, p, g if g.is_contiguous() else g.contiguous(), self._new_state(group, p)))
            if not todo:
                continue
            blk = self._block(gi)
            dev = blk.device
            n = len(todo)
            pp = (C.c_void_p * n)(*[p.data_ptr() for _, p, _, _ in todo])
            gp = (C.c_void_p * n)(*[g.data_ptr() for _, _, g, _ in todo])
            s = [(C.c_void_p * n)(*[(st[k].data_ptr() if st[k] is not None else None) for _, _, _, st in todo]) for k in range(3)]
            ne = (C.c_int64 * n)(*[p.numel() for _, p, _, _ in todo])
            sl = (C.c_int32 * n)(*[slot for slot, _, _, _ in todo])
            with _on(dev):
                st = self._launch(lib, blk.data_ptr(), len(group["params"]), n, pp, gp, s, ne, sl, _raw_stream(dev))
            nat.check(st, f"{type(self).__name__}.step")
            # the kernel wrote through raw pointers: tell autograd (and MOTMPNet's packed-weight cache, which keys on the versions)
            for _, p, _, _ in todo:
                torch.autograd.graph.increment_version(p)
        return loss

    # -- checkpoints: the dictionaries of torch.optim.SGD / Adam -------------------------------------------------------------------
    def _export_counts(self, gi, group):
        """Writes what the device step counts mean for state_dict() into self.state (Adam: the 'step' entries; may synchronise)."""

    def _import_counts(self, group):
        """The step counts that a loaded state implies -> list of ints, one per parameter of the group."""
        raise NotImplementedError

    def state_dict(self):
        for gi, group in enumerate(self.param_groups):
            if group["params"] and gi < len(self._blocks) and self._blocks[gi] is not None:
                self._export_counts(gi, group)
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        old = {p: dict(st) for p, st in self.state.items()}
        super().load_state_dict(state_dict)
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            for p in group["params"]:
                new, was = self.state.get(p), old.get(p)
                if not new:
                    continue
                for k in self._STATE_KEYS:   # keep the addresses captured graphs hold: copy into the tensors that exist already
                    t = new.get(k)
                    if torch.is_tensor(t):
                        t = t.to(device=p.device, dtype=torch.float32).contiguous()
                        keep = was.get(k) if was else None
                        if torch.is_tensor(keep) and keep.shape == t.shape and keep.device == t.device:
                            keep.copy_(t)
                            t = keep
                        new[k] = t
            if group["params"]:
                counts = self._import_counts(group)
                self._steps(gi).copy_(torch.tensor(counts, dtype=torch.int32))
        self._uploaded = [None] * len(self.param_groups)


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD (weight_decay, momentum, dampening, nesterov) as one launch per parameter group."""
    _RULE = nat.OPTIM_SGD
    _STATE_KEYS = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        # (the keys, and their order, of torch.optim.SGD's param_groups: the two classes' state_dict()s are interchangeable)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused))

    def _hyper(self, group):
        return (float(group["lr"]), float(group["weight_decay"]), float(group["momentum"]), float(group["dampening"]), 0.0,
                bool(group["nesterov"]))

    def _new_state(self, group, p):
        if group["momentum"] == 0:
            return (None, None, None)
        st = self.state[p]
        buf = st.get("momentum_buffer")
        if buf is None:
            # not initialised: the kernel does not read the buffer on the step that finds the slot's count at 0, it writes b = g
            buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
        return (buf, None, None)

    def _launch(self, lib, blk, n_slots, n, pp, gp, s, ne, sl, stream):
        return lib.gnncca_optim_sgd_step(blk, n_slots, n, pp, gp, s[0], ne, sl, stream)

    def _import_counts(self, group):
        # only "has this buffer seen a step" matters to the rule
        return [1 if torch.is_tensor(self.state.get(p, {}).get("momentum_buffer")) else 0 for p in group["params"]]


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam (betas, eps, L2 weight_decay, amsgrad) as one launch per parameter group; the step counts advance on the device."""
    _RULE = nat.OPTIM_ADAM
    _STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=decoupled_weight_decay))

    def _hyper(self, group):
        b1, b2 = group["betas"]
        return (float(group["lr"]), float(group["weight_decay"]), float(b1), float(b2), float(group["eps"]), bool(group["amsgrad"]))

    def _new_state(self, group, p):
        st = self.state[p]
        keys = self._STATE_KEYS if group["amsgrad"] else self._STATE_KEYS[:2]
        for k in keys:
            if not torch.is_tensor(st.get(k)):
                st[k] = torch.empty_like(p, memory_format=torch.contiguous_format)   # taken as zero on the slot's first step, not read
        if "step" not in st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)   # torch's entry; the live count is on the device (see state_dict)
        return (st["exp_avg"], st["exp_avg_sq"], st.get("max_exp_avg_sq") if group["amsgrad"] else None)

    def _launch(self, lib, blk, n_slots, n, pp, gp, s, ne, sl, stream):
        return lib.gnncca_optim_adam_step(blk, n_slots, n, pp, gp, s[0], s[1], s[2], ne, sl, stream)

    def _export_counts(self, gi, group):
        for p, c in zip(group["params"], self._steps(gi).cpu().tolist()):
            if p in self.state and self.state[p]:
                self.state[p]["step"] = torch.tensor(float(c), dtype=torch.float32)

    def _import_counts(self, group):
        return [int(round(float(self.state[p]["step"]))) if p in self.state and "step" in self.state[p] else 0 for p in group["params"]]

    def step_counts(self):
        """The device step counts, one list per parameter group (synchronises)."""
        return [self._steps(gi).cpu().tolist() if g["params"] else [] for gi, g in enumerate(self.param_groups)]
