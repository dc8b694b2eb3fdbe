"""Trajectories from track ids: a constant-velocity Kalman filter along every track, a stage behind tracking.FrameLinker, on the GPU and
without a host wait.

    link = FrameLinker(max_step=0.8, max_gap=2)
    smooth = TrackSmoother(link, process_noise=0.01, measurement_noise=0.0025, vel_var=1.0)   # per_detection=False
    t = link(r)                                    # Tracks, as ever
    tr = smooth(r, t)                              # Trajectories: pos / vel [N, 2], cov [N, 3], nis [N], age [N], rows as cluster_track
    t = link(r2, times=ts); tr = smooth(r2, t, times=ts)   # a timed linker: the same times to both

The tracking chain ends in ids; ClusterSummaries.pos is the raw fused position of one frame and Tracks.velocity (motion='velocity') one
subtraction and one division.  The smoother filters AFTER linking: it consumes the links the linker made (matched_prev, matched_gap, the
time stamps if any), decides nothing and gates nothing, and works behind every linker mode (with max_gap = 0, where Tracks.matched_gap is
derived from matched_prev, too); kalman.KalmanLinker runs the same filter INSIDE the linker, where it predicts and gates.  The reference has
no counterpart.

The rule (include/gnncca_mpn.h has it word for word, tests/track_smooth_oracle.py as numpy loops).  The two ground-plane axes are
independent and share one 2 x 2 covariance (a, b, c) = (var pos, cov pos/vel, var vel).  q = process_noise (finite, >= 0), r =
measurement_noise (a variance; finite, > 0), vel_var (finite, > 0); with per_detection the measurement variance of a cluster is
re = r / float64(size) -- a cluster fused from more detections is trusted more -- else re = r.  For cluster a of frame t, z = pos(a):
  Birth (matched_gap(a) == -1):  p = z, v = (0, 0), (a, b, c) = (re, 0, vel_var), age = 0, nis = 0.
  Link to cluster m = matched_prev(a) of frame t - 1 - k, k = matched_gap(a):  dt = float64(k + 1), with time stamps T[t] - T[t - 1 - k]
  (frames counted among frames present, as the linker counts them); from that cluster's filtered state, one fp64 operation per
  operator, left to right, no FMA:
    dt2 = dt*dt;  dt3 = dt2*dt;  pp = p + dt*v
    a_ = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0;  b_ = (b + dt*c) + (q*dt2)/2.0;  c_ = c + q*dt
    s = a_ + re;  k1 = a_/s;  k2 = b_/s;  i = z - pp
    p' = pp + k1*i;  v' = v + k2*i;  a' = a_ - k1*a_;  b' = b_ - k1*b_;  c' = c_ - k2*b_
    nis = (ix*ix + iy*iy)/s;  age' = age + 1
Non-finite inputs propagate.  Rows at or beyond a frame's count, and every row of a refused frame, are zero with age = -1.  The rule is
causal along predecessor links only, so the result does not depend on how a sequence is cut into calls: the smoother carries the
filtered state of the rows of the last max_gap + 1 frames, aligned with the linker's kept frames.
Kernels (csrc/identities_smooth.cuh): three launches whatever max_gap and the number of frames are, kernels only -- the workspace is
cleared, every linked cluster writes its row into its predecessor's successor slot, then the head of every chain walks it; tracks are
independent, so all chains go side by side and no workgroup waits for another.  Nothing is read back; a call can be captured in a HIP
graph and replayed.
Limits: constant velocity and one (q, r) for all tracks: a sharp turn shows as a large nis, it is not followed faster; nis is per link,
chi-square with two degrees of freedom only if q and r are right; the smoother follows the linker's links only -- a track that
reentry.TrackGallery re-attaches starts a fresh filter; `tracks` must come from the linker the smoother was built with, for the same
summaries, every batch of the sequence in order.  DESIGN.md section 9 has call times and what it does to position and velocity error on
synthetic walks with ground-truth clusters; with a trained model it has not been measured.
No CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as nat
from .frames import _on, _raw_stream
from .tracking import MAX_FRAME_NODES, ClusterSummaries, FrameLinker, Tracks, _real


class Trajectories:
    """What one TrackSmoother call returns (device tensors, row-aligned with Tracks.cluster_track): pos, vel float64 [N, 2] (filtered
    position and velocity per frame period), cov float64 [N, 3] (var pos, cov pos/vel, var vel: the same for both axes), nis float64 [N]
    (squared innovation over its variance, summed over the axes; 0 at a birth), age int32 [N] (links since birth; -1 beyond a frame's
    count, where the others are zero)."""
    __slots__ = ("pos", "vel", "cov", "nis", "age")

    def __init__(self, pos, vel, cov, nis, age):
        self.pos, self.vel, self.cov, self.nis, self.age = pos, vel, cov, nis, age


def _finite(v):
    return _real(v) and math.isfinite(v)


class TrackSmoother:
    """The filter behind `linker` (the module docstring has the rule).  `smoother(x, tracks, times=None)` takes x, a ClusterSummaries or a
    pipeline.FrameResult, the Tracks `linker(x)` returned for the same x and, behind a timed linker, the `times` given to it for that
    call; returns a Trajectories and advances the state, all on the device: nothing waits for the GPU, every size comes from numbers the
    host knows (node counts, linker.max_gap).  The smoother keeps the node counts (and times) of the frames its state holds, by the
    linker's rule: the last max_gap + 1.  `reset()` drops the state (reset the linker with it).

    process_noise: q, finite and >= 0 (0: a track is a straight line, the filter is recursive least squares).  measurement_noise: r, the
    VARIANCE of a cluster's position per axis, finite and > 0.  vel_var: the velocity variance at birth, finite and > 0 (large: the first
    link sets the velocity).  per_detection: r is the variance of one detection, a cluster of `size` detections has r / size.
    ValueError, on the host before any launch and with the state unmoved: a bad argument, tracks of another length, a frame above 4096
    detections, linker.max_gap changed, the state on another device, a timed state continued untimed or the reverse, times that are not
    one finite number per frame.  CPU tensors: RuntimeError."""

    def __init__(self, linker, process_noise, measurement_noise, vel_var, per_detection=False):
        if not isinstance(linker, FrameLinker):
            raise ValueError("linker must be the FrameLinker whose tracks the smoother will see")
        if not _finite(process_noise) or process_noise < 0:
            raise ValueError(f"process_noise must be a finite number >= 0, not {process_noise!r}")
        if not _finite(measurement_noise) or not measurement_noise > 0:
            raise ValueError(f"measurement_noise must be a finite number > 0, not {measurement_noise!r}")
        if not _finite(vel_var) or not vel_var > 0:
            raise ValueError(f"vel_var must be a finite number > 0, not {vel_var!r}")
        if not isinstance(per_detection, bool):
            raise ValueError(f"per_detection must be a bool, not {per_detection!r}")
        self.linker, self.per_detection = linker, per_detection
        self.process_noise, self.measurement_noise, self.vel_var = float(process_noise), float(measurement_noise), float(vel_var)
        self.max_gap = linker.max_gap   # the state is sized by it: fixed at construction
        self.reset()

    def reset(self):
        """Drop the carried state."""
        self._state, self._frame_rows, self._frame_times, self._state_timed = None, [], [], None

    def _host_times(self, times, g):
        try:
            seq = list(times)
        except TypeError:
            raise ValueError(f"times must be a sequence of {g} numbers, one per frame, not {times!r}") from None
        if len(seq) != g:
            raise ValueError(f"the batch has {g} frames, times has {len(seq)} entries")
        for v in seq:
            if not _finite(v):
                raise ValueError(f"every time must be a finite real number, not {v!r}")
        return [float(v) for v in seq]

    def __call__(self, x, tracks, times=None):
        s = x.identities() if hasattr(x, "identities") else x
        if not isinstance(s, ClusterSummaries):
            raise ValueError("TrackSmoother takes a ClusterSummaries or a FrameResult")
        if not isinstance(tracks, Tracks):
            raise ValueError("TrackSmoother takes the Tracks its linker returned for the same batch")
        if self.linker.max_gap != self.max_gap:
            raise ValueError(f"the linker's max_gap changed from {self.max_gap} to {self.linker.max_gap}: build a new smoother")
        for name, v, low in (("process_noise", self.process_noise, True), ("measurement_noise", self.measurement_noise, False),
                             ("vel_var", self.vel_var, False)):   # (changed after construction)
            if not _finite(v) or v < 0 or (v == 0 and not low):
                raise ValueError(f"{name} must be a finite number {'>= 0' if low else '> 0'}, not {v!r}")
        if not isinstance(self.per_detection, bool):
            raise ValueError(f"per_detection must be a bool, not {self.per_detection!r}")
        ptr = np.asarray(s.node_ptr, dtype=np.int64)
        g, n = len(ptr) - 1, int(s.rank.numel())
        sizes = np.diff(ptr)
        max_n = int(sizes.max()) if g > 0 else 0
        if max_n > MAX_FRAME_NODES:
            raise ValueError(f"a frame has {max_n} detections; TrackSmoother takes frames of at most {MAX_FRAME_NODES}")
        if int(tracks.cluster_track.numel()) != n or int(tracks.matched_prev.numel()) != n:
            raise ValueError(f"tracks has {int(tracks.cluster_track.numel())} rows, the summaries {n}: they are not of the same batch")
        timed = times is not None
        if timed:
            times = self._host_times(times, g)
        if self._state is not None and g > 0 and self._state_timed != timed:
            was, now = ("with", "without") if self._state_timed else ("without", "with")
            raise ValueError(f"the carried state was written {was} time stamps, which a call {now} them cannot continue: reset() it first")
        if not (s.count.is_cuda and tracks.matched_prev.is_cuda):
            raise RuntimeError("gnn_cca_amd.smoothing runs on MI355X only (no CPU fallback)")
        dev = s.count.device
        if self._state is not None and self._state.device != dev:
            raise ValueError(f"the smoother's state is on {self._state.device}, the batch on {dev}: reset() it first")
        lib = nat.lib()
        with _on(dev):
            out = torch.empty(8 * n, dtype=torch.float64, device=dev)   # pos | vel | cov | nis: one allocation, four contiguous views
            pos, vel, cov, nis = out[:2 * n].view(n, 2), out[2 * n:4 * n].view(n, 2), out[4 * n:7 * n].view(n, 3), out[7 * n:]
            age = torch.empty(n, dtype=torch.int32, device=dev)
            if g == 0:   # no time passes: the state stays
                return Trajectories(pos, vel, cov, nis, age)
            in_rows = self._frame_rows
            out_rows = (in_rows + [int(v) for v in sizes])[-(self.max_gap + 1):]
            c_in, c_out = (C.c_int32 * max(len(in_rows), 1))(*in_rows), (C.c_int32 * len(out_rows))(*out_rows)
            state = torch.empty(lib.gnncca_track_smooth_state_bytes(sum(out_rows), len(out_rows)), dtype=torch.uint8, device=dev)
            ws_bytes = lib.gnncca_track_smooth_workspace_bytes(n, g, sum(in_rows))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            times_dev, all_times = None, []
            if timed:   # the times of the carried frames, then the batch's: one non-blocking copy through a fresh pinned buffer
                all_times = self._frame_times + times
                staged = torch.empty(len(all_times), dtype=torch.float64, pin_memory=True)
                staged.copy_(torch.from_numpy(np.asarray(all_times, dtype=np.float64)))
                times_dev = staged.to(dev, non_blocking=True)
            gap = tracks.matched_gap
            st = lib.gnncca_track_smooth(
                s.node_ptr_dev.data_ptr(), s.count.data_ptr(), s.size.data_ptr() if n else None, s.pos.data_ptr() if n else None,
                tracks.matched_prev.data_ptr() if n else None, gap.data_ptr() if n else None, n, g, max_n, self.max_gap, self.process_noise,
                self.measurement_noise, self.vel_var, int(self.per_detection), self._state.data_ptr() if in_rows else None, c_in,
                len(in_rows), state.data_ptr(), c_out, len(out_rows), pos.data_ptr() if n else None, vel.data_ptr() if n else None,
                cov.data_ptr() if n else None, nis.data_ptr() if n else None, age.data_ptr() if n else None, ws.data_ptr(), ws_bytes,
                _raw_stream(dev), times_dev.data_ptr() if timed else None, self.linker.max_dt if timed else 0.0)
            if st:
                nat.check(st, "gnncca_track_smooth")
            # the previous state, the workspace and the times are freed in stream order (allocated on this stream): the launches still read them
        self._state, self._frame_rows, self._state_timed = state, out_rows, timed
        self._frame_times = all_times[-len(out_rows):] if timed else []
        return Trajectories(pos, vel, cov, nis, age)


__all__ = ["Trajectories", "TrackSmoother"]
