"""Linking by the filtered state: tracking.FrameLinker whose motion model is the constant-velocity Kalman filter of smoothing.TrackSmoother,
run INSIDE the linker, on the GPU and without a host wait.

    link = KalmanLinker(max_step=0.4, process_noise=0.001, measurement_noise=0.01, vel_var=0.25, lam=0.0, max_gap=2)
    t = link(r)                                    # KalmanTracks: a Tracks (velocity: the FILTERED velocity) with t.trajectories
    t.trajectories                                 # smoothing.Trajectories: pos / vel [N, 2], cov [N, 3], nis [N], age [N]
    link = KalmanLinker(1.4, 0.001, 0.01, 0.25, max_nis=13.8)   # also gate by the variance of the prediction: a wide max_step, a chi-square bound
    t = link(r, times=[0.0, 1.0, 3.0, 4.1])        # time stamps, as with every linker

FrameLinker(motion='velocity') predicts from one subtraction and one division of two raw fused positions, starts its prediction at the raw
last position, and its gate max_step * dt is the same for a track born a frame ago and one followed for fifty.  TrackSmoother filters, but
behind the linker: it gates nothing.  This linker looks for a track where its filtered state predicts it, feeds every link to the filter,
and with max_nis gates a pair by the variance of that prediction: a newborn track, whose velocity is unknown (variance vel_var), is looked
for widely, an established one narrowly -- which no single max_step can do.  The reference has no counterpart.

The rule (include/gnncca_mpn.h has it word for word, tests/tracking_kalman_oracle.py as numpy loops).  Frames outside, levels 0 .. max_gap
inside, as in the motion walk; dt = float64(k + 1), with time stamps T[t] - T[t - 1 - k] (a table with dt outside (0, max_dt] is skipped
whole).  Every cluster carries a filtered state x = (px, py, vx, vy, a, b, c) and an age.  At level k the clusters b of frame t - 1 - k
without a successor stand at pred(b) = p(b) + dt * v(b) (filtered values; one multiplication, one addition); the pair rule is the shared
one between the RAW pos(a) and pred(b): d = sqrt(dx*dx + dy*dy), gate max_step * dt, the cosine term and max_cos unchanged,
cost = d / gate + lam * dcos.  With max_nis a pair is admissible only if also (dx*dx + dy*dy) / s <= max_nis, s = a_ + r,
a_ = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0: the smoother's operations in its order, no FMA; a NaN is admissible with nobody.  Mutual
best, ties to the smaller index, a shorter gap wins.  On commit x(a), nis(a), age(a) = step(x(b), age(b), z = pos(a), dt, q, r), the
smoother's link rule verbatim; a cluster without a predecessor starts as (z, 0, 0, r, 0, vel_var), age 0, nis 0.  Ids as ever.
Consequences: the result does not depend on how a sequence is cut into calls; and TrackSmoother(linker, q, r, vel_var)(x, tracks, times)
returns exactly tracks.trajectories.
Kernels (csrc/identities_kalman.cuh): three launches whatever max_gap is -- a clear, ONE workgroup that walks the frames in order, a
frame-parallel finish.  The state is a history state of its own kind (filtered pos and vel, cov, age).  Nothing is read back.
Limits: constant velocity and one (q, r) for all tracks; no per_detection (re = r); mutual best only (no matching='optimal'); a track that
reentry.TrackGallery re-attaches starts a fresh filter.  DESIGN.md section 9 has what it does to identity switches on synthetic crossing
walks with ground-truth clusters and the call times; with a trained model it has not been measured.
No CPU fallback."""
import ctypes as C
import math

import torch

from . import _native as nat
from .frames import _raw_stream
from .smoothing import Trajectories
from .tracking import FrameLinker, Tracks, _real


class KalmanTracks(Tracks):
    """The Tracks of a KalmanLinker: `velocity` float64 [N, 2] is the FILTERED velocity, and `trajectories` a smoothing.Trajectories,
    row-aligned with cluster_track -- pos, vel float64 [N, 2], cov float64 [N, 3], nis float64 [N], age int32 [N]; rows at or beyond a
    frame's count are zero with age -1.  trajectories.vel and velocity are the same tensor."""
    __slots__ = ("trajectories",)

    def __init__(self, cluster_track, node_track, matched_prev, next_id, state, matched_gap, trajectories):
        super().__init__(cluster_track, node_track, matched_prev, next_id, state, matched_gap, trajectories.vel)
        self.trajectories = trajectories


def _finite(v):
    return _real(v) and math.isfinite(v)


def _empty_trajectories(n, dev):
    out = torch.empty(8 * n, dtype=torch.float64, device=dev)   # pos | vel | cov | nis: one allocation, four contiguous views
    return Trajectories(out[:2 * n].view(n, 2), out[2 * n:4 * n].view(n, 2), out[4 * n:7 * n].view(n, 3), out[7 * n:],
                        torch.empty(n, dtype=torch.int32, device=dev))


class KalmanLinker(FrameLinker):
    """A FrameLinker (TrackGallery, TrackSmoother and TrackScorer take it and its tracks) that links by the filtered state (the module
    docstring has the rule).  `linker(x, times=None)` returns a KalmanTracks and advances the state; `reset()` forgets it; the state
    carried across calls, empty batches and time stamps work as in every history linker.

    max_step, lam, max_cos, max_gap, max_dt: FrameLinker's (max_step bounds the deviation from the PREDICTED position per frame period).
    process_noise: q, finite and >= 0.  measurement_noise: r, the variance of a cluster's position per axis, finite and > 0.  vel_var: the
    velocity variance at birth, finite and > 0.  max_nis: None (no variance gate) or a finite number > 0, the largest squared innovation
    over its predicted variance a link may have -- chi-square with two degrees of freedom if q and r are right (13.8: one in a thousand).
    matching is always 'mutual' and motion reads 'kalman'.  ValueError, on the host before any launch and with the state unmoved: a bad
    argument, a frame above 4096 detections, a state of another kind or reid width, a timed state continued untimed or the reverse, bad
    times."""

    def __init__(self, max_step, process_noise, measurement_noise, vel_var, lam=1.0, max_cos=None, max_gap=0, max_nis=None, max_dt=None):
        if not _finite(process_noise) or process_noise < 0:
            raise ValueError(f"process_noise must be a finite number >= 0, not {process_noise!r}")
        if not _finite(measurement_noise) or not measurement_noise > 0:
            raise ValueError(f"measurement_noise must be a finite number > 0, not {measurement_noise!r}")
        if not _finite(vel_var) or not vel_var > 0:
            raise ValueError(f"vel_var must be a finite number > 0, not {vel_var!r}")
        if max_nis is not None and (not _finite(max_nis) or not max_nis > 0):
            raise ValueError(f"max_nis must be None or a finite number > 0, not {max_nis!r}")
        super().__init__(max_step, lam=lam, max_cos=max_cos, max_gap=max_gap, max_dt=max_dt)
        self.process_noise, self.measurement_noise, self.vel_var = float(process_noise), float(measurement_noise), float(vel_var)
        self.max_nis = None if max_nis is None else float(max_nis)
        self.motion = "kalman"   # (a mode of this class: not one of nat.MOTION, which FrameLinker's own entries take)

    def _check_mode(self):
        if self.motion != "kalman" or self.matching != "mutual":   # (changed after construction)
            raise ValueError(f"motion={self.motion!r} with matching={self.matching!r} is not a linker KalmanLinker is: it links with "
                             "motion='kalman', matching='mutual'")
        for name, v, low in (("process_noise", self.process_noise, True), ("measurement_noise", self.measurement_noise, False),
                             ("vel_var", self.vel_var, False)):
            if not _finite(v) or v < 0 or (v == 0 and not low):
                raise ValueError(f"{name} must be a finite number {'>= 0' if low else '> 0'}, not {v!r}")
        if self.max_nis is not None and (not _finite(self.max_nis) or not self.max_nis > 0):
            raise ValueError(f"max_nis must be None or a finite number > 0, not {self.max_nis!r}")

    def _no_frames(self, dev):
        t = super()._no_frames(dev)
        return KalmanTracks(t.cluster_track, t.node_track, t.matched_prev, t.next_id, self._state, t.matched_gap, _empty_trajectories(0, dev))

    def _link_history(self, lib, s, dev, sizes, g, n, max_n, r, times=None):
        """FrameLinker._link_history for this class's entry (inside _on(dev), g > 0): everything is sized from host-known node counts,
        nothing waits for the GPU."""
        in_rows = self._frame_rows
        out_rows = (in_rows + [int(v) for v in sizes])[-(self.max_gap + 1):]
        c_in, c_out = (C.c_int32 * max(len(in_rows), 1))(*in_rows), (C.c_int32 * len(out_rows))(*out_rows)
        state = torch.empty(lib.gnncca_link_kalman_state_bytes(sum(out_rows), len(out_rows), r), dtype=torch.uint8, device=dev)
        tracks = torch.empty((2, n), dtype=torch.int64, device=dev)    # cluster_track | node_track
        matched = torch.empty((2, n), dtype=torch.int32, device=dev)   # matched_prev | matched_gap
        tr = _empty_trajectories(n, dev)
        ws_bytes = lib.gnncca_link_kalman_workspace_bytes(n, g, sum(in_rows))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        all_times, times_dev = (None, None) if times is None else self._stage_times(times, dev)
        ptr = lambda t: t.data_ptr() if n else None
        st = lib.gnncca_link_frames_kalman(
            s.node_ptr_dev.data_ptr(), s.count.data_ptr(), ptr(s.rank), ptr(s.pos), s.emb.data_ptr() if r and n else None, r, n, g, max_n,
            self.max_step, self.lam, int(self.max_cos is not None), self.max_cos if self.max_cos is not None else 0.0, self.max_gap,
            self.process_noise, self.measurement_noise, self.vel_var, int(self.max_nis is not None),
            self.max_nis if self.max_nis is not None else 0.0, self._state.data_ptr() if in_rows else None, c_in, len(in_rows),
            state.data_ptr(), c_out, len(out_rows), ptr(tracks[0]), ptr(tracks[1]), ptr(matched[0]), ptr(matched[1]), ptr(tr.pos), ptr(tr.vel),
            ptr(tr.cov), ptr(tr.nis), ptr(tr.age), ws.data_ptr(), ws_bytes, _raw_stream(dev),
            times_dev.data_ptr() if times is not None else None, self.max_dt if times is not None else 0.0)
        if st:
            nat.check(st, "gnncca_link_frames_kalman")
        # the previous state, the workspace and the times are freed in stream order (allocated on this stream): the launches still read them
        self._advance(state, out_rows, all_times)
        return KalmanTracks(tracks[0], tracks[1], matched[0], state[:8].view(torch.int64), state, matched[1], tr)


__all__ = ["KalmanLinker", "KalmanTracks"]
