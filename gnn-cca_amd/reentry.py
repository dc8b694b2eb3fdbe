"""A returning person gets the old identity back: the re-entry gallery, a second stage behind tracking.FrameLinker, on the GPU and without
a host wait.

    link = FrameLinker(max_step=0.8, max_gap=1)
    gal = TrackGallery(link, max_cos=0.3)          # window=1024, max_batch=2048, max_age=None, max_speed=None
    t = link(r)                                    # Tracks, as ever: a person unseen for more than max_gap frames comes back as a NEW track
    ids = gal(r, t)                                # Identities: cluster_identity [N], node_identity [N], reentered_from [N]
    scorer.add_raw(y, cam, ids.node_identity, r.batch.node_ptr)   # score identities where node_track stood

FrameLinker continues a track across at most max_gap <= 8 missed frames; its design rules a longer gap out (the gate grows with the
gap, the carried state holds max_gap + 1 frames of appearance rows).  The gallery is the usual second stage of a multi-camera tracker:
ended tracks, matched against newly born tracks by appearance.  Track ids stay exactly as the linker gave them; an IDENTITY is the track id
of the first track of a chain of re-entries.  The reference has no counterpart.

The rule (include/gnncca_mpn.h has it step by step, tests/reentry_oracle.py as numpy loops; M = linker.max_gap, W = window,
S = W + max_batch ring slots, f = frames the gallery has seen before this one, over all calls; a BIRTH is a usable cluster with
matched_prev == -1, b its track id).  Per track j, in ring slot j mod S: the running fp32 sum of its clusters' appearance rows, the frame
`last` and position of its latest cluster, its identity and a `continued` flag.  Frames in order:
  1. a cluster the linker continued takes the identity of its predecessor's row (from the batch or from the identities of the last M + 1
     frames, which the gallery carries -- never through the ring, so a track may live longer than S births);
  2. track j is eligible for birth b iff b - W <= j < b and the slot still holds j; j is not continued; f - last[j] >= M + 2 (the linker can
     no longer continue it); f - last[j] <= max_age if given; the distance from the birth to j's last position is <= max_speed * (f - last[j])
     if given; and the cosine distance dcos of the birth's appearance row and sum[j] (fp64; 1 if a norm is 0) is <= max_cos.  cost = dcos;
  3. mutual best among the births of the frame (ties: the smaller track id, the smaller rank): the birth takes j's identity, j is
     continued, reentered_from = j.  Every other birth's identity is its own track id;
  4. a birth takes slot b mod S, whatever it held;  5. every cluster whose track still owns its slot adds its row to the sum and moves
     last / pos.
The rule is causal: the result does not depend on how a sequence is cut into calls.  An eligible track cannot be continued by the linker
any more, so its sum, last and pos are final; the kernels (csrc/identities_reentry.cuh, six launches) accumulate them for the whole call,
compute the births x window cosine table with a tiled fp64 kernel, and one workgroup then walks the frames over table rows only.
Limits: appearance decides -- max_speed is the only use of position; chains are one-to-one, an ended track is continued once; a person
absent while more than W other tracks are born is forgotten; N <= max_batch rows per call; window <= 4096; `tracks` must come from the
linker the gallery was built with, for the same summaries, every batch of the sequence in order.  What it does to IDSW / IDF1 on synthetic
sequences with ground-truth clusters is in DESIGN.md section 9; with a trained model it has not been measured.
No CPU fallback."""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _native as nat
from .frames import _on, _raw_stream
from .tracking import MAX_FRAME_NODES, ClusterSummaries, FrameLinker, Tracks, _real

MAX_WINDOW = nat.REENTRY_MAX_WINDOW


class Identities:
    """What one TrackGallery call returns (device tensors, int64 [N]): cluster_identity (row-aligned with Tracks.cluster_track, -1 beyond a
    frame's count), node_identity (a detection's identity: feed it to TrackScorer.add_raw in place of node_track), reentered_from (the old
    TRACK id a born cluster was attached to, else -1)."""
    __slots__ = ("cluster_identity", "node_identity", "reentered_from")

    def __init__(self, cluster_identity, node_identity, reentered_from):
        self.cluster_identity, self.node_identity, self.reentered_from = cluster_identity, node_identity, reentered_from


def _integer(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


class TrackGallery:
    """The gallery of ended tracks behind `linker` (the module docstring has the rule).  `gal(x, tracks)` takes x, a ClusterSummaries or a
    pipeline.FrameResult, and the Tracks `linker(x)` returned for the same x; returns an Identities and advances the state, all on the
    device: nothing waits for the GPU, every size comes from numbers the host knows (node counts, window, max_batch, linker.max_gap, the
    frames seen so far).  `reset()` forgets everything (reset the linker with it).

    max_cos: the largest admissible cosine distance, in [0, 2].  window: W >= 1 (at most MAX_WINDOW = 4096), how many births back an ended
    track is still looked for.  max_batch: the largest N of a call; the ring has window + max_batch slots of R floats (25 MB at 3072 x 2048),
    updated in place.  max_age: None or an integer >= linker.max_gap + 2, the longest absence in frames.  max_speed: None or a finite
    number > 0, ground-plane units per frame: a birth farther than max_speed * absence from where the track was last seen is not it.
    ValueError, on the host before any launch and with the state unmoved: a bad argument, summaries without appearance columns, N >
    max_batch, a frame above 4096 detections, R differing from the state's, tracks of another length.  CPU tensors: RuntimeError.
    After a call `ring` gives int64 / int32 / fp views of the state (owner, identity, last, pos, continued, sum) for inspection."""

    def __init__(self, linker, max_cos, window=1024, max_batch=2048, max_age=None, max_speed=None):
        if not isinstance(linker, FrameLinker):
            raise ValueError("linker must be the FrameLinker whose tracks the gallery will see")
        if not _real(max_cos) or not 0 <= max_cos <= 2:
            raise ValueError(f"max_cos must be a number in [0, 2], not {max_cos!r}")
        if not _integer(window) or not 1 <= window <= MAX_WINDOW:
            raise ValueError(f"window must be an integer in [1, {MAX_WINDOW}], not {window!r}")
        if not _integer(max_batch) or not 1 <= max_batch < 2 ** 30:
            raise ValueError(f"max_batch must be an integer >= 1, not {max_batch!r}")
        if max_age is not None and (not _integer(max_age) or max_age < linker.max_gap + 2):
            raise ValueError(f"max_age must be None or an integer >= linker.max_gap + 2 = {linker.max_gap + 2}, not {max_age!r}")
        if max_speed is not None and (not _real(max_speed) or not math.isfinite(max_speed) or not max_speed > 0):
            raise ValueError(f"max_speed must be None or a finite number > 0, not {max_speed!r}")
        self.linker, self.max_cos, self.window, self.max_batch = linker, float(max_cos), int(window), int(max_batch)
        self.max_age = None if max_age is None else int(max_age)
        self.max_speed = None if max_speed is None else float(max_speed)
        self.max_gap = linker.max_gap   # the state's history is sized by it: fixed at construction
        self.reset()

    def reset(self):
        """Forget the ring, the identity history and the frame counter."""
        self._ring, self._reid_dim, self._hist, self._frame_rows, self.frames_seen = None, None, None, [], 0

    @property
    def n_slots(self):
        return self.window + self.max_batch

    @property
    def ring(self):
        """Views of the ring state (None before the first call): dict(owner, identity, last int64 [S]; pos fp64 [S, 2]; continued int32 [S];
        sum fp32 [S, R])."""
        if self._ring is None:
            return None
        s, r, buf = self.n_slots, self._reid_dim, self._ring
        i64 = buf[:24 * s].view(torch.int64)
        sum_off = (44 * s + 255) // 256 * 256
        return dict(owner=i64[:s], identity=i64[s:2 * s], last=i64[2 * s:], pos=buf[24 * s:40 * s].view(torch.float64).view(s, 2),
                    continued=buf[40 * s:44 * s].view(torch.int32), sum=buf[sum_off:sum_off + 4 * s * r].view(torch.float32).view(s, r))

    def __call__(self, x, tracks):
        s = x.identities() if hasattr(x, "identities") else x
        if not isinstance(s, ClusterSummaries):
            raise ValueError("TrackGallery takes a ClusterSummaries or a FrameResult")
        if not isinstance(tracks, Tracks):
            raise ValueError("TrackGallery takes the Tracks its linker returned for the same batch")
        if self.linker.max_gap != self.max_gap:
            raise ValueError(f"the linker's max_gap changed from {self.max_gap} to {self.linker.max_gap}: build a new gallery")
        r = int(s.emb.shape[1])
        if r == 0:
            raise ValueError("the summaries have no appearance columns (R == 0): the gallery matches by appearance")
        if self._reid_dim is not None and r != self._reid_dim:
            raise ValueError(f"the summaries carry {r} appearance columns, the gallery's state {self._reid_dim}: reset() it first")
        ptr = np.asarray(s.node_ptr, dtype=np.int64)
        g, n = len(ptr) - 1, int(s.rank.numel())
        sizes = np.diff(ptr)
        max_n = int(sizes.max()) if g > 0 else 0
        if n > self.max_batch:
            raise ValueError(f"the batch has {n} rows, the gallery was built for at most max_batch = {self.max_batch} per call")
        if max_n > MAX_FRAME_NODES:
            raise ValueError(f"a frame has {max_n} detections; TrackGallery takes frames of at most {MAX_FRAME_NODES}")
        if int(tracks.cluster_track.numel()) != n or int(tracks.matched_prev.numel()) != n:
            raise ValueError(f"tracks has {int(tracks.cluster_track.numel())} rows, the summaries {n}: they are not of the same batch")
        if not (s.count.is_cuda and tracks.cluster_track.is_cuda):
            raise RuntimeError("gnn_cca_amd.reentry runs on MI355X only (no CPU fallback)")
        dev = s.count.device
        if self._ring is not None and self._ring.device != dev:
            raise ValueError(f"the gallery's state is on {self._ring.device}, the batch on {dev}: reset() it first")
        lib = nat.lib()
        with _on(dev):
            out = torch.empty((3, n), dtype=torch.int64, device=dev)   # cluster_identity | node_identity | reentered_from
            if g == 0:   # no time passes: the state stays
                return Identities(out[0], out[1], out[2])
            if self._ring is None:
                self._ring = torch.zeros(lib.gnncca_reentry_state_bytes(self.n_slots, r), dtype=torch.uint8, device=dev)
                self._reid_dim = r
                self.ring["owner"].fill_(-1)
            in_rows = self._frame_rows
            out_rows = (in_rows + [int(v) for v in sizes])[-(self.max_gap + 1):]
            c_in, c_out = (C.c_int32 * max(len(in_rows), 1))(*in_rows), (C.c_int32 * len(out_rows))(*out_rows)
            hist = torch.empty(max(sum(out_rows), 1), dtype=torch.int64, device=dev)
            ws_bytes = lib.gnncca_reentry_workspace_bytes(n, self.window, self.max_batch)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            gap = tracks.matched_gap
            st = lib.gnncca_reentry_update(
                s.node_ptr_dev.data_ptr(), s.count.data_ptr(), s.rank.data_ptr() if n else None, s.pos.data_ptr() if n else None,
                s.emb.data_ptr() if n else None, r, n, g, max_n, tracks.cluster_track.data_ptr() if n else None,
                tracks.matched_prev.data_ptr() if n else None, gap.data_ptr() if n else None, self.max_gap, self.max_cos, self.window,
                self.max_batch, int(self.max_age is not None), self.max_age if self.max_age is not None else 0,
                int(self.max_speed is not None), self.max_speed if self.max_speed is not None else 0.0, self.frames_seen,
                self._ring.data_ptr(), self._hist.data_ptr() if in_rows else None, c_in, len(in_rows), hist.data_ptr(), c_out, len(out_rows),
                out[0].data_ptr() if n else None, out[1].data_ptr() if n else None, out[2].data_ptr() if n else None, ws.data_ptr(), ws_bytes,
                _raw_stream(dev))
            if st:
                nat.check(st, "gnncca_reentry_update")
            # the previous history and the workspace are freed in stream order (allocated on this stream): the launches above still read them
        self._hist, self._frame_rows, self.frames_seen = hist, out_rows, self.frames_seen + g
        return Identities(out[0], out[1], out[2])


__all__ = ["MAX_WINDOW", "Identities", "TrackGallery"]
