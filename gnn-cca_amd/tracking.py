"""What a consumer does with the partition of a batch of frames, on the GPU and without a host wait: per-cluster summaries (the fused
ground-plane position, the mean appearance, the size and the number of cameras of every identity cluster) and track ids that persist
over the frames of a batch and from one batch to the next.

    s = cluster_summaries(batch, labels)          # ClusterSummaries: count [G], rank [N], size / n_cams [N], pos [N, 2], emb [N, R]
    s = r.identities()                            # r: a pipeline.FrameResult -- summaries of final()'s labels (final=False: r.labels)
    link = FrameLinker(max_step=0.8, lam=1.0)     # metres a person may move between two frames; weight of the appearance term
    t = link(r)                                   # Tracks: cluster_track [N], node_track [N], matched_prev [N], next_id [1]
    t = link(next_r)                              # ... frame 0 of this batch continues the last frame of the previous one
    link = FrameLinker(max_step=0.8, max_gap=2)   # a track survives up to 2 frames that miss it; t.matched_gap [N]: frames skipped

The reference has NO counterpart: it scores single frames (inference.py:349-371), never fuses the views of a cluster into a position and
never carries an identity from one frame to the next.  What these rules do to tracking quality with a trained model has NOT been measured.

Summaries (csrc/identities.hip, two launches).  `labels` is int32 [N] in the convention of postprocess.prune_and_cluster / finalize: a
node's label is the smallest node id of its cluster.  Nothing is compacted across frames, so every output has a fixed shape: cluster c of
frame g (clusters ordered by ascending root id) is ROW node_ptr[g] + c of size, n_cams, pos and emb; rows at or beyond count[g] are zero.
pos is the sum of xw (yw) over the members in ascending node id, then one division by float64(size); emb the same per column in float32:
the sum orders are part of the contract (tests/tracking_oracle.py restates them as numpy loops and the kernels match it bit for bit).
A frame whose labels point outside it or at a non-root gets count -1 and zero rows; frames above 4096 detections are refused (ValueError).

Linking (three launches).  Frame t is linked to frame t - 1, frame 0 to the state carried from the previous call.  For cluster a of the
current and b of the previous frame:  d = sqrt(dx^2 + dy^2);  dcos = 1 - <ea, eb> / (|ea| |eb|) in float64 (1 if a norm is 0);
cost = d / max_step + lam * dcos;  the pair is admissible iff d <= max_step and (if given) dcos <= max_cos.  fwd[a] is the admissible b of
smallest cost, bwd[b] the admissible a of smallest cost, ties to the smaller index; a continues b iff each is the other's best -- one to
one by construction, and deterministic.  A matched cluster takes its partner's id; the others get next_id, next_id + 1, ... in ascending
(frame, cluster) order.  With lam == 0 and no max_cos the embeddings are not read.
Gaps (max_gap = M > 0: csrc/identities_gap.cuh, M + 4 launches).  Every cluster has a predecessor (none at first) and a has-a-successor
flag (clear at first).  Levels k = 0 .. M run one after the other, all frames of the batch in parallel within a level: the clusters of frame
t WITHOUT a predecessor meet the clusters of frame t - 1 - k (of this batch or of the carried history) WITHOUT a successor, under
gate_k = max_step * (k + 1): admissible iff d <= gate_k (and dcos <= max_cos), cost = d / gate_k + lam * dcos, mutual best as above with
ties to the smaller rank within the frame.  Level 0 is the rule above word for word, so a shorter gap always wins over a longer one, even
at higher cost.  Time is the frame index over all calls since reset(): an empty or refused frame still counts as a frame, an empty batch
passes no time.  The rule is causal, so the ids do not depend on how a sequence is cut into batches; the state holds the last M + 1 frames.
Limits: frames are taken to be CONSECUTIVE and IN ORDER (there are no time stamps); a track unseen for more than max_gap frames ends (with
the default max_gap = 0: in the first frame that misses it); a cluster is looked for where it was last seen -- there is no motion
prediction (no velocity term), only a gate that grows with the gap; the matching is mutual-best, not an optimal assignment.
No CPU fallback."""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _native as nat
from .frames import _on, _raw_stream

MAX_FRAME_NODES = 4096
MAX_GAP = nat.TRACK_MAX_GAP


class ClusterSummaries:
    """Per-cluster rows of a batch (device tensors; cluster c of frame g is row node_ptr[g] + c): count int32 [G] (-1: a refused frame),
    rank int32 [N] (a detection's cluster within its frame), size / n_cams int32 [N], pos float64 [N, 2], emb float32 [N, R]; node_ptr is
    the host list of frame offsets and node_ptr_dev its int32 device copy."""
    __slots__ = ("count", "rank", "size", "n_cams", "pos", "emb", "node_ptr", "node_ptr_dev")

    def __init__(self, count, rank, size, n_cams, pos, emb, node_ptr, node_ptr_dev):
        self.count, self.rank, self.size, self.n_cams, self.pos, self.emb = count, rank, size, n_cams, pos, emb
        self.node_ptr, self.node_ptr_dev = node_ptr, node_ptr_dev


class Tracks:
    """Track ids of a batch (device tensors): cluster_track int64 [N] (row-aligned with the summaries, -1 beyond a frame's count),
    node_track int64 [N] (a detection's track), matched_prev int32 [N] (the rank of the cluster's predecessor in ITS OWN frame, or -1),
    matched_gap int32 [N] (-1: no predecessor; k: the predecessor is k + 1 frames back, k frames were skipped -- all 0 / -1 from a linker
    without max_gap, where it is derived from matched_prev when first read), next_id int64 [1] (the first id nobody has yet)."""
    __slots__ = ("cluster_track", "node_track", "matched_prev", "next_id", "_state", "_matched_gap")

    def __init__(self, cluster_track, node_track, matched_prev, next_id, state, matched_gap=None):
        self.cluster_track, self.node_track, self.matched_prev, self.next_id, self._state = cluster_track, node_track, matched_prev, next_id, state
        self._matched_gap = matched_gap

    @property
    def matched_gap(self):
        if self._matched_gap is None:   # the max_gap = 0 path launches nothing for it unless somebody asks: -1 stays, a rank becomes 0
            self._matched_gap = torch.clamp(self.matched_prev, max=0)
        return self._matched_gap


def _host_ptr(node_ptr):
    ptr = np.asarray(node_ptr, dtype=np.int64).reshape(-1)
    if len(ptr) < 1:
        raise ValueError("node_ptr needs at least one entry")
    return ptr


def _summaries(labels, ptr, node_ptr_dev, xw, yw, cam, embeds):
    g = len(ptr) - 1
    n = int(labels.numel())
    max_n = int(np.diff(ptr).max()) if g > 0 else 0
    if max_n > MAX_FRAME_NODES:
        raise ValueError(f"a frame has {max_n} detections; cluster_summaries takes frames of at most {MAX_FRAME_NODES}")
    if not labels.is_cuda:
        raise RuntimeError("gnn_cca_amd.tracking runs on MI355X only (no CPU fallback)")
    if xw.numel() != n or yw.numel() != n or cam.numel() != n or (g > 0 and int(ptr[-1]) != n):
        raise ValueError(f"labels [{n}], xw [{xw.numel()}], yw [{yw.numel()}], cam [{cam.numel()}] and node_ptr (N={int(ptr[-1])}) disagree")
    r = 0
    if embeds is not None:
        if embeds.dim() != 2 or embeds.shape[0] != n:
            raise ValueError(f"embeds must be [N, R] with N={n}, not {tuple(embeds.shape)}")
        r = int(embeds.shape[1])
    dev = labels.device
    lib = nat.lib()
    with _on(dev):
        lb = labels.to(torch.int32).contiguous()
        nptr = node_ptr_dev.to(device=dev, dtype=torch.int32).contiguous()
        x64, y64 = xw.to(device=dev, dtype=torch.float64).contiguous(), yw.to(device=dev, dtype=torch.float64).contiguous()
        cm = cam.to(device=dev, dtype=torch.int32).contiguous()
        em = embeds.detach().to(device=dev, dtype=torch.float32).contiguous() if r else None
        count = torch.empty(g, dtype=torch.int32, device=dev)
        ints = torch.empty((3, n), dtype=torch.int32, device=dev)   # rank | size | n_cams
        pos = torch.empty((n, 2), dtype=torch.float64, device=dev)
        emb = torch.empty((n, r), dtype=torch.float32, device=dev)
        ws_bytes = lib.gnncca_cluster_summaries_bytes(n, g)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = lib.gnncca_cluster_summaries(lb.data_ptr() if n else None, nptr.data_ptr(), x64.data_ptr() if n else None,
                                          y64.data_ptr() if n else None, cm.data_ptr() if n else None, em.data_ptr() if r and n else None, r,
                                          n, g, max_n, count.data_ptr() if g else None, ints[0].data_ptr() if n else None,
                                          ints[1].data_ptr() if n else None, ints[2].data_ptr() if n else None, pos.data_ptr() if n else None,
                                          emb.data_ptr() if r and n else None, ws.data_ptr(), ws_bytes, _raw_stream(dev))
        if st:
            nat.check(st, "gnncca_cluster_summaries")
        # the workspace is freed by the caching allocator in stream order (it was allocated on this stream): nothing to keep
    return ClusterSummaries(count, ints[0], ints[1], ints[2], pos, emb, ptr.tolist(), nptr)


def cluster_summaries_raw(labels, node_ptr, xw, yw, cam, embeds=None):
    """Summaries from plain device tensors: labels int32 [N], xw / yw float64 [N], cam int32 [N], embeds float32 [N, R] or None (R = 0).
    node_ptr: the G + 1 frame offsets as a HOST sequence (uploaded here) or a tensor (then read back once: its largest frame has to be
    known before anything is launched).  Enqueued on the current stream -> ClusterSummaries."""
    if isinstance(node_ptr, torch.Tensor):
        ptr, dev_ptr = _host_ptr(node_ptr.cpu().numpy()), node_ptr
    else:
        ptr = _host_ptr(node_ptr)
        dev_ptr = None
    if len(ptr) > 1 and int(np.diff(ptr).max()) > MAX_FRAME_NODES:   # before the GPU is touched
        raise ValueError(f"a frame has {int(np.diff(ptr).max())} detections; cluster_summaries takes frames of at most {MAX_FRAME_NODES}")
    if dev_ptr is None:
        dev_ptr = torch.from_numpy(ptr.astype(np.int32))
    return _summaries(labels, ptr, dev_ptr, xw, yw, cam, embeds)


def cluster_summaries(batch, labels, embeds=None):
    """Summaries of `labels` (int32 [N] on the device) over the frames of `batch`, a GraphBatch of graph_build.build_graph_batch or
    pipeline.FramePipeline: xw, yw and cam are read from the batch's staging image on the device (which is not modified), the frame
    offsets from batch.node_ptr / node_ptr_dev; `embeds` defaults to batch.reid_embeds (the normalised appearance rows).  Enqueued on the
    current stream, no synchronisation -> ClusterSummaries.  Frames above 4096 detections: ValueError."""
    frames = getattr(batch, "_frames", None)
    if frames is None:
        raise ValueError("cluster_summaries needs a batch of build_graph_batch / FramePipeline (its staging image holds xw, yw and cam); "
                         "use cluster_summaries_raw for plain tensors")
    image, layout = frames
    if embeds is None:
        embeds = batch.reid_embeds
    return _summaries(labels, _host_ptr(batch.node_ptr), batch.node_ptr_dev, layout.view(image, "xw"), layout.view(image, "yw"),
                      layout.view(image, "cam"), embeds)


class FrameLinker:
    """Persistent track ids for the clusters of consecutive frames (the module docstring has the rule).  `linker(x)` links the frames of
    one batch -- x a ClusterSummaries, or a pipeline.FrameResult (its identities()) -- to each other and frame 0 to the last frame of
    the previous call, returns a Tracks and advances the state, all on the device: nothing waits for the GPU (the state is sized by the
    last frame's node count, which bounds its cluster count and is known on the host).  `reset()` forgets the state: ids start at 0 again.

    max_step: the largest ground-plane distance (the units of xw / yw) a cluster may move between two frames, finite and > 0.
    lam: the weight of the cosine distance of the mean appearances in the cost, finite and >= 0 (0 with max_cos=None: position only, the
    embeddings are not read).  max_cos: None, or the largest admissible cosine distance, in [0, 2].
    max_gap: an integer in 0 .. 8, the number of consecutive frames a track may be missing from and still be continued (gate
    max_step * (k + 1) after k missed frames; a shorter gap always wins).  0: the adjacent-frame linker, three launches, as ever; M > 0:
    M + 4 launches, and the state holds the last M + 1 frames (sized from their node counts, which the linker keeps on the host).
    Frames are taken to be consecutive and in order (no time stamps); a track missing from more than max_gap frames ends; there is no
    motion prediction (no velocity term) and the matching is mutual-best, not an optimal assignment.  No counterpart in the reference; the
    effect on tracking quality with a trained model has not been measured."""

    def __init__(self, max_step, lam=1.0, max_cos=None, max_gap=0):
        def real(v):
            return isinstance(v, numbers.Real) and not isinstance(v, bool)
        if not real(max_step) or not math.isfinite(max_step) or not max_step > 0:
            raise ValueError(f"max_step must be a finite number > 0, not {max_step!r}")
        if not real(lam) or not math.isfinite(lam) or lam < 0:
            raise ValueError(f"lam must be a finite number >= 0, not {lam!r}")
        if max_cos is not None and (not real(max_cos) or not 0 <= max_cos <= 2):
            raise ValueError(f"max_cos must be None or a number in [0, 2], not {max_cos!r}")
        if isinstance(max_gap, bool) or not isinstance(max_gap, numbers.Integral) or not 0 <= max_gap <= MAX_GAP:
            raise ValueError(f"max_gap must be an integer in [0, {MAX_GAP}], not {max_gap!r}")
        self.max_step, self.lam, self.max_cos = float(max_step), float(lam), None if max_cos is None else float(max_cos)
        self.max_gap = int(max_gap)
        self.reset()

    def reset(self):
        """Forget the carried frames and the id counter."""
        self._state, self._cap, self._reid_dim = None, 0, None
        self._frame_rows = []   # max_gap > 0: the node counts of the frames the state holds, oldest first (they bound the cluster counts)

    @property
    def needs_embeddings(self):
        return self.lam != 0.0 or self.max_cos is not None

    def __call__(self, x):
        s = x.identities() if hasattr(x, "identities") else x
        if not isinstance(s, ClusterSummaries):
            raise ValueError("FrameLinker takes a ClusterSummaries or a FrameResult")
        r_all = int(s.emb.shape[1])
        if self._reid_dim is not None and r_all != self._reid_dim:
            raise ValueError(f"the summaries carry {r_all} appearance columns, the linker's state {self._reid_dim}: reset() it first")
        ptr = np.asarray(s.node_ptr, dtype=np.int64)
        g, n = len(ptr) - 1, int(s.rank.numel())
        sizes = np.diff(ptr)
        max_n = int(sizes.max()) if g > 0 else 0
        if max_n > MAX_FRAME_NODES:
            raise ValueError(f"a frame has {max_n} detections; FrameLinker takes frames of at most {MAX_FRAME_NODES}")
        dev = s.count.device
        self._reid_dim = r_all
        r = r_all if self.needs_embeddings else 0
        lib = nat.lib()
        with _on(dev):
            if g == 0:   # nothing to link: the state stays
                nid = self._state[:8].view(torch.int64) if self._state is not None else torch.zeros(1, dtype=torch.int64, device=dev)
                e64, e32 = torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
                return Tracks(e64, e64.clone(), e32, nid, self._state, e32.clone())
            if self.max_gap > 0:
                return self._link_gap(lib, s, dev, sizes, g, n, max_n, r)
            cap = int(sizes[-1])
            state = torch.empty(lib.gnncca_link_state_bytes(cap, r), dtype=torch.uint8, device=dev)
            tracks = torch.empty((2, n), dtype=torch.int64, device=dev)   # cluster_track | node_track
            matched = torch.empty(n, dtype=torch.int32, device=dev)
            ws_bytes = lib.gnncca_link_workspace_bytes(n, g)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            st = lib.gnncca_link_frames(s.node_ptr_dev.data_ptr(), s.count.data_ptr(), s.rank.data_ptr() if n else None,
                                        s.pos.data_ptr() if n else None, s.emb.data_ptr() if r and n else None, r, n, g, max_n, self.max_step,
                                        self.lam, int(self.max_cos is not None), self.max_cos if self.max_cos is not None else 0.0,
                                        self._state.data_ptr() if self._state is not None else None, self._cap, state.data_ptr(), cap,
                                        tracks[0].data_ptr() if n else None, tracks[1].data_ptr() if n else None,
                                        matched.data_ptr() if n else None, ws.data_ptr(), ws_bytes, _raw_stream(dev))
            if st:
                nat.check(st, "gnncca_link_frames")
            # the previous state and the workspace are freed in stream order (allocated on this stream): the launches above still read them
        self._state, self._cap = state, cap
        return Tracks(tracks[0], tracks[1], matched, state[:8].view(torch.int64), state)

    def _link_gap(self, lib, s, dev, sizes, g, n, max_n, r):
        """The max_gap > 0 call (inside _on(dev), g > 0): everything is sized from host-known node counts, nothing waits for the GPU."""
        in_rows = self._frame_rows
        out_rows = (in_rows + [int(v) for v in sizes])[-(self.max_gap + 1):]
        c_in, c_out = (C.c_int32 * max(len(in_rows), 1))(*in_rows), (C.c_int32 * len(out_rows))(*out_rows)
        state = torch.empty(lib.gnncca_link_gap_state_bytes(sum(out_rows), len(out_rows), r), dtype=torch.uint8, device=dev)
        tracks = torch.empty((2, n), dtype=torch.int64, device=dev)   # cluster_track | node_track
        matched = torch.empty((2, n), dtype=torch.int32, device=dev)   # matched_prev | matched_gap
        ws_bytes = lib.gnncca_link_gap_workspace_bytes(n, g, sum(in_rows))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = lib.gnncca_link_frames_gap(s.node_ptr_dev.data_ptr(), s.count.data_ptr(), s.rank.data_ptr() if n else None,
                                        s.pos.data_ptr() if n else None, s.emb.data_ptr() if r and n else None, r, n, g, max_n, self.max_step,
                                        self.lam, int(self.max_cos is not None), self.max_cos if self.max_cos is not None else 0.0,
                                        self.max_gap, self._state.data_ptr() if in_rows else None, c_in, len(in_rows), state.data_ptr(), c_out,
                                        len(out_rows), tracks[0].data_ptr() if n else None, tracks[1].data_ptr() if n else None,
                                        matched[0].data_ptr() if n else None, matched[1].data_ptr() if n else None, ws.data_ptr(), ws_bytes,
                                        _raw_stream(dev))
        if st:
            nat.check(st, "gnncca_link_frames_gap")
        # the previous state and the workspace are freed in stream order (allocated on this stream): the launches above still read them
        self._state, self._frame_rows = state, out_rows
        return Tracks(tracks[0], tracks[1], matched[0], state[:8].view(torch.int64), state, matched[1])


__all__ = ["MAX_FRAME_NODES", "MAX_GAP", "ClusterSummaries", "Tracks", "cluster_summaries", "cluster_summaries_raw", "FrameLinker"]
