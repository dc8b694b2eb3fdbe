"""What a consumer does with the partition of a batch of frames, on the GPU and without a host wait: per-cluster summaries (the fused
ground-plane position, the mean appearance, the size and the number of cameras of every identity cluster) and track ids that persist
over the frames of a batch and from one batch to the next.

    s = cluster_summaries(batch, labels)          # ClusterSummaries: count [G], rank [N], size / n_cams [N], pos [N, 2], emb [N, R]
    s = r.identities()                            # r: a pipeline.FrameResult -- summaries of final()'s labels (final=False: r.labels)
    link = FrameLinker(max_step=0.8, lam=1.0)     # metres a person may move between two frames; weight of the appearance term
    t = link(r)                                   # Tracks: cluster_track [N], node_track [N], matched_prev [N], next_id [1]
    t = link(next_r)                              # ... frame 0 of this batch continues the last frame of the previous one
    link = FrameLinker(max_step=0.8, max_gap=2)   # a track survives up to 2 frames that miss it; t.matched_gap [N]: frames skipped
    link = FrameLinker(max_step=0.8, matching='optimal')   # per frame pair the min-cost assignment instead of mutual best
    link = FrameLinker(max_step=0.4, max_gap=2, motion='velocity')   # look for a track where it is heading; t.velocity [N, 2]
    t = link(r, times=[0.0, 1.0, 3.0, 4.1])       # any mode: one time per frame, in frame periods -- a dropped frame is a gap (max_dt)
    score = TrackScorer(max_ids=1024, max_cams=8) # identity-tracking scores against the caller's person ids, accumulated on the device
    score.add(r, t).switched                      # int32 [N]: -1 not scored, 0, 1 = this detection is an identity switch
    score.result()                                # IDSW, IDTP, IDF1, AssA, purity, coverage, MT / PT / ML ...: ONE synchronisation

The reference has NO counterpart: it scores single frames (inference.py:349-371), never fuses the views of a cluster into a position and
never carries an identity from one frame to the next.  What these rules do to tracking quality CAN now be measured wherever ground-truth
person ids exist (TrackScorer; DESIGN.md section 9 has a table on synthetic sequences with ground-truth clusters); with a trained model it
still has NOT been measured.

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
Limits: without time stamps (below) frames are taken to be CONSECUTIVE and IN ORDER; a track unseen for more than max_gap frames ends (with
the default max_gap = 0: in the first frame that misses it); a cluster is looked for where it was last seen -- there is no motion
prediction (no velocity term), only a gate that grows with the gap -- unless motion='velocity' is asked for:
Motion (motion='velocity': csrc/identities_motion.cuh, THREE launches whatever max_gap is).  The levels, gates, masks, cost, mutual best,
ties and id numbering are those of the gap rule, and two things are added.  Every cluster has a velocity, float64 [2] in ground-plane
units per frame: (0, 0) without a predecessor; when cluster a of frame t is linked at level k to cluster b of frame t - 1 - k,
vel(a) = (pos(a) - pos(b)) / float64(k + 1) per component -- one subtraction, one division, no smoothing.  And at level k cluster b is
looked for at pred(b) = pos(b) + float64(k + 1) * vel(b) (one multiplication, one addition, no FMA): d is the distance from pos(a) to
pred(b), admissible iff d <= gate_k = max_step * (k + 1), cost = d / gate_k + lam * dcos -- so max_step becomes the largest DEVIATION from
the predicted position per frame, and may be smaller than the distance a person walks in one.  A non-finite prediction is admissible with
nobody.  vel(b) is known only when b's frame has been through all its levels, so the frames go in order and the levels inside each frame
(for zero velocities that order gives the gap rule's result): one workgroup walks the batch, and hands out the ids as it goes.  The rule
is causal (the carried state holds the velocities of its M + 1 frames; it is a state of its own kind).  Tracks.velocity is float64 [N, 2].
Limits: constant velocity from the LAST link only -- the prediction is wrong after a sharp turn, so a track can end there and restart;
matching='optimal' has no motion yet (the combination is refused).  DESIGN.md section 9 has what it does to identity switches on synthetic crossing walks.
kalman.KalmanLinker, a subclass with a mode of its own, predicts with a constant-velocity Kalman filter instead and can gate by its variance.
Optimal matching (matching='optimal': csrc/identities_assign.cuh, the same M + 4 launches, also with max_gap = 0).  Mutual best leaves a
cluster unlinked whenever its best partner prefers somebody else, even when a second admissible partner is free.  In this mode the levels,
gates, masks and cost stay as above and only the choice of pairs inside a (level, frame pair) table changes: with A the clusters of frame t
without a predecessor and B those of frame t - 1 - k without a successor, both in ascending rank, w = cost - miss_cost for every admissible
pair whose cost is not NaN, the one-to-one set of pairs that minimises the sum of w is linked, where leaving a pair's clusters unlinked is
worth 0 -- so a pair dearer than miss_cost is never taken.  miss_cost defaults to 1 + lam * (max_cos if given, else 2), the dearest an
admissible pair can be.  The optimum's total is unique, its pairs need not be, so the algorithm is the contract: shortest augmenting
paths, rows inserted in ascending rank, ties to the smaller column (include/gnncca_mpn.h has it step by step, tests/tracking_assign_oracle.py
as loops, and the kernel equals them bit for bit).  The table of a frame pair lives in LDS, so such a linker takes frames of at most
MAX_OPTIMAL_FRAME_NODES = 128 detections (ValueError before any launch, for a frame of the batch or of the carried history).  The
assignment is optimal per (level, frame pair), NOT over time: a shorter gap still wins over a longer one at any cost, this mode has no
motion prediction (motion='velocity' above is mutual best only).
Time stamps (linker(x, times=...), every mode: gnncca_link_frames_gap_timed / gnncca_link_frames_motion_timed, the kernels and launches of
the mode).  A timed call gives one fp64 time per frame of the batch, in units of the nominal frame period: finite, strictly increasing,
the first strictly greater than the last time of the previous call.  T[f] is the time of frame f over the combined list (the carried
history, then the batch).  Level order: for frame t at level k the other frame is still s = t - 1 - k, counted in frames PRESENT; a
shorter gap still wins, and the history still holds the last max_gap + 1 frames.  Elapsed time: dt = T[t] - T[s], one fp64 subtraction,
replaces float64(k + 1) everywhere: gate = max_step * dt; with motion pred(b) = pos(b) + dt * vel(b) and vel(a) = (pos(a) - pos(b)) / dt
-- each one operation, in the order of the untimed code, no FMA.  Skipped tables: a table with not (dt > 0 and dt <= max_dt) has no
admissible pair and is skipped whole (which also makes a bad device array harmless); max_dt defaults to max_gap + 1, so a hole of one
frame period consumes one unit of max_gap.  Everything else is the mode's own rule, unchanged: masks, the cosine term, max_cos,
cost = d / gate + lam * dcos, ties, mutual best or the assignment with miss_cost, the numbering of fresh ids, and matched_gap (still the
level k).  Consequence: with T = 0, 1, 2, ... continuing across calls dt is exactly k + 1 and every output equals the untimed linker's bit
for bit.  The times are checked on the host before any launch; the linker keeps the times of the frames its state holds on the host and
sends the combined array through a fresh pinned buffer with one non-blocking copy on the current stream: still no wait for the GPU.  A
timed linker with matching='mutual', max_gap=0, motion='none' runs the gap path with M = 0.  A state written with time stamps is not
continued without them, nor the reverse (ValueError: reset() it first).  Limit: levels count frames present, so max_gap also bounds how
many PRESENT frames a track may skip.
Scores (csrc/track_score.cuh; per call one memset and two launches).  TrackScorer joins ids (batch.y), cam and Tracks.node_track over time.
Detection i is VALID iff 0 <= ids[i] < max_ids, 0 <= cam[i] < max_cams and 0 <= node_track[i] < 2**40; it is SCORED iff it is valid and no
valid detection j > i of its frame has the same (id, cam) (the largest node id wins a duplicate); every other detection is IGNORED (a
negative id says "no ground truth"; the -1 tracks of a refused frame are not scored).  A stream is a (person, camera) pair -- the
per-camera trajectories of the reference's gt.txt files.  A scored detection with track t is a SWITCH iff the latest earlier scored
detection of its stream, however many frames or calls back, had another track; IDSW counts them.  n[p][t] counts the scored detections of
person p (over all cameras) with track t; result() derives IDTP / IDF1, AssA, purity, coverage and MT / PT / ML from it on the host, in a
fixed order (tests/track_score_oracle.py restates all of it as loops and the device path equals it exactly).  The rule is causal: the
scores do not depend on how a sequence is cut into calls.
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
MAX_OPTIMAL_FRAME_NODES = nat.TRACK_MAX_OPTIMAL_FRAME_NODES


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
    without max_gap, where it is derived from matched_prev when first read), next_id int64 [1] (the first id nobody has yet), velocity
    float64 [N, 2] (row-aligned with cluster_track: the displacement per frame since the predecessor, zero without one and beyond a
    frame's count) from a linker with motion='velocity', None from any other."""
    __slots__ = ("cluster_track", "node_track", "matched_prev", "next_id", "velocity", "_state", "_matched_gap")

    def __init__(self, cluster_track, node_track, matched_prev, next_id, state, matched_gap=None, velocity=None):
        self.cluster_track, self.node_track, self.matched_prev, self.next_id, self._state = cluster_track, node_track, matched_prev, next_id, state
        self._matched_gap, self.velocity = matched_gap, velocity

    @property
    def matched_gap(self):
        if self._matched_gap is None:   # the max_gap = 0 path launches nothing for it unless somebody asks: -1 stays, a rank becomes 0
            self._matched_gap = torch.clamp(self.matched_prev, max=0)
        return self._matched_gap


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


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
    matching: 'mutual' (each of a pair is the other's best: the code paths above, untouched) or 'optimal' (per level and frame pair the
    min-cost assignment, where staying unlinked costs miss_cost: always the gap path, M + 4 launches also with max_gap = 0, and frames of
    at most MAX_OPTIMAL_FRAME_NODES = 128 detections).  miss_cost: None (1 + lam * (max_cos, or 2 without one): the dearest an admissible
    pair can be) or a finite number > 0; a pair dearer than it is never linked.  Only with matching='optimal'.
    motion: 'none' (a cluster is looked for where it was last seen: the code paths above, untouched) or 'velocity' (it is looked for at
    its last position plus its last displacement per frame times the frames gone by, and max_step bounds the deviation from there: three
    launches whatever max_gap is, one workgroup walking the frames in order; Tracks.velocity).  Constant velocity from the last link only:
    wrong after a sharp turn, where a track can end and restart.  Not with matching='optimal': the assignment kernel's frame-parallel
    level launch cannot know the velocities; combining the two is left to a later change and refused until then.
    max_dt: None (max_gap + 1) or a finite number > 0, read by calls with time stamps only: the longest time, in frame periods, over which
    a track is continued.  `linker(x, times=seq)`: seq a host sequence or numpy array of one real, finite number per frame of the batch,
    strictly increasing and after the previous call's last (ValueError before any launch otherwise, the state unmoved); the time between
    two frames then stands where their distance in frames stood -- in the gate, the prediction and the velocity -- so a dropped frame is
    a gap and jitter is accounted for.  A linker is timed or not from its first call to the next reset().
    Without time stamps frames are taken to be consecutive and in order; a track missing from more than max_gap frames ends (levels
    count frames present, so with time stamps max_gap also bounds how many present frames a track may skip); without
    motion='velocity' there is no motion prediction; the assignment is optimal per (level, frame pair), not over time.  No counterpart in the
    reference; what max_step, lam, max_cos, max_gap and matching do to tracking quality can be measured with TrackScorer wherever person
    ids exist (DESIGN.md section 9 has both matchings on synthetic sequences); with a trained model it has not been."""

    def __init__(self, max_step, lam=1.0, max_cos=None, max_gap=0, matching="mutual", miss_cost=None, motion="none", max_dt=None):
        real = _real
        if not real(max_step) or not math.isfinite(max_step) or not max_step > 0:
            raise ValueError(f"max_step must be a finite number > 0, not {max_step!r}")
        if not real(lam) or not math.isfinite(lam) or lam < 0:
            raise ValueError(f"lam must be a finite number >= 0, not {lam!r}")
        if max_cos is not None and (not real(max_cos) or not 0 <= max_cos <= 2):
            raise ValueError(f"max_cos must be None or a number in [0, 2], not {max_cos!r}")
        if isinstance(max_gap, bool) or not isinstance(max_gap, numbers.Integral) or not 0 <= max_gap <= MAX_GAP:
            raise ValueError(f"max_gap must be an integer in [0, {MAX_GAP}], not {max_gap!r}")
        self.max_step, self.lam, self.max_cos = float(max_step), float(lam), None if max_cos is None else float(max_cos)
        if not isinstance(matching, str) or matching not in nat.MATCHING:
            raise ValueError(f"matching must be 'mutual' or 'optimal', not {matching!r}")
        if miss_cost is not None:
            if matching != "optimal":
                raise ValueError("miss_cost is the price of staying unlinked under matching='optimal'; matching='mutual' has no such price")
            if not real(miss_cost) or not math.isfinite(miss_cost) or not miss_cost > 0:
                raise ValueError(f"miss_cost must be None or a finite number > 0, not {miss_cost!r}")
        if not isinstance(motion, str) or motion not in nat.MOTION:
            raise ValueError(f"motion must be 'none' or 'velocity', not {motion!r}")
        if motion == "velocity" and matching == "optimal":
            raise ValueError("motion='velocity' cannot be combined with matching='optimal' yet: the assignment kernel links all frames of a "
                             "level at once and cannot know the velocities")
        if max_dt is not None and (not real(max_dt) or not math.isfinite(max_dt) or not max_dt > 0):
            raise ValueError(f"max_dt must be None or a finite number > 0, not {max_dt!r}")
        self.max_gap = int(max_gap)
        self.max_dt = float(max_dt) if max_dt is not None else float(self.max_gap + 1)   # (read by timed calls only)
        self.matching = matching
        self.motion = motion
        self.miss_cost = float(miss_cost) if miss_cost is not None else 1.0 + self.lam * (self.max_cos if self.max_cos is not None else 2.0)
        self.reset()

    def reset(self):
        """Forget the carried frames and the id counter."""
        self._state, self._cap, self._reid_dim = None, 0, None
        self._state_motion = None   # the motion of the linker that wrote the state (only by changing `motion` can it differ from self.motion)
        self._frame_rows = []   # max_gap > 0: the node counts of the frames the state holds, oldest first (they bound the cluster counts)
        self._frame_times = []  # timed calls: the times of those frames, beside _frame_rows (the state on the device does not hold them)
        self._state_timed = None   # did the call that wrote the state have time stamps (a state continues only in kind)

    @property
    def needs_embeddings(self):
        return self.lam != 0.0 or self.max_cos is not None

    def _host_times(self, times, g):
        """The time stamps of a batch of g frames, checked on the host -> float64 [g].  ValueError: not a sequence of g real, finite,
        strictly increasing numbers, or the first is not after the last time of the previous call."""
        try:
            seq = list(times)
        except TypeError:
            raise ValueError(f"times must be a sequence of {g} numbers, one per frame, not {times!r}") from None
        if len(seq) != g:
            raise ValueError(f"the batch has {g} frames, times has {len(seq)} entries")
        for v in seq:
            if not _real(v) or not math.isfinite(v):
                raise ValueError(f"every time must be a finite real number, not {v!r}")
        t = np.array([float(v) for v in seq], dtype=np.float64)
        if g > 1 and not bool((np.diff(t) > 0).all()):
            raise ValueError("times must be strictly increasing: frames come in order, one time stamp each")
        if g > 0 and self._frame_times and not t[0] > self._frame_times[-1]:
            raise ValueError(f"the first time, {t[0]!r}, is not after the last time of the previous call, {self._frame_times[-1]!r}")
        return t

    def __call__(self, x, times=None):
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
        if self.matching == "optimal":   # before any launch, and before the state moves
            if self._state is not None and not self._frame_rows:   # (only by changing `matching` on a linker that has linked already)
                raise ValueError("the carried state was written by the adjacent-frame linker (matching='mutual', max_gap=0), which "
                                 "matching='optimal' cannot continue: reset() it first")
            worst = max([max_n] + self._frame_rows)
            if worst > MAX_OPTIMAL_FRAME_NODES:
                where = "the batch" if max_n > MAX_OPTIMAL_FRAME_NODES else "the carried history"
                raise ValueError(f"a frame of {where} has {worst} detections; FrameLinker(matching='optimal') takes frames of at most "
                                 f"{MAX_OPTIMAL_FRAME_NODES} (reset() forgets the history)")
        self._check_mode()
        if self._state is not None and self._state_motion != self.motion:
            raise ValueError(f"the carried state was written with motion={self._state_motion!r}, which motion={self.motion!r} cannot "
                             "continue (the states differ in kind): reset() it first")
        timed = times is not None
        if self._state is not None and self._state_timed != timed:
            was, now = ("with", "without") if self._state_timed else ("without", "with")
            raise ValueError(f"the carried state was written {was} time stamps, which a call {now} them cannot continue: reset() it first")
        if timed:   # on the host, before any launch and before the state moves
            if not _real(self.max_dt) or not math.isfinite(self.max_dt) or not self.max_dt > 0:   # (changed after construction)
                raise ValueError(f"max_dt must be a finite number > 0, not {self.max_dt!r}")
            times = self._host_times(times, g)
        dev = s.count.device
        self._reid_dim = r_all
        r = r_all if self.needs_embeddings else 0
        lib = nat.lib()
        with _on(dev):
            if g == 0:   # nothing to link: the state stays
                return self._no_frames(dev)
            if timed or self.motion != "none" or self.max_gap > 0 or self.matching == "optimal":
                return self._link_history(lib, s, dev, sizes, g, n, max_n, r, times)
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
        self._state, self._cap, self._state_motion, self._state_timed = state, cap, self.motion, False
        return Tracks(tracks[0], tracks[1], matched, state[:8].view(torch.int64), state)

    def _check_mode(self):
        """ValueError unless the attributes that choose the kernels (they may have been changed after construction) name a linker this
        class has.  A subclass with a mode of its own answers for it here."""
        if self.motion not in nat.MOTION or (self.motion == "velocity" and self.matching == "optimal"):
            raise ValueError(f"motion={self.motion!r} with matching={self.matching!r} is not a linker this module has")

    def _no_frames(self, dev):
        """What a call with a batch of no frames returns (inside _on(dev)): empty Tracks, the id counter as it stands; the state stays."""
        nid = self._state[:8].view(torch.int64) if self._state is not None else torch.zeros(1, dtype=torch.int64, device=dev)
        e64, e32 = torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
        vel = torch.empty((0, 2), dtype=torch.float64, device=dev) if self.motion != "none" else None
        return Tracks(e64, e64.clone(), e32, nid, self._state, e32.clone(), vel)

    def _stage_times(self, times, dev):
        """The times of the carried frames, then the batch's checked `times` -> (the combined host list, its device copy: a fresh pinned
        buffer and one non-blocking copy on the current stream)."""
        all_times = self._frame_times + times.tolist()   # (one time per carried frame: _frame_times moves with _frame_rows)
        staged = torch.empty(len(all_times), dtype=torch.float64, pin_memory=True)
        staged.copy_(torch.from_numpy(np.asarray(all_times, dtype=np.float64)))
        return all_times, staged.to(dev, non_blocking=True)

    def _advance(self, state, out_rows, all_times):
        """The history state moves on after a call that linked: the new device state, the node counts of the frames it holds and, from
        a timed call (all_times not None), their times."""
        self._state, self._frame_rows, self._state_motion, self._state_timed = state, out_rows, self.motion, all_times is not None
        self._frame_times = all_times[-len(out_rows):] if all_times is not None else []

    def _link_history(self, lib, s, dev, sizes, g, n, max_n, r, times=None):
        """The call of every linker whose state is a history of frames (inside _on(dev), g > 0) -- max_gap > 0, matching='optimal',
        motion='velocity', and every call with time stamps: everything is sized from host-known node counts, nothing waits for the GPU.
        The entries differ in the kind of their state and workspace, and with motion (three launches do it all) a velocity per row comes
        back.  `times`: None, or the checked float64 [g] of the batch -- the times of the carried frames come before them, the whole goes
        through a fresh pinned buffer (the host allocator hands its block out again only after the copy's event has passed) and one
        non-blocking copy on the current stream, and the _timed form of the entry is called."""
        moving = self.motion == "velocity"
        state_bytes, workspace_bytes = ((lib.gnncca_link_motion_state_bytes, lib.gnncca_link_motion_workspace_bytes) if moving else
                                        (lib.gnncca_link_gap_state_bytes, lib.gnncca_link_gap_workspace_bytes))
        in_rows = self._frame_rows
        out_rows = (in_rows + [int(v) for v in sizes])[-(self.max_gap + 1):]
        c_in, c_out = (C.c_int32 * max(len(in_rows), 1))(*in_rows), (C.c_int32 * len(out_rows))(*out_rows)
        state = torch.empty(state_bytes(sum(out_rows), len(out_rows), r), dtype=torch.uint8, device=dev)
        tracks = torch.empty((2, n), dtype=torch.int64, device=dev)   # cluster_track | node_track
        matched = torch.empty((2, n), dtype=torch.int32, device=dev)   # matched_prev | matched_gap
        velocity = torch.empty((n, 2), dtype=torch.float64, device=dev) if moving else None
        ws_bytes = workspace_bytes(n, g, sum(in_rows))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        head = (s.node_ptr_dev.data_ptr(), s.count.data_ptr(), s.rank.data_ptr() if n else None, s.pos.data_ptr() if n else None,
                s.emb.data_ptr() if r and n else None, r, n, g, max_n, self.max_step, self.lam, int(self.max_cos is not None),
                self.max_cos if self.max_cos is not None else 0.0, self.max_gap)
        tail = (self._state.data_ptr() if in_rows else None, c_in, len(in_rows), state.data_ptr(), c_out, len(out_rows),
                tracks[0].data_ptr() if n else None, tracks[1].data_ptr() if n else None, matched[0].data_ptr() if n else None,
                matched[1].data_ptr() if n else None)
        end = (ws.data_ptr(), ws_bytes, _raw_stream(dev))
        all_times = None
        if times is not None:
            all_times, times_dev = self._stage_times(times, dev)
            if moving:
                name = "gnncca_link_frames_motion_timed"
                st = lib.gnncca_link_frames_motion_timed(*head, nat.MOTION[self.motion], *tail, velocity.data_ptr() if n else None, *end,
                                                         times_dev.data_ptr(), self.max_dt)
            else:
                name = "gnncca_link_frames_gap_timed"
                st = lib.gnncca_link_frames_gap_timed(*head, nat.MATCHING[self.matching], self.miss_cost, *tail, *end, times_dev.data_ptr(),
                                                      self.max_dt)
            # times_dev is freed in stream order like the workspace (allocated on this stream): the launches above still read it
        elif moving:
            name = "gnncca_link_frames_motion"
            st = lib.gnncca_link_frames_motion(*head, nat.MOTION[self.motion], *tail, velocity.data_ptr() if n else None, *end)
        elif self.matching == "optimal":
            name = "gnncca_link_frames_gap"
            st = lib.gnncca_link_frames_gap_ex(*head, nat.MATCHING[self.matching], self.miss_cost, *tail, *end)
        else:   # 'mutual': the entry it has always run
            name = "gnncca_link_frames_gap"
            st = lib.gnncca_link_frames_gap(*head, *tail, *end)
        if st:
            nat.check(st, name)
        # the previous state and the workspace are freed in stream order (allocated on this stream): the launches above still read them
        self._advance(state, out_rows, all_times)
        return Tracks(tracks[0], tracks[1], matched[0], state[:8].view(torch.int64), state, matched[1], velocity)


class TrackScores:
    """What one TrackScorer.add returns: switched int32 [N] on the device -- -1: the detection is not scored, 0, 1: it is an identity
    switch (its stream's latest earlier scored detection had another track)."""
    __slots__ = ("switched",)

    def __init__(self, switched):
        self.switched = switched


_TRACK_BITS = 40


def _scores_of(cells, ignored, idsw):
    """result() from the integer state: cells = the non-zero (p, t, n) of the pair table in ascending (p, t), Python ints throughout."""
    from scipy.optimize import linear_sum_assignment
    total = sum(c[2] for c in cells)
    if total == 0:
        raise ValueError("TrackScorer.result: no detection was scored")
    row, col, best_of_p, best_of_t = {}, {}, {}, {}
    for p, t, n in cells:
        row[p], col[t] = row.get(p, 0) + n, col.get(t, 0) + n
        best_of_p[p], best_of_t[t] = max(best_of_p.get(p, 0), n), max(best_of_t.get(t, 0), n)
    pi, ti = {p: i for i, p in enumerate(sorted(row))}, {t: i for i, t in enumerate(sorted(col))}
    dense = np.zeros((len(pi), len(ti)), np.int64)
    for p, t, n in cells:
        dense[pi[p], ti[t]] = n
    rr, cc = linear_sum_assignment(dense, maximize=True)   # the assignment may not be unique, its total is
    idtp = int(dense[rr, cc].sum())
    assa = math.fsum(n * n / (row[p] + col[t] - n) for p, t, n in cells) / total
    mt = sum(1 for p in row if best_of_p[p] / row[p] >= 0.8)
    ml = sum(1 for p in row if best_of_p[p] / row[p] <= 0.2)
    return {"detections": total, "ignored": ignored, "ids": len(row), "tracks": len(col), "pairs": len(cells), "IDSW": idsw, "IDTP": idtp,
            "IDF1": idtp / total, "AssA": assa, "purity": sum(best_of_t.values()) / total, "coverage": sum(best_of_p.values()) / total,
            "MT": mt, "PT": len(row) - mt - ml, "ML": ml, "tracks_per_id": len(cells) / len(row)}


class TrackScorer:
    """Identity-tracking scores of track ids against the caller's person ids, accumulated over the frames of a sequence on the device (the
    module docstring has the rule).  `add(x, tracks)` takes x, a pipeline.FrameResult or a GraphBatch of build_graph_batch / FramePipeline
    (ids = batch.y, cam and the frame offsets from the batch), and the Tracks a FrameLinker made of it; `add_raw` plain device tensors.
    Both enqueue on the current stream, never wait for the GPU and return a TrackScores (switched int32 [N]).  `counts` is an int64 [4]
    device view of scored, ignored, switches, pairs (the non-zero cells of n[person][track]), cumulative since reset() (zeros on the host
    before the first add).  `result()` copies the state back ONCE and returns a dict:
      detections (N, the scored ones), ignored, ids / tracks (persons / tracks with a scored detection), pairs, IDSW;
      IDTP  the largest total of n over one-to-one assignments of persons to tracks (scipy's linear_sum_assignment on the dense matrix);
      IDF1 = IDTP / N.  Every ground-truth detection is also a hypothesis detection here, so IDP = IDR = IDF1;
      AssA = fsum(n * n / (row[p] + col[t] - n) over the cells in ascending (p, t)) / N: HOTA's association accuracy at perfect detection;
      purity = sum_t max_p n / N, coverage = sum_p max_t n / N;
      MT, PT, ML  persons with max_t n[p][t] / row[p] >= 0.8, in between, <= 0.2 (on identity coverage: detection is perfect here);
      tracks_per_id = pairs / ids.
    ValueError if nothing was scored.  The state is sized from numbers the host knows: last [max_ids * max_cams] and a hash table of `cap`
    cells, cap >= 2 x the detections passed so far (they bound the pairs) and >= 1024; a call that needs more allocates the next power of
    two and one launch re-inserts the old cells.  A batch whose slot image [G][max_ids * max_cams] exceeds 2**22 entries is cut into runs
    of frames (the rule is causal).  Frames have no size limit here.  No counterpart in the reference."""

    def __init__(self, max_ids=1024, max_cams=8):
        def integer(v):
            return isinstance(v, numbers.Integral) and not isinstance(v, bool)
        if not integer(max_ids) or not 1 <= max_ids <= nat.SCORE_MAX_IDS:
            raise ValueError(f"max_ids must be an integer in [1, {nat.SCORE_MAX_IDS}], not {max_ids!r}")
        if not integer(max_cams) or not 1 <= max_cams <= nat.SCORE_MAX_CAMS:
            raise ValueError(f"max_cams must be an integer in [1, {nat.SCORE_MAX_CAMS}], not {max_cams!r}")
        if max_ids * max_cams > nat.SCORE_MAX_STREAMS:
            raise ValueError(f"max_ids * max_cams = {max_ids * max_cams} streams; TrackScorer takes at most {nat.SCORE_MAX_STREAMS}")
        self.max_ids, self.max_cams, self.n_streams = int(max_ids), int(max_cams), int(max_ids) * int(max_cams)
        self.reset()

    def reset(self):
        """Forget everything scored so far."""
        self._table, self._last, self._cap, self._seen = None, None, 0, 0

    @property
    def cap(self):
        """The cells of the pair table as it stands (0 before the first add)."""
        return self._cap

    @property
    def counts(self):
        return self._table[:4] if self._table is not None else torch.zeros(4, dtype=torch.int64)

    def _grow(self, lib, dev, n):
        """The state for n more detections (inside _on(dev)): first use, or a table of the next sufficient power of two."""
        need = nat.SCORE_MIN_CAP
        while need < 2 * (self._seen + n):
            need *= 2
        if self._table is not None and self._table.device != dev:
            raise ValueError(f"the scorer's state is on {self._table.device}, the batch on {dev}: reset() it first")
        if self._table is not None and need <= self._cap:
            return
        table = torch.empty(nat.SCORE_HEADER_LEN + 2 * need, dtype=torch.int64, device=dev)
        if self._table is None:
            self._last = torch.empty(self.n_streams, dtype=torch.int64, device=dev)
            st = lib.gnncca_track_score_reset(table.data_ptr(), need, self._last.data_ptr(), self.n_streams, _raw_stream(dev))
        else:   # (the old table is freed in stream order: the launch above it still reads it)
            st = lib.gnncca_track_score_rehash(self._table.data_ptr(), self._cap, table.data_ptr(), need, _raw_stream(dev))
        if st:
            nat.check(st, "gnncca_track_score_reset / rehash")
        self._table, self._cap = table, need

    def add_raw(self, ids, cam, node_track, node_ptr, node_ptr_dev=None):
        """ids int64 [N], cam int32 [N], node_track int64 [N] on the device; node_ptr: the G + 1 frame offsets as a HOST sequence (uploaded
        here unless node_ptr_dev, its int32 device copy, is given).  Enqueued on the current stream -> TrackScores."""
        ptr = _host_ptr(node_ptr)
        g = len(ptr) - 1
        for name, t, dt in (("ids", ids, torch.int64), ("cam", cam, torch.int32), ("node_track", node_track, torch.int64)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
                raise ValueError(f"{name} must be a 1-D {dt} tensor")
        n = int(ids.numel())
        if cam.numel() != n or node_track.numel() != n or int(ptr[0]) != 0 or int(ptr[-1]) != n or (g > 0 and int(np.diff(ptr).min()) < 0):
            raise ValueError(f"ids [{n}], cam [{cam.numel()}], node_track [{node_track.numel()}] and node_ptr ({ptr[0]} .. {ptr[-1]}) disagree")
        if n >= 2 ** 31 - 256:
            raise ValueError(f"{n} detections in one call; TrackScorer takes fewer than 2**31")
        if node_ptr_dev is not None and (node_ptr_dev.dtype != torch.int32 or node_ptr_dev.numel() != g + 1):
            raise ValueError(f"node_ptr_dev must be int32 [{g + 1}]")
        if not (ids.is_cuda and cam.is_cuda and node_track.is_cuda):
            raise RuntimeError("gnn_cca_amd.tracking runs on MI355X only (no CPU fallback)")
        dev = ids.device
        lib = nat.lib()
        with _on(dev):
            switched = torch.empty(n, dtype=torch.int32, device=dev)
            if g == 0:   # no time passes (and the state holds no time anyway)
                return TrackScores(switched)
            self._grow(lib, dev, n)
            if n:
                ids, cam, node_track = ids.contiguous(), cam.contiguous(), node_track.contiguous()
                nptr = (node_ptr_dev if node_ptr_dev is not None else torch.from_numpy(ptr.astype(np.int32))).to(device=dev).contiguous()
                per_run = nat.SCORE_MAX_SLOTS // self.n_streams   # frames per native call: its slot image holds at most 2**22 entries
                slot = torch.empty(min(g, per_run) * self.n_streams, dtype=torch.int32, device=dev)
                for f0 in range(0, g, per_run):
                    f1 = min(g, f0 + per_run)
                    v0, v1 = int(ptr[f0]), int(ptr[f1])
                    if v1 == v0:
                        continue
                    st = lib.gnncca_track_score_add(ids.data_ptr() + 8 * v0, cam.data_ptr() + 4 * v0, node_track.data_ptr() + 8 * v0,
                                                    nptr.data_ptr() + 4 * f0, v0, v1 - v0, f1 - f0, self.max_ids, self.max_cams,
                                                    self._table.data_ptr(), self._cap, self._last.data_ptr(), slot.data_ptr(),
                                                    switched.data_ptr() + 4 * v0, _raw_stream(dev))
                    if st:
                        nat.check(st, "gnncca_track_score_add")
                # the slot image is freed in stream order (allocated on this stream): the launches above still use it
                self._seen += n
        return TrackScores(switched)

    def add(self, x, tracks):
        """x: a pipeline.FrameResult or a GraphBatch (ids = batch.y, cam from its staging image, frame offsets batch.node_ptr / node_ptr_dev);
        tracks: the Tracks a FrameLinker returned for it.  Enqueued on the current stream, no synchronisation -> TrackScores."""
        batch = getattr(x, "batch", x)
        frames = getattr(batch, "_frames", None)
        if frames is None:
            raise ValueError("TrackScorer.add needs a FrameResult or a batch of build_graph_batch / FramePipeline (its staging image holds the "
                             "cameras); use add_raw for plain tensors")
        if not isinstance(tracks, Tracks):
            raise ValueError("TrackScorer.add takes the Tracks of a FrameLinker")
        image, layout = frames
        return self.add_raw(batch.y, layout.view(image, "cam"), tracks.node_track, batch.node_ptr, node_ptr_dev=batch.node_ptr_dev)

    def result(self):
        """The scores so far as a dict (the class docstring has the keys): ONE copy of the state, one synchronisation, then integer work on
        the host in a fixed order.  ValueError if nothing was scored; RuntimeError if the pair table overflowed (a sizing bug: it cannot)."""
        if self._table is None:
            raise ValueError("TrackScorer.result: no detection was scored")
        host = self._table.cpu().numpy()   # the one synchronisation
        scored, ignored, switches, pairs, overflow = (int(v) for v in host[:5])
        if overflow:
            raise RuntimeError("TrackScorer: the pair table overflowed and dropped counts (its capacity was sized wrongly)")
        keys = host[nat.SCORE_HEADER_LEN:nat.SCORE_HEADER_LEN + self._cap].view(np.uint64)
        cnt = host[nat.SCORE_HEADER_LEN + self._cap:]
        used = np.flatnonzero(keys != np.uint64(2 ** 64 - 1))
        used = used[np.argsort(keys[used], kind="stable")]   # ascending key = ascending (p, t); the keys are distinct
        cells = [(int(k) >> _TRACK_BITS, int(k) & (2 ** _TRACK_BITS - 1), int(c)) for k, c in zip(keys[used].tolist(), cnt[used].tolist())]
        if len(cells) != pairs or sum(c[2] for c in cells) != scored:
            raise RuntimeError(f"TrackScorer: the pair table ({len(cells)} cells, {sum(c[2] for c in cells)} detections) and the counters "
                               f"({pairs}, {scored}) disagree")
        return _scores_of(cells, ignored, switches)


__all__ = ["MAX_FRAME_NODES", "MAX_GAP", "MAX_OPTIMAL_FRAME_NODES", "ClusterSummaries", "Tracks", "cluster_summaries", "cluster_summaries_raw", "FrameLinker", "TrackScorer",
           "TrackScores"]
