"""The staging image of a batch of frames (gnncca_plan_frames writes it, ONE non-blocking copy uploads it; the edge kernels, the one-call
pipeline and the post stage read it) and the host work in front of the kernels that graph_build.build_graph_batch and
pipeline.FramePipeline share.  `FrameLayout` is the only place in Python that knows the order of the image's fields (the library's is
csrc/internal.h: StagingImage).  All of it runs once per batch on a host-bound path: __slots__, integer arithmetic, no per-field objects."""
import ctypes as C
import numbers
from itertools import accumulate
from operator import mul

import numpy as np
import torch

from . import _native as nat


def _raw_stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index)


_stream_objs = {}


def _current_stream(dev):
    """torch.cuda.current_stream(dev) through a cache keyed by the raw handle (the call itself costs ~10 us of host time)."""
    raw = _raw_stream(dev)
    hit = _stream_objs.get(dev.index)
    if hit is None or hit[0] != raw:
        hit = _stream_objs[dev.index] = (raw, torch.cuda.current_stream(dev))
    return hit[1]


class _on:
    """`with torch.cuda.device(dev)` only when `dev` is not the current device already (the context manager costs ~5 us of host
    time per use, more than a launch)."""

    def __init__(self, dev):
        self._ctx = None if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()

    def __exit__(self, *a):
        if self._ctx is not None:
            self._ctx.__exit__(*a)


def _f32c(x):
    return x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()


def _as(a, dtype):
    a = np.asarray(a)
    if a.dtype != dtype or not a.flags.c_contiguous:
        a = np.ascontiguousarray(a, dtype=dtype)
    return a


class _Staging:
    """Ring of pinned host buffers for the per-batch staging image (gnncca_plan_frames writes it, ONE non-blocking copy uploads
    it): the host never waits for the GPU, so the graph of the next batch of frames is planned while this one's kernels run.
    A slot is reused only after the copy that read it has completed (its event)."""
    SLOTS = 8

    def __init__(self):
        self._bufs, self._events, self._next = [None] * self.SLOTS, [None] * self.SLOTS, 0

    def take(self, nbytes):
        i = self._next
        self._next = (i + 1) % self.SLOTS
        if self._events[i] is not None:
            self._events[i].synchronize()
        buf = self._bufs[i]
        if buf is None or buf.numel() < nbytes:
            buf = self._bufs[i] = torch.empty(max(2 * nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        if self._events[i] is None:
            self._events[i] = torch.cuda.Event()
        return buf, self._events[i]


_staging = {}   # device index -> its ring


FIELDS = ("xw", "yw", "max_dist", "ids", "person", "cam", "graph_of", "graph_ptr", "src_order", "edge_ptr", "edge_ptr_g")
INDEX = {name: k for k, name in enumerate(FIELDS)}
_TYPES = ((np.float64, torch.float64),) * 3 + ((np.int64, torch.int64),) + ((np.int32, torch.int32),) * 7   # (numpy, torch) per field
_SIZES = tuple(np.dtype(t[0]).itemsize for t in _TYPES)
_FRAMES = tuple(INDEX["person" if name == "person_id" else name] for name, _ in nat.Frames._fields_)   # gnncca_frames: nine of the eleven


class FrameLayout:
    """The staging image of `n` detections in `g` frames, eleven arrays back to back in the order of FIELDS, 8-byte fields first:
      f64 xw[n], yw[n], max_dist[g];  i64 ids[n] (the caller's person ids: batch.y);  i32 person[n] (their relabelling, equality preserved),
      cam[n], graph_of[n], graph_ptr[g + 1], src_order[n], edge_ptr[n + 1], edge_ptr_g[g + 1] (the first edge of each frame)
    `cnt[k]` elements at byte `off[k]` for field k = INDEX[name]; off[-1] == nbytes."""
    __slots__ = ("n", "g", "cnt", "off", "nbytes")

    def __init__(self, n, g):
        self.n, self.g = n, g
        self.cnt = cnt = (n, n, g, n, n, n, n, g + 1, n, n + 1, g + 1)
        self.off = off = (0, *accumulate(map(mul, _SIZES, cnt)))
        self.nbytes = off[-1]

    def view(self, image, name):
        """Field `name` of an image held in a uint8 torch tensor (device or pinned) or numpy array, as a typed view."""
        k = INDEX[name]
        return image[self.off[k]:self.off[k + 1]].view(_TYPES[k][isinstance(image, torch.Tensor)])

    def frames(self, base):
        """gnncca_frames for an image at address `base`."""
        return nat.Frames(*[base + self.off[k] for k in _FRAMES])

    def host_ptrs(self, pinned):
        """(node_ptr, edge_ptr) as host lists: frame q owns the nodes node_ptr[q] .. node_ptr[q + 1] and the edges edge_ptr[q] .. edge_ptr[q + 1]."""
        image = pinned.numpy()
        return self.view(image, "graph_ptr").tolist(), self.view(image, "edge_ptr_g").tolist()


def check_cap(top_k, rank_by, symmetric):
    """The arguments of a capped graph (build_graph_batch has their meaning) -> (top_k, rank code, symmetric code), or ValueError."""
    if rank_by not in nat.RANK_BY:
        raise ValueError(f"rank_by must be 'ground' or 'reid', not {rank_by!r}")
    if symmetric is not None:
        if not isinstance(symmetric, str) or symmetric not in nat.SYMMETRIC:
            raise ValueError(f"symmetric must be None, 'union' or 'mutual', not {symmetric!r}")
        if top_k is None:
            raise ValueError("symmetric=... closes a capped graph under reversal: it needs top_k")
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral):
            raise ValueError(f"top_k must be None or an integer >= 1, not {top_k!r}")
        if top_k < 1:
            raise ValueError(f"top_k must be >= 1, not {top_k}")
        top_k = min(int(top_k), 2 ** 31 - 1)
    return top_k, nat.RANK_BY[rank_by], nat.SYMMETRIC[symmetric] if symmetric else 0


def check_radius(radius, radius_unit, top_k=None, symmetric=None):
    """The arguments of a radius-gated graph (build_graph_batch has their meaning) -> (radius as a float or None, unit code), or ValueError:
    radius is None, a finite number >= 0 or inf (no bool, no NaN); the unit 'ground' or 'max_dist'; no top_k / symmetric next to a radius."""
    if not isinstance(radius_unit, str) or radius_unit not in nat.RADIUS_UNIT:
        raise ValueError(f"radius_unit must be 'ground' or 'max_dist', not {radius_unit!r}")
    if radius is None:
        return None, nat.RADIUS_UNIT[radius_unit]
    if isinstance(radius, bool) or not isinstance(radius, numbers.Real):
        raise ValueError(f"radius must be None, a number >= 0 or inf, not {radius!r}")
    radius = float(radius)
    if not radius >= 0.0:   # (a NaN fails the comparison too)
        raise ValueError(f"radius must be None, a number >= 0 or inf, not {radius!r}")
    if top_k is not None or symmetric is not None:
        raise ValueError("radius together with top_k / symmetric is not supported: a radius-gated k-nearest list has no definition here yet")
    return radius, nat.RADIUS_UNIT[radius_unit]


class Selection:
    """Which of a detection's cross-camera candidates a graph keeps: all (dense), the top_k with the smallest key (capped; sym != 0 closes
    the list under reversal), or those within a radius (gated).  The codes are check_cap's and check_radius'.  The native library has one
    entry point per kind and stage -- gnncca_plan_frames / _ex / _radius, gnncca_build_edges / _topk / _radius, gnncca_frames_forward /
    _topk / _radius -- and this class is the one place that chooses among them."""
    __slots__ = ("top_k", "rank", "sym", "radius", "unit")

    def __init__(self, top_k, rank, sym, radius, unit):
        self.top_k, self.rank, self.sym, self.radius, self.unit = top_k, rank, sym, radius, unit

    @property
    def pruned(self):
        """The edge list is a proper subsequence of the dense one."""
        return self.top_k is not None or self.radius is not None

    def plan(self, lib, arrays, image_ptr, nbytes, max_deg):
        """The host plan of this selection into the image; `max_deg` (a c_int32) receives the largest uncapped degree of a capped plan."""
        if self.radius is not None:
            return lib.gnncca_plan_frames_radius(*arrays, self.radius, self.unit, image_ptr, nbytes)
        if self.top_k is None:
            return lib.gnncca_plan_frames(*arrays, image_ptr, nbytes)
        return lib.gnncca_plan_frames_ex(*arrays, self.top_k, image_ptr, nbytes, C.byref(max_deg))

    def launch(self, lib, base, head, max_deg, tail):
        """base(*head, <this selection's own arguments>, *tail) at the entry point of this kind: `base` itself for the dense graph, base +
        '_topk' / '_radius' otherwise, whose signatures differ from the dense one's by those arguments.  Raises on a refusal."""
        if self.radius is not None:
            base, own = base + "_radius", (self.radius, self.unit)
        elif self.top_k is not None:
            base, own = base + "_topk", (self.top_k, self.rank, max_deg)
        else:
            own = ()
        st = getattr(lib, base)(*head, *own, *tail)
        if st:
            nat.check(st, base)


def select(top_k, rank_by, symmetric, radius, radius_unit):
    """The Selection of build_graph_batch's / FramePipeline's arguments, or their ValueError: check_cap, then check_radius."""
    top_k, rank, sym = check_cap(top_k, rank_by, symmetric)
    return Selection(top_k, rank, sym, *check_radius(radius, radius_unit, top_k, symmetric))


class StagedFrames:
    """The host side of one batch of frames.  The constructor converts the six host arrays (`arrays`: xw, yw, ids, id_cam, graph_sizes,
    max_dist as contiguous float64 / int64) and checks their lengths; nothing else is touched, so the caller can still refuse the batch.
    plan() enumerates the edges into a slot of the device's pinned ring (sets e, max_deg, pinned), upload(dst) queues the one copy."""
    __slots__ = ("arrays", "n", "g", "layout", "e", "max_deg", "pinned", "_event")
    LENGTHS_DISAGREE = "per-detection / per-frame arrays disagree on their lengths"

    def __init__(self, xw, yw, ids, id_cam, graph_sizes, max_dist):
        xw, yw, md = _as(xw, np.float64), _as(yw, np.float64), _as(max_dist, np.float64)
        ids64, cam64, sizes = _as(ids, np.int64), _as(id_cam, np.int64), _as(graph_sizes, np.int64)
        n, g = len(cam64), len(sizes)
        if not (len(xw) == len(yw) == len(ids64) == n) or len(md) != g:
            raise ValueError(self.LENGTHS_DISAGREE)
        self.arrays, self.n, self.g, self.layout = (xw, yw, ids64, cam64, sizes, md), n, g, FrameLayout(n, g)

    def plan(self, dev, sel):
        """The host plan of Selection `sel` into the ring's next slot; waits only if that slot's upload is still queued."""
        lib = nat.lib()
        nbytes = lib.gnncca_plan_frames_bytes(self.n, self.g)
        assert nbytes == self.layout.nbytes   # the library's StagingImage and FrameLayout agree
        ring = _staging.get(dev.index) or _staging.setdefault(dev.index, _Staging())
        self.pinned, self._event = pinned, _ = ring.take(nbytes)
        xw, yw, ids64, cam64, sizes, md = self.arrays
        args = (xw.ctypes.data, yw.ctypes.data, ids64.ctypes.data, cam64.ctypes.data, self.n, sizes.ctypes.data, md.ctypes.data, self.g)
        max_deg = C.c_int32(0)
        e = sel.plan(lib, args, pinned.data_ptr(), nbytes, max_deg)
        if e < 0:
            if -e == nat.ERR_INVALID_ARG:
                raise ValueError("id_cam length does not match graph_sizes")
            nat.check(int(-e), "gnncca_plan_frames")
        self.e, self.max_deg = e, max_deg.value
        if self.max_deg > nat.TOPK_MAX_DEG:   # (gnncca_build_edges_topk refuses it too; here nothing has been launched yet)
            raise NotImplementedError(f"build_graph_batch(top_k=...): a detection with {self.max_deg} cross-camera candidates; the capped "
                                      f"build takes at most {nat.TOPK_MAX_DEG} per detection")

    def upload(self, dst):
        """The image into `dst` (uint8 [layout.nbytes] on the device), non-blocking; the ring slot is free again when the copy has run."""
        dst.copy_(self.pinned[:self.layout.nbytes], non_blocking=True)
        self._event.record(_current_stream(dst.device))


def attach(batch, staged, layout, cam_host=None):
    """The device views a GraphBatch carries of its staging image: node_ptr_dev / edge_ptr_dev (int32 [G + 1], for the per-frame
    post-processing), y (the int64 person ids) and the image itself, which batch.person_dev / batch.cam_dev slice when asked for.
    `cam_host`: the host camera ids the image was planned from (StagedFrames.arrays[3]; kept by reference, so that a consumer with a
    limit on them -- FrameResult.exclusive -- can refuse a batch without waiting for the device)."""
    batch.node_ptr_dev, batch.edge_ptr_dev = layout.view(staged, "graph_ptr"), layout.view(staged, "edge_ptr_g")
    batch.y, batch._frames = layout.view(staged, "ids"), (staged, layout)
    batch.cam_host = cam_host
