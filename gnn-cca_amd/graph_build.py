"""Row N1 of SURVEY.md 8f: the step right before the MPN -- building the cross-camera graph and its edge attributes
(`inference.py:189-279`, duplicated at `train.py:257-361` and `train.py:616-692`) -- on the GPU.

The reference does this per frame with Python list comprehensions, sklearn on the host and several GPU<->CPU round
trips (its real end-to-end bottleneck).  Here the host only derives the edge ENUMERATION from the camera ids (O(N)
numpy, `plan_frames`); one HIP kernel (`gnncca_build_edges`) then writes `edge_index`, `edge_attr` and `edge_labels`
for the whole batch of frames, and `gnncca_normalize_columns` does the `F.normalize(..., dim=0)` of the embeddings.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .frames import StagedFrames, _current_stream, _f32c, _on, _raw_stream, attach, check_cap, check_radius, select  # noqa: F401  (the lean device helpers live there)
from .sharding import GraphBatch

MODE_FULL, MODE_ONLY_APPEARANCE, MODE_ONLY_DIST = 0, 1, 2


@dataclass
class FramePlan:
    src_order: np.ndarray   # [N] int32  node ids in the order the reference emits their out-edges
    edge_ptr: np.ndarray    # [N+1] int32 first edge of each source position
    graph_ptr: np.ndarray   # [G+1] int32 node range of each frame graph
    graph_of: np.ndarray    # [N] int32
    n_edges: int


def plan_frames(id_cam, graph_sizes):
    """Edge enumeration of inference.py:207-212: per graph, cameras in np.unique order; within a camera its nodes in
    ascending id; each connects to every node of the other cameras in ascending id."""
    id_cam = np.asarray(id_cam)
    sizes = np.asarray(graph_sizes, dtype=np.int64)
    graph_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(graph_ptr[-1])
    if len(id_cam) != n:
        raise ValueError("id_cam length does not match graph_sizes")
    graph_of = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    # one stable sort of (graph, camera) keys for the whole batch: graph-major, np.unique's camera order inside a graph,
    # node id ascending inside a camera
    _, cam_rank = np.unique(id_cam, return_inverse=True)
    n_cam = int(cam_rank.max()) + 1 if n else 1
    key = graph_of.astype(np.int64) * n_cam + cam_rank
    src_order = np.argsort(key, kind="stable").astype(np.int32)
    same_cam = np.bincount(key, minlength=len(sizes) * n_cam)
    deg = (sizes[graph_of] - same_cam[key])[src_order]
    edge_ptr = np.concatenate([[0], np.cumsum(deg)])
    if edge_ptr[-1] >= 2 ** 31 - 64:
        raise NotImplementedError("more than 2^31 edges in one batch")
    return FramePlan(src_order, edge_ptr.astype(np.int32), graph_ptr, graph_of, int(edge_ptr[-1]))


FUSED_NORMALIZE_MAX_ROWS = 4096   # gnncca_normalize_columns2: one launch for up to two matrices of a batch of frames


def _normalize_launch(x, other=None):
    """The launches of normalize_columns on fp32 contiguous matrices: new tensors, no autograd."""
    out = torch.empty_like(x)
    if other is not None:
        if other.shape[0] != x.shape[0]:
            raise ValueError("normalize_columns(x, other): both matrices must have the same number of rows")
        out2 = torch.empty_like(other)
    lib = nat.lib()
    with _on(x.device):
        if x.shape[0] <= FUSED_NORMALIZE_MAX_ROWS and x.dim() == 2:
            st = lib.gnncca_normalize_columns2(x.data_ptr(), x.shape[1], out.data_ptr(), other.data_ptr() if other is not None else None,
                                               other.shape[1] if other is not None else 0, out2.data_ptr() if other is not None else None,
                                               x.shape[0], _raw_stream(x.device))
        else:
            st = 0
            for a, o in ((x, out),) + (((other, out2),) if other is not None else ()):
                scratch = torch.empty(((a.shape[0] + 63) // 64 + 1) * a.shape[1], dtype=torch.float32, device=a.device)  # 64-row chunk sums + norms
                st = st or lib.gnncca_normalize_columns(a.data_ptr(), a.shape[0], a.shape[1], scratch.data_ptr(), o.data_ptr(), _raw_stream(a.device))
    if st:
        nat.check(st, "gnncca_normalize_columns")
    return out if other is None else (out, out2)


def _normalize_backward_launch(jobs):
    """Backward of F.normalize(x, p=2, dim=0) for one or two (x, grad_out) pairs with the same number of rows: [grad_x, ...].  One launch up
    to FUSED_NORMALIZE_MAX_ROWS rows, the three-kernel form (same bits) beyond."""
    lib = nat.lib()
    jobs = [(x, g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous()) for x, g in jobs]
    outs = [torch.empty_like(x) for x, _ in jobs]
    dev = jobs[0][0].device
    with _on(dev):
        if jobs[0][0].shape[0] <= FUSED_NORMALIZE_MAX_ROWS and jobs[0][0].dim() == 2:
            (x0, g0), o0 = jobs[0], outs[0]
            x1, g1, o1 = (jobs[1][0], jobs[1][1], outs[1]) if len(jobs) > 1 else (None, None, None)
            st = lib.gnncca_normalize_columns_backward2(x0.data_ptr(), g0.data_ptr(), x0.shape[1], o0.data_ptr(),
                                                        x1.data_ptr() if x1 is not None else None, g1.data_ptr() if x1 is not None else None,
                                                        x1.shape[1] if x1 is not None else 0, o1.data_ptr() if x1 is not None else None,
                                                        x0.shape[0], _raw_stream(dev))
        else:
            st = 0
            for (x, g), o in zip(jobs, outs):
                rows, cols = x.shape[0], x.numel() // max(x.shape[0], 1)
                nbytes = lib.gnncca_normalize_columns_backward_bytes(rows, cols)
                scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                st = st or lib.gnncca_normalize_columns_backward(x.data_ptr(), g.data_ptr(), rows, cols, scratch.data_ptr(), nbytes, o.data_ptr(),
                                                                 _raw_stream(dev))
    if st:
        nat.check(st, "gnncca_normalize_columns_backward")
    return outs


class _NormalizeFunction(torch.autograd.Function):
    """Autograd bridge of normalize_columns: forward = today's launches, backward = gnncca_normalize_columns_backward(2) for the inputs
    that require grad (nothing is launched or allocated for the others).  Differentiable once."""

    @staticmethod
    def forward(ctx, x, other):
        ctx.set_materialize_grads(False)   # an output nobody used arrives as None, not as a zero matrix
        ctx.save_for_backward(x, other)
        return _normalize_launch(x, other)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        jobs = [(k, saved[k], grads[k]) for k in range(len(grads)) if ctx.needs_input_grad[k] and grads[k] is not None]
        res = [None, None]
        if jobs:
            for (k, _, _), gx in zip(jobs, _normalize_backward_launch([(x, g) for _, x, g in jobs])):
                res[k] = gx
        return tuple(res)


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def normalize_columns(x, other=None):
    """F.normalize(x, p=2, dim=0) (inference.py:189-190) on the GPU; returns a new tensor -- or, given a second matrix with the same
    number of rows (`other`: the reid and the node embeddings of a batch), the pair, normalised in one launch when the batch has at
    most 4096 rows (same bits as the three-kernel form, which takes any size).  Differentiable (once) when grad is enabled and an
    input requires grad; otherwise exactly the launches and allocations of the plain call."""
    if not x.is_cuda or (other is not None and not other.is_cuda):
        raise RuntimeError("gnn_cca_amd.graph_build runs on MI355X only (no CPU fallback)")
    x = _f32c(x)
    if other is not None:
        other = _f32c(other)
    if _wants_grad(x, other):
        if other is not None and other.shape[0] != x.shape[0]:
            raise ValueError("normalize_columns(x, other): both matrices must have the same number of rows")
        return _NormalizeFunction.apply(x, other)
    return _normalize_launch(x, other)


class _EdgeJob:
    """What the edge kernels of one batch need besides the reid table: the staged frame image and its layout, the Selection (frames.py) and,
    for a capped one, the batch's largest uncapped degree; for a symmetric one the host array of frame sizes too -- and `e` /
    `edge_ptr_g` are what its count read back, set by _edges_launch."""
    __slots__ = ("staged", "layout", "n", "g", "e", "mode", "sel", "max_deg", "sizes", "edge_ptr_g")

    def __init__(self, staged, layout, e, mode, sel, max_deg=0, sizes=None):
        self.staged, self.layout, self.n, self.g, self.e, self.mode = staged, layout, layout.n, layout.g, e, mode
        self.sel, self.max_deg, self.sizes, self.edge_ptr_g = sel, max_deg, sizes, None


_readback = {}   # device index -> (pinned int32 buffer, event) of the symmetric build's one read-back


def _sym_edges_launch(job, reid_embeds):
    """The symmetric capped build on the current stream: gnncca_build_edges_topk_sym_count, ONE pinned device-to-host copy of the G + 1
    per-frame edge offsets (the last is E) queued behind it and waited on through an event -- the call's only host wait -- then the
    outputs are allocated and gnncca_build_edges_topk_sym_emit fills them.  Sets job.e and job.edge_ptr_g (host list)."""
    dev, n, g = reid_embeds.device, job.n, job.g
    lib = nat.lib()
    fr = job.layout.frames(job.staged.data_ptr())
    sizes = job.sizes
    nbytes = lib.gnncca_build_edges_topk_sym_bytes(sizes.ctypes.data, g)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    eptr_g = job.layout.view(job.staged, "edge_ptr_g")
    st = lib.gnncca_build_edges_topk_sym_count(C.byref(fr), reid_embeds.data_ptr(), reid_embeds.shape[1], n, sizes.ctypes.data, g, job.sel.top_k,
                                               job.sel.rank, job.max_deg, job.sel.sym, ws.data_ptr(), nbytes, eptr_g.data_ptr(), _raw_stream(dev))
    if st:
        nat.check(st, "gnncca_build_edges_topk_sym_count")
    hit = _readback.get(dev.index)
    if hit is None or hit[0].numel() < g + 1:
        hit = _readback[dev.index] = (torch.empty(max(2 * (g + 1), 256), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
    host, event = hit
    host[:g + 1].copy_(eptr_g, non_blocking=True)
    event.record(_current_stream(dev))
    event.synchronize()
    job.edge_ptr_g = host[:g + 1].tolist()
    e = job.e = job.edge_ptr_g[-1]
    if e >= 2 ** 31 - 64:
        raise NotImplementedError("more than 2^31 edges in one batch")
    n_attr = 4 if job.mode == MODE_FULL else 2
    edge_index = torch.empty((2, e), dtype=torch.int64, device=dev)
    edge_attr = torch.empty((e, n_attr), dtype=torch.float32, device=dev)
    edge_labels = torch.empty(e, dtype=torch.float32, device=dev)
    st = lib.gnncca_build_edges_topk_sym_emit(C.byref(fr), reid_embeds.data_ptr(), reid_embeds.shape[1], n, sizes.ctypes.data, g, e, job.mode,
                                              ws.data_ptr(), nbytes, edge_index.data_ptr(), edge_attr.data_ptr(), edge_labels.data_ptr(),
                                              _raw_stream(dev))
    if st:
        nat.check(st, "gnncca_build_edges_topk_sym_emit")
    return edge_index, edge_attr, edge_labels


def _edges_launch(job, reid_embeds):
    """The build of job.sel on the current stream -- gnncca_build_edges, _topk or _radius (Selection.launch), or the two ..._topk_sym_*
    calls for a symmetric one: (edge_index, edge_attr, edge_labels), new tensors."""
    sel = job.sel
    if sel.sym:
        return _sym_edges_launch(job, reid_embeds)
    dev, n, e = reid_embeds.device, job.n, job.e
    n_attr = 4 if job.mode == MODE_FULL else 2
    fr = job.layout.frames(job.staged.data_ptr())
    edge_index = torch.empty((2, e), dtype=torch.int64, device=dev)
    edge_attr = torch.empty((e, n_attr), dtype=torch.float32, device=dev)
    edge_labels = torch.empty(e, dtype=torch.float32, device=dev)
    # (a capped or gated build is called with E == 0 too: its entry point checks its arguments, the degree limit among them, before it looks
    # at the sizes, and launches nothing then)
    if e > 0 or sel.pruned:
        sel.launch(nat.lib(), "gnncca_build_edges", (C.byref(fr), reid_embeds.data_ptr(), reid_embeds.shape[1], n, e, job.mode), job.max_deg,
                   (edge_index.data_ptr(), edge_attr.data_ptr(), edge_labels.data_ptr(), _raw_stream(dev)))
    return edge_index, edge_attr, edge_labels


class _GraphBuildFunction(torch.autograd.Function):
    """Autograd bridge of build_graph_batch (the reference's statements are torch ops: F.normalize(dim=0), gathers, F.pairwise_distance,
    F.cosine_similarity -- train.py:257-259, 306-308, 344, 357; with the no_grad around its CNN removed, the association loss reaches
    the raw embeddings through them).  forward(node_raw | None, reid, job): with node_raw the embeddings are normalised here and the
    outputs are (x, edge_attr, reid_normalised, edge_index, edge_labels); with None (normalize=False) `reid` is used as given and the
    outputs are (edge_attr, edge_index, edge_labels).  backward: gnncca_build_edges_backward (gnncca_build_edges_topk_backward for a
    capped or radius-gated build: the selection is piecewise constant, the gradient flows through the kept edges; that entry serves any
    subsequence of the dense list whose runs ascend in the destination) on grad_edge_attr, plus whatever arrives
    on the normalised reid table directly, then gnncca_normalize_columns_backward per matrix; an input that does not require grad
    costs no launch and no allocation.  The ground-plane attributes, edge_index and edge_labels carry no gradient.  Differentiable
    once (double backward raises torch's error)."""

    @staticmethod
    def forward(ctx, node_raw, reid, job):
        ctx.job, ctx.normalized = job, node_raw is not None
        ctx.set_materialize_grads(False)   # an output nobody used arrives as None, not as a zero matrix
        if ctx.normalized:
            reid_n, x = _normalize_launch(reid, node_raw)
        else:
            reid_n, x = reid, None
        edge_index, edge_attr, edge_labels = _edges_launch(job, reid_n)
        ctx.mark_non_differentiable(edge_index, edge_labels)
        pruned = (edge_index,) if job.sel.pruned else ()   # the capped / gated backward looks its edges up in the forward's edge list
        if ctx.normalized:
            ctx.save_for_backward(node_raw, reid, reid_n, edge_attr, *pruned)
            return x, edge_attr, reid_n, edge_index, edge_labels
        ctx.save_for_backward(reid, edge_attr, *pruned)
        return edge_attr, edge_index, edge_labels

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        job = ctx.job
        saved = ctx.saved_tensors
        edge_index = saved[-1] if job.sel.pruned else None
        if ctx.normalized:
            node_raw, reid_raw, reid_n, edge_attr = saved[:4]
            g_x, g_ea, g_reid = grads[0], grads[1], grads[2]
        else:
            reid_n, edge_attr = saved[:2]
            node_raw = reid_raw = g_x = g_reid = None
            g_ea = grads[0]
        want_node, want_reid = ctx.needs_input_grad[0] and g_x is not None, ctx.needs_input_grad[1]
        d_rn = None   # d loss / d (the reid table the edge kernel read)
        if want_reid:
            if g_ea is not None and job.e == 0 and job.mode != MODE_ONLY_DIST:
                d_rn = torch.zeros_like(reid_n)   # no edge: what torch's empty gathers give, and nothing to launch
            elif g_ea is not None and job.mode != MODE_ONLY_DIST:
                dev = reid_n.device
                lib = nat.lib()
                g_ea = g_ea if g_ea.dtype == torch.float32 and g_ea.is_contiguous() else g_ea.float().contiguous()
                d_rn = torch.empty_like(reid_n)
                nbytes = lib.gnncca_build_edges_backward_bytes(job.n)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                fr = job.layout.frames(job.staged.data_ptr())
                with _on(dev):
                    if edge_index is not None:
                        st = lib.gnncca_build_edges_topk_backward(C.byref(fr), reid_n.data_ptr(), reid_n.shape[1], job.n, job.e, job.mode,
                                                                  edge_index.data_ptr(), edge_attr.data_ptr(), g_ea.data_ptr(), ws.data_ptr(),
                                                                  nbytes, d_rn.data_ptr(), _raw_stream(dev))
                    else:
                        st = lib.gnncca_build_edges_backward(C.byref(fr), reid_n.data_ptr(), reid_n.shape[1], job.n, job.e, job.mode,
                                                             edge_attr.data_ptr(), g_ea.data_ptr(), ws.data_ptr(), nbytes, d_rn.data_ptr(),
                                                             _raw_stream(dev))
                if st:
                    nat.check(st, "gnncca_build_edges_backward")
            if g_reid is not None:   # a gradient on batch.reid_embeds itself (the caller's own ReID loss)
                d_rn = g_reid if d_rn is None else d_rn.add_(g_reid)
        if not ctx.normalized:
            return None, d_rn, None
        jobs = ([(1, reid_raw, d_rn)] if d_rn is not None else []) + ([(0, node_raw, g_x)] if want_node else [])
        res = [None, None, None]
        if jobs:
            for (k, _, _), gx in zip(jobs, _normalize_backward_launch([(x, g) for _, x, g in jobs])):
                res[k] = gx
        return tuple(res)


def build_graph_batch(xw, yw, ids, id_cam, graph_sizes, max_dist, node_embeds, reid_embeds, only_appearance=False,
                      only_dist=False, normalize=True, top_k=None, rank_by="ground", symmetric=None, radius=None, radius_unit="ground"):
    """One call per batch of frames.  Host inputs (numpy, one entry per detection, frames concatenated): xw, yw, ids,
    id_cam; graph_sizes / max_dist per frame.  Device inputs: node_embeds [N, D], reid_embeds [N, R].
    Returns a GraphBatch (x, edge_index, edge_attr) with .edge_labels and .y, laid out exactly like the reference's
    `Batch.from_data_list(batch)` (inference.py:279).
    Host work: one native call that enumerates the edges (gnncca_plan_frames, include/gnncca_mpn.h) into a pinned staging buffer,
    one non-blocking upload, four launches; the call never synchronises.

    top_k=None (the default) builds the reference's complete cross-camera graph.  top_k=k (an integer >= 1; no counterpart in the reference)
    keeps, for every detection i, the min(k, deg_i) of its deg_i cross-camera candidates in its own frame with the smallest key, ties to the
    smaller destination node id.  rank_by='ground': the ground-plane L2 distance in float64 (before the division by max_dist);
    rank_by='reid': the F.pairwise_distance value of the (normalised) reid rows, the fp32 number that goes into edge_attr.  The key need
    not be an emitted attribute ('reid' with only_dist and 'ground' with only_appearance are legal).  The kept edges stay in the dense
    order, so the result is a subsequence of the dense edge list -- for k >= max deg the dense build, bit for bit -- with
    E = sum_i min(k, deg_i) known on the host (gnncca_plan_frames_ex): still no synchronisation.  edge_ptr, node_ptr, their device copies,
    edge_labels and y keep their meaning.
    The capped graph is DIRECTED: i may keep j while j does not keep i.  postprocess' remove_edges_single_direction therefore keeps
    mutual pairs only, and a kept edge without its reverse can never become an association (symmetric= below closes the list).
    At most 4096 candidates per source (NotImplementedError beyond).  Differentiable like the dense build: gradients flow through the
    kept edges' emb / cos attributes.

    symmetric=None (the default) is that directed list D, down to the native call.  symmetric='union' keeps the dense edge (i, j) iff
    (i, j) or (j, i) is in D, symmetric='mutual' iff both are (no counterpart in the reference either: it only builds complete graphs,
    every pair in both directions, and its pruning deletes an active edge without an active reverse).  Whether i is in j's list is j's
    own selection, made with the key bits j ranks with ('reid' keys are not symmetric: F.pairwise_distance adds its eps to a - b); no key
    is evaluated from two sides.  The result is a subsequence of the dense edge list in dense order, a kept edge carries the dense
    build's bits (attributes, label, ids), it is closed under reversal, mutual <= D <= union, and for k >= max deg both modes are the
    dense build, bit for bit (edge_index, edge_attr, edge_labels, x, y, edge_ptr, node_ptr and the device copies).  edge_ptr,
    edge_ptr_dev, node_ptr, edge_labels and y keep their meaning; a frame or a source may end with no edge, and E = 0 is legal.  The
    limit of 4096 candidates per source stays (NotImplementedError before any launch), and the build stays differentiable.
    symmetric without top_k, or an unknown value, is a ValueError raised before the GPU is touched.
    E now depends on the data, so a symmetric build SYNCHRONISES ONCE: one small pinned device-to-host copy carries the G + 1 per-frame
    edge offsets (the last one is E), queued behind the count launches and waited on through an event; there is no other host wait.
    Under stream capture it raises RuntimeError before anything is launched.  The directed build (symmetric=None) still never waits.

    radius=None (the default) is the code above, down to the native call.  radius=r keeps the dense edge (i, j) of frame g iff the two
    detections are within r on the ground plane (no counterpart in the reference's graph build).  The definition (include/gnncca_mpn.h):
    s = dx*dx + dy*dy with dx = xw[i] - xw[j], dy = yw[i] - yw[j] -- two products and one sum, each rounded once in float64, no FMA;
    t_g = r for radius_unit='ground' (the units of xw / yw, before the division by max_dist), t_g = r * max_dist[g] (one rounded product)
    for radius_unit='max_dist' (mixed-data-set batches; a gate in the units of edge_attr[:, 0]); t2_g = t_g * t_g; kept iff s <= t2_g.
    The test is on the squared distance: s(i, j) == s(j, i) bit for bit, so the list is CLOSED UNDER REVERSAL by construction, and the
    host plan (gnncca_plan_frames_radius) evaluates the identical IEEE sequence, so E is known before any launch: no wait, no closure
    pass, capturable.  A NaN compares false (a pair with a NaN position is dropped); radius=inf keeps every pair without a NaN and is, on
    NaN-free positions, the dense build bit for bit (edge_index, edge_attr, edge_labels, x, y, edge_ptr, node_ptr and the device copies).
    The result is a subsequence of the dense list in dense order, a kept edge carries the dense build's bits, the reid rows are read for
    the kept candidates only, and a source, a frame or the whole batch may end with no edge (E = 0 is legal).  Differentiable like the
    capped build.  radius must be a finite number >= 0 or inf; a bool, NaN, negative or non-number, an unknown radius_unit, and radius
    together with top_k or symmetric (a gated k-nearest list is not defined here yet) are ValueErrors raised before the GPU is touched.
    The host plan evaluates every unordered pair of a frame once: O(sum n_g^2 / 2) host work per batch."""
    sel = select(top_k, rank_by, symmetric, radius, radius_unit)
    if not (node_embeds.is_cuda and reid_embeds.is_cuda):
        raise RuntimeError("gnn_cca_amd.graph_build runs on MI355X only (no CPU fallback)")
    dev = reid_embeds.device
    frames = StagedFrames(xw, yw, ids, id_cam, graph_sizes, max_dist)
    if reid_embeds.shape[0] != frames.n or node_embeds.shape[0] != frames.n:
        raise RuntimeError("embeddings and detections disagree on the number of nodes")
    if symmetric is not None and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("build_graph_batch(symmetric=...) waits for its edge count and cannot be captured into a graph")
    frames.plan(dev, sel)
    mode = MODE_ONLY_APPEARANCE if only_appearance else (MODE_ONLY_DIST if only_dist else MODE_FULL)
    with _on(dev):
        staged = torch.empty(frames.layout.nbytes, dtype=torch.uint8, device=dev)
        frames.upload(staged)
        job = _EdgeJob(staged, frames.layout, frames.e, mode, sel, frames.max_deg, frames.arrays[4])
        if _wants_grad(node_embeds, reid_embeds):
            # the differentiable build: x, edge_attr and reid_embeds are outputs of ONE autograd node (see _GraphBuildFunction)
            reid_embeds = _f32c(reid_embeds)
            if normalize:
                node_embeds, edge_attr, reid_embeds, edge_index, edge_labels = _GraphBuildFunction.apply(_f32c(node_embeds), reid_embeds, job)
            else:   # x and reid_embeds are the caller's tensors: their history is torch's own
                edge_attr, edge_index, edge_labels = _GraphBuildFunction.apply(None, reid_embeds, job)
        else:
            if normalize:
                reid_embeds, node_embeds = normalize_columns(reid_embeds, node_embeds)
            elif reid_embeds.dtype != torch.float32 or not reid_embeds.is_contiguous():
                reid_embeds = reid_embeds.float().contiguous()
            edge_index, edge_attr, edge_labels = _edges_launch(job, reid_embeds)
    node_ptr, edge_ptr = frames.layout.host_ptrs(frames.pinned)
    # (a symmetric build: the offsets its count read back; the device image holds the same, the pinned one still the plan's)
    batch = GraphBatch(node_embeds, edge_index, edge_attr, job.edge_ptr_g if sel.sym else edge_ptr, node_ptr)
    attach(batch, staged, frames.layout, frames.arrays[3])
    batch.edge_labels = edge_labels
    batch.reid_embeds = reid_embeds
    return batch
