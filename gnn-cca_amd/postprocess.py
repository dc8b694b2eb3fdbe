"""Row N2 of SURVEY.md 8f: the step right after the MPN on the GPU.

`threshold` = inference.py:286-291 (sigmoid, >= 0.5); `prune_and_cluster` = utils.remove_edges_single_direction
(libs/utils.py:387-404) + the flow counts of utils.compute_rounding (libs/utils.py:54-59) + the clusters
utils.compute_SCC_and_Clusters (libs/utils.py:295-317) returns for the pruned edge set -- without the networkx /
Python-list round trips through the host -- and, per frame, the two TRIGGER bits of the reference's bridge-based heuristics
(a node with flow > 3: utils.compute_rounding has work to do, libs/utils.py:58-62; a cluster with more than four members:
utils.disjoint_big_clusters has, libs/utils.py:321-322).  `finalize` runs those heuristics, in the order of the shipped
configuration (config_inference.yaml:6-8 ROUNDING / PRUNING / SPLITTING = True; inference.py:306-345), for the frames that
raised a bit: native host code (csrc/post_host.cpp; SURVEY.md 8f keeps the bridge searches on the CPU), one frame at a time
as the reference does.  A frame with no bit set already has its final partition.

`strong_clusters` is PRUNING = False (config_inference.yaml:7): nothing is pruned and the clusters are the strongly connected components
of the active edges (inference.py:302-304), one memset and one launch (csrc/strong.cuh); `finalize(..., pruning=False)` runs the host
heuristics on that result without the pruning switch.

`exclusive_clusters` has no counterpart in the reference: a partition in which no cluster holds two detections of one camera, for any
number of cameras, computed on the device without a wait (csrc/exclusive.cuh).
"""
import ctypes as C
import numbers

import numpy as np
import torch

from . import _native as nat


from .frames import _on, _raw_stream as _stream   # the lean device guard / raw stream handle (host time matters here: ~6 launches)


def check_threshold(at):
    """A decision threshold on a probability: a real number strictly between 0 and 1 -> float (ValueError otherwise)."""
    if isinstance(at, bool) or not isinstance(at, numbers.Real):
        raise ValueError(f"the threshold must be a real number in (0, 1), not {at!r}")
    th = float(at)
    if not 0.0 < th < 1.0:
        raise ValueError(f"the threshold must lie strictly between 0 and 1, not {at!r}")
    return th


NO_CPU = "gnn_cca_amd.postprocess runs on MI355X only (no CPU fallback)"


def _edge_index_i64(edge_index):
    """edge_index as a contiguous int64 tensor: itself where it already is one."""
    return edge_index if edge_index.dtype == torch.int64 and edge_index.is_contiguous() else edge_index.long().contiguous()


def _flat(t, dtype):
    """t flattened to a contiguous tensor of `dtype`: a view of itself where it already is one."""
    t = t.reshape(-1)
    return t if t.dtype == dtype and t.is_contiguous() else t.to(dtype).contiguous()


def _int32_on(v, dev):
    """A tensor or a host sequence of integers (numpy's included) as a contiguous int32 tensor on `dev`: itself where it already is one.
    (evaluation._dev_i32 is the batch-level cousin: tensors only, and it trusts the device of a tensor that is already int32.)"""
    if torch.is_tensor(v):
        if v.dtype == torch.int32 and v.device == dev and v.is_contiguous():
            return v
        return v.to(device=dev, dtype=torch.int32).contiguous()
    return torch.tensor([int(q) for q in v], dtype=torch.int32).to(dev)


def threshold(logits, at=0.5):
    """logits: Tensor[E] or [E,1] on the GPU -> (probs float32 [E], predictions int64 [E]): probs = sigmoid(logits), predictions =
    (probs >= at).  at=0.5 is the reference's threshold (inference.py:286-291) and the launch this function has always made; any other
    value in (0, 1) -- one chosen with calibration.sweep_thresholds -- is compared in float64 against the widened float32 probability."""
    at = check_threshold(at)
    if not logits.is_cuda:
        raise RuntimeError(NO_CPU)
    x = _flat(logits, torch.float32)
    probs = torch.empty_like(x)
    preds = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    with _on(x.device):
        if at == 0.5:
            st = nat.lib().gnncca_post_threshold(x.data_ptr(), x.shape[0], probs.data_ptr(), preds.data_ptr(), _stream(x.device))
        else:
            st = nat.lib().gnncca_post_threshold_at(x.data_ptr(), x.shape[0], at, probs.data_ptr(), preds.data_ptr(), _stream(x.device))
    if st:
        nat.check(st, "gnncca_post_threshold")
    return probs, preds


def prune_and_cluster(edge_index, predictions, n_nodes, node_ptr=None, edge_ptr=None):
    """-> dict(pruned int64 [E], flow_out / flow_in int32 [N], labels int32 [N] (smallest node id of the component),
    n_clusters int32 [1] on the device).

    `node_ptr` / `edge_ptr` (optional, both or neither): the frame ranges of a batch laid out like
    Batch.from_data_list -- sequences of G + 1 ints or int32 device tensors (GraphBatch.node_ptr / .edge_ptr, or the
    device copies build_graph_batch keeps).  With them every frame is clustered by its own workgroup."""
    if not (edge_index.is_cuda and predictions.is_cuda):
        raise RuntimeError(NO_CPU)
    dev = edge_index.device
    ei, pred = _edge_index_i64(edge_index), _flat(predictions, torch.int64)
    e = ei.shape[1]
    lib = nat.lib()
    ws = torch.empty(lib.gnncca_post_workspace_bytes(n_nodes, e) + 256, dtype=torch.uint8, device=dev)
    if (node_ptr is None) != (edge_ptr is None):
        raise ValueError("node_ptr and edge_ptr go together")
    n_trig = (len(node_ptr) if not torch.is_tensor(node_ptr) else node_ptr.numel()) - 1 if node_ptr is not None else 1
    # flow_out | flow_in | n_clusters | cluster sizes (scratch) | triggers: zeroed by ONE memset
    counters = torch.empty(3 * n_nodes + 1 + max(n_trig, 1), dtype=torch.int32, device=dev)
    out = {"pruned": torch.empty(e, dtype=torch.int64, device=dev),
           "flow_out": counters[:n_nodes], "flow_in": counters[n_nodes:2 * n_nodes],
           "labels": torch.empty(n_nodes, dtype=torch.int32, device=dev),
           "n_clusters": counters[2 * n_nodes:2 * n_nodes + 1],
           "triggers": counters[3 * n_nodes + 1:3 * n_nodes + 1 + max(n_trig, 1)]}
    n_frames, np_dev, ep_dev = 0, None, None
    if node_ptr is not None:   # (the offsets' VALUES are not judged here, unlike in _frame_ranges: deliberate -- the benchmark's host-bound leg)
        np_dev, ep_dev = _int32_on(node_ptr, dev), _int32_on(edge_ptr, dev)
        n_frames = np_dev.numel() - 1
        if ep_dev.numel() != n_frames + 1 or n_frames < 1:
            raise ValueError("node_ptr / edge_ptr must both have G + 1 entries")
    with _on(dev):
        cp = counters.data_ptr()
        st = lib.gnncca_post_prune_cluster_frames_ex(ei.data_ptr(), pred.data_ptr(), n_nodes, e,
                                                     np_dev.data_ptr() if np_dev is not None else None,
                                                     ep_dev.data_ptr() if ep_dev is not None else None, n_frames,
                                                     ws.data_ptr(), ws.numel(), out["pruned"].data_ptr(),
                                                     cp, cp + 4 * n_nodes, out["labels"].data_ptr(), cp + 8 * n_nodes,
                                                     cp + 8 * n_nodes + 4, cp + 12 * n_nodes + 4, _stream(dev))
    if st:
        nat.check(st, "gnncca_post_prune_cluster")
    out["_workspace"] = (ws, np_dev, ep_dev)
    return out


MAX_FRAME_NODES = nat.EXCLUSIVE_MAX_FRAME_NODES
MAX_CAMERAS = nat.EXCLUSIVE_MAX_CAMERAS


def check_cameras(cam):
    """HOST camera ids (any integer sequence or array) must lie in [0, 64) for exclusive_clusters: a cluster's cameras are one 64-bit
    mask.  ValueError otherwise; nothing is launched."""
    cam = np.asarray(cam)
    if cam.size and (cam.dtype.kind not in "iu" or int(cam.min()) < 0 or int(cam.max()) >= MAX_CAMERAS):
        raise ValueError(f"camera ids must be integers in [0, {MAX_CAMERAS}) for the camera-exclusive clusters "
                         f"(found {cam.min()!r} .. {cam.max()!r})")


def _host_ptr(v, name):
    """A frame-offset sequence as a host int64 array, or None for a device tensor (whose values are not read: no synchronisation)."""
    if torch.is_tensor(v):
        if v.is_cuda:
            return None
        v = v.numpy()
    a = np.asarray(v)
    if a.ndim != 1 or a.size < 2 or a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold G + 1 integer offsets")
    return a.astype(np.int64)


def widest_frame(node_ptr):
    """The detections of the widest frame of HOST offsets (G + 1 ints; 0 without a frame)."""
    sizes = np.diff(np.asarray(node_ptr, dtype=np.int64))
    return int(sizes.max()) if sizes.size else 0


def _frame_ranges(node_ptr, edge_ptr, n_nodes, e, limit, who, max_frame_nodes):
    """The frame ranges of exclusive_clusters / strong_clusters (`who`, for the messages) -> (g, max_frame_nodes), or a ValueError: both
    must have G + 1 entries, G >= 1; HOST offsets must ascend from 0 to n_nodes / E and no frame may be wider than `limit` (the values of a
    device tensor are not read: no synchronisation -- the kernel flags such a frame).  max_frame_nodes: the caller's, else the widest
    frame where the host knows it, else min(n_nodes, limit); in [0, limit], clamped to n_nodes.  node_ptr None (strong_clusters): the
    whole graph is the one frame, g = 0, and n_nodes itself must fit.  prune_and_cluster, on the benchmark's host-bound step-by-step leg,
    makes none of these checks and never has."""
    g = 0
    if node_ptr is not None:
        np_h, ep_h = _host_ptr(node_ptr, "node_ptr"), _host_ptr(edge_ptr, "edge_ptr")
        g = (np_h.size if np_h is not None else node_ptr.numel()) - 1
        if (ep_h.size if ep_h is not None else edge_ptr.numel()) != g + 1 or g < 1:
            raise ValueError("node_ptr / edge_ptr must both have G + 1 entries")
        if np_h is not None:
            if int(np_h[0]) != 0 or int(np_h[-1]) != n_nodes or (np.diff(np_h) < 0).any():
                raise ValueError("node_ptr must ascend from 0 to n_nodes")
            widest = widest_frame(np_h)
            if widest > limit:
                raise ValueError(f"a frame has {widest} detections; {who} takes frames of at most {limit}")
            max_frame_nodes = widest if max_frame_nodes is None else max_frame_nodes
        if ep_h is not None and (int(ep_h[0]) != 0 or int(ep_h[-1]) != e or (np.diff(ep_h) < 0).any()):
            raise ValueError("edge_ptr must ascend from 0 to E")
    elif n_nodes > limit:
        raise ValueError(f"the graph has {n_nodes} detections; {who} takes frames of at most {limit} "
                         "(pass node_ptr / edge_ptr for a batch of frames)")
    if max_frame_nodes is None:
        max_frame_nodes = min(n_nodes, limit)
    max_frame_nodes = int(max_frame_nodes)
    if not 0 <= max_frame_nodes <= limit:
        raise ValueError(f"max_frame_nodes must lie in [0, {limit}], not {max_frame_nodes}")
    return g, min(max_frame_nodes, n_nodes)


def exclusive_clusters(edge_index, probs, cam, n_nodes, node_ptr, edge_ptr, at=0.5, max_frame_nodes=None):
    """Camera-exclusive identity clusters: a partition of every frame in which no cluster holds two detections of one camera, for any
    number of cameras, on the device and without a synchronisation (csrc/exclusive.cuh; no counterpart in the reference).  The rule
    (include/gnncca_mpn.h has it in full, tests/exclusive_oracle.py in numpy): an edge is active iff float64(probs[k]) >= at; a pair
    {i, j} is a candidate iff both of its edges exist in the frame and are active (the pruning rule); its weight is the smaller of the two
    probabilities; candidates are walked by descending weight (ties: smaller min(i, j), then smaller max) and a candidate's two clusters
    merge iff they differ and share no camera.  Where a frame's plain connected components are already legal the result is
    prune_and_cluster's, exactly.

    edge_index int64 [2, E], probs float32 [E] or [E, 1], cam int32 [N] camera ids in [0, 64): device tensors.  node_ptr / edge_ptr: the
    frame ranges as prune_and_cluster takes them (sequences of G + 1 ints, or int32 device tensors).  With device tensors the largest
    frame is not known on the host: pass max_frame_nodes (default: min(n_nodes, 4096), which sizes the kernel's LDS for the worst case).

    -> dict(predictions int64 [E]: 1 iff the edge belongs to a candidate pair inside one cluster; labels int32 [N]: the smallest node
    id of the node's cluster; n_clusters int32 [1]; cut int32 [G]: candidate pairs of the frame that ended up between two clusters;
    flags uint32-valued int32 [G]: 0, 1 = a camera id outside [0, 64) reached the device, 2 = the frame's ranges do not fit -- every node
    of such a frame is its own cluster with predictions 0), all on the device.  ValueError before any launch: a threshold outside (0, 1),
    mismatched lengths, a frame of more than 4096 detections (where the host knows the sizes)."""
    at = check_threshold(at)
    if node_ptr is None or edge_ptr is None:
        raise ValueError("exclusive_clusters works frame by frame: node_ptr and edge_ptr are required")
    n_nodes = int(n_nodes)
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], not {tuple(edge_index.shape)}")
    e = int(edge_index.shape[1])
    if probs.numel() != e:
        raise ValueError(f"probs [{probs.numel()}] does not match edge_index (E={e})")
    if cam.numel() != n_nodes:
        raise ValueError(f"cam [{cam.numel()}] does not match n_nodes ({n_nodes})")
    if not cam.is_cuda:   # a host array can be judged here (the batch-level entry points do; a device tensor is judged by the kernel)
        check_cameras(cam.numpy())
    g, max_frame_nodes = _frame_ranges(node_ptr, edge_ptr, n_nodes, e, MAX_FRAME_NODES, "exclusive_clusters", max_frame_nodes)
    if not (edge_index.is_cuda and probs.is_cuda and cam.is_cuda):
        raise RuntimeError(NO_CPU)
    dev = edge_index.device
    lib = nat.lib()
    with _on(dev):
        ei, pr = _edge_index_i64(edge_index), _flat(probs, torch.float32)
        cm, np_dev, ep_dev = _int32_on(cam, dev), _int32_on(node_ptr, dev), _int32_on(edge_ptr, dev)
        ws_bytes = lib.gnncca_post_exclusive_workspace_bytes(n_nodes, e, g)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        preds = torch.empty(e, dtype=torch.int64, device=dev)
        ints = torch.empty(n_nodes + 1 + 2 * g, dtype=torch.int32, device=dev)   # labels | n_clusters | cut | flags
        ip = ints.data_ptr()
        st = lib.gnncca_post_exclusive_frames(ei.data_ptr() if e else None, pr.data_ptr() if e else None, n_nodes, e,
                                              cm.data_ptr() if n_nodes else None, np_dev.data_ptr(), ep_dev.data_ptr(), g, max_frame_nodes, at,
                                              preds.data_ptr() if e else None, ip if n_nodes else None, ip + 4 * n_nodes, ip + 4 * (n_nodes + 1),
                                              ip + 4 * (n_nodes + 1 + g), ws.data_ptr(), ws_bytes, _stream(dev))
    if st:
        nat.check(st, "gnncca_post_exclusive_frames")
    # (the workspace is freed by the caching allocator in stream order: nothing to keep)
    return {"predictions": preds, "labels": ints[:n_nodes], "n_clusters": ints[n_nodes:n_nodes + 1],
            "cut": ints[n_nodes + 1:n_nodes + 1 + g], "flags": ints[n_nodes + 1 + g:]}


STRONG_MAX_FRAME_NODES = nat.STRONG_MAX_FRAME_NODES

NO_SPLITTING_WITHOUT_PRUNING = ("SPLITTING = True needs PRUNING = True: the reference itself has no behaviour there -- disjoint_big_clusters "
                                "(libs/utils.py:319-386) looks up the reverse of every edge it removes, and on unpruned predictions that "
                                "reverse need not be active (inference.py:339-345 then ends in 'ValueError: ... is not in list')")


def strong_clusters(edge_index, predictions, n_nodes, node_ptr=None, edge_ptr=None, max_frame_nodes=None):
    """Identity clusters WITHOUT pruning: the strongly connected components of every frame's active edges, which is what
    utils.compute_SCC_and_Clusters (libs/utils.py:295-317) returns under PRUNING = False (inference.py:302-304, 733-738, 904-908) -- a
    directed cycle without a mutual pair is one identity -- on the device and without a synchronisation (csrc/strong.cuh; include/gnncca_mpn.h
    has the rule in full).  One memset and one launch: no graph plan, no workspace.  On a directed capped list (top_k=) these are the
    reference's own clusters, with no closure and no wait.  On symmetric predictions the result is prune_and_cluster's exactly.

    edge_index int64 [2, E], predictions [E] or [E, 1] (1 = active): device tensors.  node_ptr / edge_ptr (both or neither): the frame
    ranges as prune_and_cluster takes them (sequences of G + 1 ints, or int32 device tensors); without them the whole graph is one frame.
    With device tensors the largest frame is not known on the host: pass max_frame_nodes (default: min(n_nodes, 1024), which sizes the
    kernel's LDS for the worst case, 128 KiB).

    -> dict(predictions int64 [E]: the input, contiguous -- nothing is pruned; flow_out / flow_in int32 [N]: active edges leaving / entering
    each node; labels int32 [N]: the smallest node id of the node's component; n_clusters int32 [1]; triggers int32 [G]: bit 0 = a node with
    a flow above 3, bit 1 = a component of more than four members (prune_and_cluster's bits); flags uint32-valued int32 [G]: 0, or 2 = the
    frame's ranges do not fit -- every node of such a frame is its own cluster with flows and triggers 0), all on the device.  ValueError
    before any launch: mismatched lengths, offsets that do not ascend from 0 to N / E, a frame of more than 1024 detections (where the host
    knows the sizes)."""
    if (node_ptr is None) != (edge_ptr is None):
        raise ValueError("node_ptr and edge_ptr go together")
    n_nodes = int(n_nodes)
    if n_nodes < 0:
        raise ValueError(f"n_nodes must not be negative, not {n_nodes}")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], not {tuple(edge_index.shape)}")
    e = int(edge_index.shape[1])
    if predictions.numel() != e:
        raise ValueError(f"predictions [{predictions.numel()}] does not match edge_index (E={e})")
    g, max_frame_nodes = _frame_ranges(node_ptr, edge_ptr, n_nodes, e, STRONG_MAX_FRAME_NODES, "strong_clusters", max_frame_nodes)
    if not (edge_index.is_cuda and predictions.is_cuda):
        raise RuntimeError(NO_CPU)
    dev = edge_index.device
    lib = nat.lib()
    with _on(dev):
        ei, pred = _edge_index_i64(edge_index), _flat(predictions, torch.int64)
        np_dev, ep_dev = (_int32_on(node_ptr, dev), _int32_on(edge_ptr, dev)) if g else (None, None)
        n_trig = max(g, 1)
        # flow_out | flow_in | n_clusters (zeroed by ONE memset) | labels | triggers | flags
        ints = torch.empty(3 * n_nodes + 1 + 2 * n_trig, dtype=torch.int32, device=dev)
        ip = ints.data_ptr()
        o_lab, o_trig = 2 * n_nodes + 1, 3 * n_nodes + 1
        st = lib.gnncca_post_strong_frames(ei.data_ptr() if e else None, pred.data_ptr() if e else None, n_nodes, e,
                                           np_dev.data_ptr() if g else None, ep_dev.data_ptr() if g else None, g, max_frame_nodes,
                                           ip, ip + 4 * n_nodes, ip + 4 * o_lab, ip + 8 * n_nodes, ip + 4 * o_trig, ip + 4 * (o_trig + n_trig),
                                           _stream(dev))
    if st:
        nat.check(st, "gnncca_post_strong_frames")
    return {"predictions": pred, "flow_out": ints[:n_nodes], "flow_in": ints[n_nodes:2 * n_nodes], "labels": ints[o_lab:o_lab + n_nodes],
            "n_clusters": ints[2 * n_nodes:2 * n_nodes + 1], "triggers": ints[o_trig:o_trig + n_trig], "flags": ints[o_trig + n_trig:],
            "_keep": (ei, np_dev, ep_dev)}


def finalize(edge_index, probs, pruned, labels, n_clusters, triggers, node_ptr=None, edge_ptr=None, rounding=True, pruning=True,
             splitting=True):
    """The reference's FINAL predictions and identity clusters under the three switches of config_inference.yaml:6-8 (inference.py:306-345:
    PRUNING -> ROUNDING -> PRUNING -> SPLITTING), from what `threshold` + `prune_and_cluster` left on the device.

    `triggers` [G] (prune_and_cluster's) says which frames the heuristics can change; this call SYNCHRONISES to read it.  Frames with no
    bit set keep the device chain's result -- it is final for them.  For the others the frame's edges, probabilities and pruned predictions
    are copied to the host, `gnncca_post_finalize_frame_host` (csrc/post_host.cpp: utils.compute_rounding, remove_edges_single_direction,
    disjoint_big_clusters, compute_SCC_and_Clusters with the reference's artefacts) runs frame by frame, and the patched tensors go back.
    `node_ptr` / `edge_ptr`: HOST sequences of G + 1 ints (GraphBatch.node_ptr / .edge_ptr); None = the whole graph is one frame.

    -> dict(predictions int64 [E], labels int32 [N], n_clusters int32 [1] on the device, frames_finalized: list of frame ids,
            triggers: host int32 [G]).

    `pruning=False` (PRUNING: False): `pruned` is then the THRESHOLDED predictions and labels / n_clusters / triggers are those of
    `strong_clusters` on them (the strongly connected components of the unpruned edges, inference.py:302-304); the host pass gets the
    switches without the pruning, so only ROUNDING can change a frame (inference.py:316-329 on unpruned predictions).  `pruning=False` with
    `splitting=True` is a ValueError: the reference has no behaviour there (NO_SPLITTING_WITHOUT_PRUNING)."""
    if not pruning and splitting:
        raise ValueError(NO_SPLITTING_WITHOUT_PRUNING)
    trig = triggers.cpu().numpy()          # the one synchronisation of this stage
    want = (nat.POST_TRIGGER_ROUNDING if rounding else 0) | (nat.POST_TRIGGER_SPLITTING if splitting else 0)
    todo = np.nonzero(trig & want)[0].tolist()
    if not todo:
        return {"predictions": pruned, "labels": labels, "n_clusters": n_clusters, "frames_finalized": [], "triggers": trig}
    n, e = labels.shape[0], pruned.shape[0]
    if node_ptr is None:
        node_ptr, edge_ptr = [0, n], [0, e]
    node_ptr, edge_ptr = [int(v) for v in node_ptr], [int(v) for v in edge_ptr]
    ei = edge_index.cpu().numpy()
    pr = np.ascontiguousarray(probs.reshape(-1).cpu().numpy(), dtype=np.float32)
    pred = pruned.cpu().numpy().copy()
    lab = labels.cpu().numpy().copy()
    src, dst = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    total = int(n_clusters.cpu().numpy()[0])
    switches = (nat.POST_ROUNDING if rounding else 0) | (nat.POST_PRUNING if pruning else 0) | (nat.POST_SPLITTING if splitting else 0)
    lib = nat.lib()
    np_h, ep_h = np.asarray(node_ptr, dtype=np.int32), np.asarray(edge_ptr, dtype=np.int32)
    listed, k_new = np.asarray(todo, dtype=np.int32), np.zeros(len(todo), dtype=np.int32)
    roots = lab == np.arange(n, dtype=lab.dtype)                       # the device chain's labels: a component's smallest node id
    before = sum(int(roots[np_h[g]:np_h[g + 1]].sum()) for g in todo)
    st = lib.gnncca_post_finalize_frames_host(src.ctypes.data, dst.ctypes.data, np_h.ctypes.data, ep_h.ctypes.data, listed.ctypes.data, len(todo),
                                              pr.ctypes.data, pred.ctypes.data, switches, lab.ctypes.data, k_new.ctypes.data, 0)
    if st:
        nat.check(st, "gnncca_post_finalize_frames_host")
    total += int(k_new.sum()) - before
    dev = pruned.device
    return {"predictions": torch.from_numpy(pred).to(dev), "labels": torch.from_numpy(lab).to(dev),
            "n_clusters": torch.tensor([total], dtype=torch.int32, device=dev), "frames_finalized": todo, "triggers": trig}
