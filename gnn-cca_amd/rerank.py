"""The baseline the GNN has to beat: rank-R ReID association with k-reciprocal re-ranking, on the GPU.

The reference's `MODE: eval_RANK` (main.py:366-386, inference.py:388-511) links every detection to its RANK nearest cross-camera
detections by ReID distance and scores the components of those links; with `RERANK: True` (config_inference.yaml:13-15) the distances
first go through k-reciprocal re-ranking (libs/utils.py:578-644, Zhong et al., k1=20, k2=6, lambda=0.3) -- several Python loops per frame
over numpy rows, after two device-to-host copies.  Here it is three launches on the batch the GNN path already has (csrc/rerank.cuh),
none of which waits for the GPU, and the scorer is the GNN's own:

    dist = frame_distances(batch)                       # FrameMatrices: every frame's n x n L2 distances of batch.reid_embeds
    dist = rerank_frames(dist, k1=20, k2=6, lam=0.3)    # FrameMatrices: re_ranking per frame, the whole n x n
    pred = rank_predictions(batch, dist, rank=1)        # int64 [E] on the batch's own edge list
    rows = rank_baseline(batch, rank=1)                 # the chain + prune_and_cluster + evaluate_frames: float64 [G, 16]
    acc = EvalAccumulator(); acc.add(rows) ...; acc.result()   # main.py:374-386's averages, one synchronisation per run

include/gnncca_mpn.h states the re-ranking step by step; tests/rerank_oracle.py is the same statement in numpy.  Deviations from the
reference, all deliberate:

* eval_RANK passes ONE matrix to re_ranking three times (as query-gallery, query-query and gallery-gallery block), so every distance
  has an exact twin and the result depends on the tie order of numpy's unstable argsort.  That is not reproduced: a frame is re-ranked
  as one set, which is what re_ranking computes for any query / gallery split of it, and ties go to the smaller index.
* A column of zeros (a single detection, or identical embeddings) normalises to a row of zeros, where the reference divides 0 by 0.
* When RANK exceeds a detection's cross-camera candidates the reference goes on to pick same-camera detections at its filler distance
  of 100 and puts those pairs into the clustering graph; rank_predictions stops at the candidates.
* Frames of more than 128 detections are refused (NotImplementedError) by rerank_frames and rank_predictions: a frame's tables live in LDS.
* What the baseline scores with real ReID features: not measured -- no trained model or images exist in this repository."""
import numbers

import torch

from . import _native as nat
from .evaluation import _dev_i32, evaluate_frames
from .frames import _f32c, _on, _raw_stream
from .postprocess import prune_and_cluster

MAX_FRAME_NODES, MAX_K1 = nat.RERANK_MAX_FRAME_NODES, nat.RERANK_MAX_K1
_ONLY_GPU = "gnn_cca_amd.rerank runs on MI355X only (no CPU fallback)"


class FrameMatrices:
    """One square fp32 matrix per frame of a batch, back to back: `.data` float32 [sum n_g^2] on the device, frame g's n_g x n_g
    row-major matrix at `.mat_ptr[g]` (G + 1 host ints, mat_ptr[g] = sum_{q<g} n_q^2); `.node_ptr` the G + 1 host ints of the batch.
    `.node_ptr_dev` (optional, int32 [G + 1] on the device) spares the calls below an upload.  Anything with the first three fields is
    accepted where a FrameMatrices is: a caller can supply their own distances."""
    __slots__ = ("data", "mat_ptr", "node_ptr", "node_ptr_dev")

    def __init__(self, data, node_ptr, node_ptr_dev=None):
        self.node_ptr = [int(v) for v in node_ptr]
        self.mat_ptr = _mat_ptr(self.node_ptr)
        if data.numel() != self.mat_ptr[-1]:
            raise ValueError(f"data has {data.numel()} elements; node_ptr asks for {self.mat_ptr[-1]}")
        self.data, self.node_ptr_dev = data, node_ptr_dev

    def __len__(self):
        return len(self.node_ptr) - 1

    def frame(self, g):
        n = self.node_ptr[g + 1] - self.node_ptr[g]
        return self.data[self.mat_ptr[g]:self.mat_ptr[g + 1]].view(n, n)


def _mat_ptr(node_ptr):
    out = [0]
    for a, b in zip(node_ptr[:-1], node_ptr[1:]):
        if b < a:
            raise ValueError("node_ptr must not decrease")
        out.append(out[-1] + (b - a) * (b - a))
    return out


def _frames_of(obj, what):
    """The host node_ptr of a batch or a FrameMatrices -> (list, G, N, largest frame)."""
    node_ptr = [int(v) for v in obj.node_ptr]
    if len(node_ptr) < 1 or (node_ptr and node_ptr[0] != 0):
        raise ValueError(f"{what}: node_ptr must hold G + 1 entries starting at 0")
    g = len(node_ptr) - 1
    sizes = [b - a for a, b in zip(node_ptr[:-1], node_ptr[1:])]
    if any(s < 0 for s in sizes):
        raise ValueError(f"{what}: node_ptr must not decrease")
    return node_ptr, g, node_ptr[-1], max(sizes, default=0)


def _check_dist(dist, what):
    """A FrameMatrices or its like -> (node_ptr, G, N, largest frame, total); ValueError before anything touches the GPU."""
    for field in ("data", "mat_ptr", "node_ptr"):
        if not hasattr(dist, field):
            raise ValueError(f"{what}: `dist` needs the fields data, mat_ptr and node_ptr (a FrameMatrices)")
    node_ptr, g, n, max_n = _frames_of(dist, what)
    want = _mat_ptr(node_ptr)
    if [int(v) for v in dist.mat_ptr] != want:
        raise ValueError(f"{what}: dist.mat_ptr is not the running sum of the squared frame sizes of dist.node_ptr")
    if not torch.is_tensor(dist.data) or dist.data.numel() != want[-1]:
        raise ValueError(f"{what}: dist.data must be a tensor of {want[-1]} elements")
    return node_ptr, g, n, max_n, want[-1]


def _node_ptr_dev(obj, node_ptr, like):
    """The int32 [G + 1] device copy of node_ptr: the one `obj` carries, or an upload next to the device tensor `like`."""
    have = getattr(obj, "node_ptr_dev", None)
    if have is not None:
        return _dev_i32(have, like)
    staged = torch.empty(len(node_ptr), dtype=torch.int32, pin_memory=True)   # no wait: pinned, non-blocking, stream-ordered
    staged.copy_(torch.tensor(node_ptr, dtype=torch.int32))
    return staged.to(like.device, non_blocking=True)


def _int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer in [{lo}, {hi if hi is not None else 'inf'}], not {v!r}")
    return int(v)


def frame_distances(batch):
    """All-pairs L2 distances of `batch.reid_embeds` inside every frame -- torch.cdist(reid, reid, p=2) per frame (inference.py:416) -> a
    FrameMatrices.  One launch on the current stream, no wait.  sqrt of the sum of squared differences in fp32 (not |a|^2 + |b|^2 - 2ab,
    whose cancellation is worst for the near neighbours that get ranked): the diagonal is exactly 0, the matrix exactly symmetric, the
    relative error at most (R + 2) 2^-24.  Any embedding width R >= 1 and any frame size."""
    node_ptr, g, n, max_n = _frames_of(batch, "frame_distances")
    reid = batch.reid_embeds
    if reid.dim() != 2 or reid.shape[0] != n or reid.shape[1] < 1:
        raise ValueError(f"frame_distances: batch.reid_embeds must be [N, R] with N = {n} and R >= 1, not {tuple(reid.shape)}")
    if not reid.is_cuda:
        raise RuntimeError(_ONLY_GPU)
    dev = reid.device
    mat_ptr = _mat_ptr(node_ptr)
    with _on(dev):
        x = _f32c(reid.detach())
        nptr = _node_ptr_dev(batch, node_ptr, x)
        out = torch.empty(mat_ptr[-1], dtype=torch.float32, device=dev)
        st = nat.lib().gnncca_frame_distances(x.data_ptr(), x.shape[1], n, nptr.data_ptr(), g, max_n, mat_ptr[-1], out.data_ptr(),
                                              _raw_stream(dev))
        if st:
            nat.check(st, "gnncca_frame_distances")
    return FrameMatrices(out, node_ptr, nptr)


def check_rerank_args(k1, k2, lam):
    k1 = _int("k1", k1, 1, MAX_K1)
    k2 = _int("k2", k2, 1, k1)
    if isinstance(lam, bool) or not isinstance(lam, numbers.Real) or not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"lam must be a real number in [0, 1], not {lam!r}")
    return k1, k2, float(lam)


def rerank_frames(dist, k1=20, k2=6, lam=0.3, debug=False):
    """k-reciprocal re-ranking of every frame's matrix (libs/utils.py:578-644; the steps are in include/gnncca_mpn.h) -> a FrameMatrices
    with the whole n x n result per frame, diagonal included.  One launch on the current stream, one workgroup per frame, no wait; two
    runs give the same bits.  1 <= k1 <= 64, 1 <= k2 <= k1, 0 <= lam <= 1 (ValueError); frames of at most 128 detections
    (NotImplementedError) -- both before anything is launched.
    debug=True returns (result, dict(rank int32 [N, C] -- the first C = min(max(k1 + 1, k2), largest frame) entries of every detection's
    ranking as frame-local ids, -1 beyond its frame's size; expansion / support bool [N, 128] -- X(i) and the columns where V'[i] is not
    zero)), all on the device."""
    k1, k2, lam = check_rerank_args(k1, k2, lam)
    node_ptr, g, n, max_n, total = _check_dist(dist, "rerank_frames")
    if max_n > MAX_FRAME_NODES:
        raise NotImplementedError(f"rerank_frames: a frame has {max_n} detections; a frame's tables live in LDS, at most {MAX_FRAME_NODES}")
    if not dist.data.is_cuda:
        raise RuntimeError(_ONLY_GPU)
    dev = dist.data.device
    with _on(dev):
        d = _f32c(dist.data.detach()).reshape(-1)
        nptr = _node_ptr_dev(dist, node_ptr, d)
        out = torch.empty(total, dtype=torch.float32, device=dev)
        cols = max(min(max(k1 + 1, k2), max_n), 1)
        rank_out = torch.full((n, cols), -1, dtype=torch.int32, device=dev) if debug else None
        mask_out = torch.zeros((n, 4), dtype=torch.int64, device=dev) if debug else None
        st = nat.lib().gnncca_rerank_frames(d.data_ptr(), total, n, nptr.data_ptr(), g, max_n, k1, k2, lam, out.data_ptr(),
                                            rank_out.data_ptr() if debug else None, cols, mask_out.data_ptr() if debug else None,
                                            _raw_stream(dev))
        if st:
            nat.check(st, "gnncca_rerank_frames")
    res = FrameMatrices(out, node_ptr, nptr)
    if not debug:
        return res
    bits = torch.arange(64, device=dev, dtype=torch.int64)
    as_bool = ((mask_out.unsqueeze(-1) >> bits) & 1).bool()          # [N, 4, 64]
    return res, {"rank": rank_out, "expansion": as_bool[:, 0:2].reshape(n, 128), "support": as_bool[:, 2:4].reshape(n, 128)}


def rank_predictions(batch, dist, rank=1):
    """Predictions on the batch's own edge list (inference.py:454-481) -> int64 [E]: edge (i, j) is 1 iff j is among the
    min(rank, deg_i) detections of i's frame on another camera with the smallest dist[i][.], or i is among j's; ties go to the smaller
    node id.  One launch, no wait.  The result is symmetric by construction, so prune_and_cluster removes nothing and its labels are the
    reference's components.  A capped batch (top_k=) is legal: an edge that is not in the list is simply not predicted.  Needs
    batch.cam_dev, batch.node_ptr_dev / edge_ptr_dev (build_graph_batch and FramePipeline provide them); frames of at most 128."""
    rank = min(_int("rank", rank, 1), 2 ** 31 - 1)
    node_ptr, g, n, max_n, total = _check_dist(dist, "rank_predictions")
    if [int(v) for v in batch.node_ptr] != node_ptr:
        raise ValueError("rank_predictions: dist.node_ptr and batch.node_ptr disagree")
    if max_n > MAX_FRAME_NODES:
        raise NotImplementedError(f"rank_predictions: a frame has {max_n} detections; the selected sets live in LDS, at most {MAX_FRAME_NODES}")
    cam = getattr(batch, "cam_dev", None)
    if cam is None:
        raise ValueError("rank_predictions needs batch.cam_dev (int32 [N] on the device)")
    if cam.numel() != n:
        raise ValueError(f"rank_predictions: batch.cam_dev [{cam.numel()}] does not match the batch (N={n})")
    e = int(batch.edge_index.shape[1])
    if not (dist.data.is_cuda and batch.edge_index.is_cuda):
        raise RuntimeError(_ONLY_GPU)
    dev = dist.data.device
    with _on(dev):
        d = _f32c(dist.data.detach()).reshape(-1)
        ei = batch.edge_index.contiguous()
        cam = _dev_i32(cam, d)
        nptr, eptr = _dev_i32(batch.node_ptr_dev, d), _dev_i32(batch.edge_ptr_dev, d)
        pred = torch.empty(e, dtype=torch.int64, device=dev)
        st = nat.lib().gnncca_rank_predictions(d.data_ptr() if total else None, total, cam.data_ptr() if n else None, n,
                                               ei.data_ptr() if e else None, e, nptr.data_ptr(), eptr.data_ptr(), g, max_n, rank,
                                               pred.data_ptr() if e else None, _raw_stream(dev))
        if st:
            nat.check(st, "gnncca_rank_predictions")
    return pred


def rank_baseline(batch, rank=1, rerank=True, k1=20, k2=6, lam=0.3):
    """eval_RANK on one batch: frame_distances -> (rerank_frames) -> rank_predictions -> prune_and_cluster -> evaluate_frames; returns
    what evaluate_frames returns, float64 [G, 16] on the device (columns evaluation.METRICS), without a wait.  Feed the rows of a run to an
    EvalAccumulator for main.py:374-386's five averages (RI, MI, hom, com, v)."""
    rank = _int("rank", rank, 1)
    if rerank:
        check_rerank_args(k1, k2, lam)
    _, _, n, max_n = _frames_of(batch, "rank_baseline")
    if max_n > MAX_FRAME_NODES:
        raise NotImplementedError(f"rank_baseline: a frame has {max_n} detections; at most {MAX_FRAME_NODES}")
    dist = frame_distances(batch)
    if rerank:
        dist = rerank_frames(dist, k1, k2, lam)
    pred = rank_predictions(batch, dist, rank)
    post = prune_and_cluster(batch.edge_index, pred, n, batch.node_ptr_dev, batch.edge_ptr_dev)
    return evaluate_frames(batch, post["pruned"], post["labels"])


__all__ = ["MAX_FRAME_NODES", "MAX_K1", "FrameMatrices", "frame_distances", "rerank_frames", "rank_predictions", "rank_baseline"]
