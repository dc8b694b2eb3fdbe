"""Camera-exclusive clusters, the parts that need no GPU: the rule's oracle (tests/exclusive_oracle.py, the sequential walk) against an
independent restatement as mutual-best rounds -- the form the kernel is built in -- on random frames with frequent ties; the properties
the GPU tests rely on (one detection per camera in every cluster; the plain connected components wherever they are legal); hand cases
with the answer written out; the entry points declared, bound and exported; and every refusal before a device is touched (host tensors
stand in: a check that came too late would raise the module's "MI355X only" RuntimeError instead)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import exclusive_oracle as oracle
from conftest import ROOT


def _random_frame(rng, n, cams, density, coarse):
    """A frame of n nodes on `cams` cameras: every cross-camera ordered pair is an edge with probability `density`, scores either
    multiples of 1/8 (ties everywhere) or continuous, the two directions of a pair drawn separately."""
    cam = rng.integers(0, cams, size=n)
    src, dst = [], []
    for i in range(n):
        for j in range(n):
            if i != j and cam[i] != cam[j] and rng.random() < density:
                src.append(i), dst.append(j)
    e = len(src)
    scores = (rng.integers(0, 9, size=e) / 8.0 if coarse else rng.random(e)).astype(np.float32)
    return cam, np.asarray(src, np.int64), np.asarray(dst, np.int64), scores


def _rounds(src, dst, scores, cam, n, th):
    """Mutual-best rounds on one frame, written independently of the oracle's walk: in each round every cluster takes the first admissible
    candidate incident to it (descending weight, then lo, then hi); candidates chosen from both sides merge; stop when nothing is
    admissible.  -> (labels, number of rounds that merged)."""
    s64 = scores.astype(np.float64)
    where = {(int(a), int(b)): k for k, (a, b) in reversed(list(enumerate(zip(src, dst))))}
    cands = []
    for (i, j), k in where.items():
        r = where.get((j, i))
        if i < j and r is not None and s64[k] >= th and s64[r] >= th:
            cands.append((-float(np.float32(min(scores[k], scores[r]))), i, j))
    label = list(range(n))
    mask = [1 << int(c) for c in cam]
    merged_rounds = 0
    while True:
        best = {}
        for c in cands:
            a, b = label[c[1]], label[c[2]]
            if a != b and not (mask[a] & mask[b]):
                for root in (a, b):
                    if root not in best or c < best[root]:
                        best[root] = c
        merges = [(label[c[1]], label[c[2]]) for root, c in best.items()
                  if root == max(label[c[1]], label[c[2]]) and best.get(min(label[c[1]], label[c[2]])) == c]
        if not merges:
            return np.asarray(label, dtype=np.int32), merged_rounds
        merged_rounds += 1
        for a, b in merges:
            lo, hi = min(a, b), max(a, b)
            mask[lo] |= mask[hi]
            label = [lo if l == hi else l for l in label]


def test_walk_equals_mutual_best_rounds_and_keeps_one_detection_per_camera():
    rng = np.random.default_rng(7)
    legal = illegal = 0
    for trial in range(600):
        n = int(rng.integers(1, 14))
        cams = int(rng.choice([2, 3, 4, 6]))
        coarse = trial % 2 == 0
        cam, src, dst, scores = _random_frame(rng, n, cams, float(rng.choice([0.3, 0.6, 1.0])), coarse)
        th = float(rng.choice([0.25, 0.5, 0.625]))
        got = oracle.exclusive_oracle(np.stack([src, dst]), scores, cam, [0, n], [0, len(src)], th)
        want, _ = _rounds(src, dst, scores, cam, n, th)
        assert np.array_equal(got["labels"], want), (trial, n, cams, th)
        assert oracle.one_per_camera(got["labels"], cam), trial
        assert got["n_clusters"] == len(set(got["labels"].tolist())) and got["flags"].tolist() == [0]
        # the predictions: exactly the candidate edges inside a cluster; cut: the candidate pairs between two
        comp, pruned = oracle.plain_components(np.stack([src, dst]), scores, [0, n], [0, len(src)], th)
        inside = got["labels"][src] == got["labels"][dst]
        assert np.array_equal(got["predictions"], pruned * inside), trial
        assert int(got["cut"][0]) == int((pruned * ~inside).sum()) // 2, trial
        if oracle.one_per_camera(comp, cam):        # the plain components are legal: nothing is cut, nothing differs
            legal += 1
            assert np.array_equal(got["labels"], comp) and np.array_equal(got["predictions"], pruned) and got["cut"][0] == 0, trial
        else:
            illegal += 1
            assert got["cut"][0] > 0, trial
    assert legal >= 100 and illegal >= 100, (legal, illegal)     # the set is not one-sided


def test_frames_of_a_batch_do_not_influence_each_other():
    rng = np.random.default_rng(11)
    frames = [_random_frame(rng, n, 4, 0.7, True) for n in (5, 0, 9, 1, 12)]
    node_ptr, edge_ptr, ei, sc, cams = [0], [0], [], [], []
    for cam, src, dst, scores in frames:
        ei.append(np.stack([src, dst]) + node_ptr[-1])
        sc.append(scores), cams.append(cam)
        node_ptr.append(node_ptr[-1] + len(cam)), edge_ptr.append(edge_ptr[-1] + len(src))
    whole = oracle.exclusive_oracle(np.concatenate(ei, axis=1), np.concatenate(sc), np.concatenate(cams), node_ptr, edge_ptr, 0.5)
    total = 0
    for f, (cam, src, dst, scores) in enumerate(frames):
        alone = oracle.exclusive_oracle(np.stack([src, dst]), scores, cam, [0, len(cam)], [0, len(src)], 0.5)
        assert np.array_equal(whole["labels"][node_ptr[f]:node_ptr[f + 1]], alone["labels"] + node_ptr[f])
        assert np.array_equal(whole["predictions"][edge_ptr[f]:edge_ptr[f + 1]], alone["predictions"]) and whole["cut"][f] == alone["cut"][0]
        total += alone["n_clusters"]
    assert whole["n_clusters"] == total


def _one(n, pairs, weights, cam, th=0.5):
    src, dst, scores = oracle.mutual_pairs(n, pairs, weights)
    res = oracle.exclusive_oracle(np.stack([src, dst]), scores, cam, [0, n], [0, len(src)], th)
    return res, src, dst, scores


def test_hand_two_triangles_joined_by_a_strong_pair_whose_cameras_clash():
    # triangles {0, 1, 2} and {3, 4, 5} on cameras 0, 1, 2 each; the cross pair (2, 3) is the strongest of all and legal by itself
    # (cameras 2 and 0), so it merges FIRST; after it {2, 3} holds cameras 0 and 2 and can only take a camera-1 node: (1, 2) at 0.8
    # before (3, 4) at 0.7, whose node 4 is then a second camera 1 and stays out.  0 and 5 clash with the cluster's cameras 0 and 2.
    cam = [0, 1, 2, 0, 1, 2]
    pairs = [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)]
    weights = [0.6, 0.6, 0.8, 0.7, 0.6, 0.6, 0.9]
    res, src, dst, scores = _one(6, pairs, weights, cam)
    assert res["labels"].tolist() == [0, 1, 1, 1, 4, 4]            # {0}, {1, 2, 3}, {4, 5}: (4, 5) at 0.6 is still legal
    assert res["n_clusters"] == 3 and res["cut"].tolist() == [4]   # cut: (0, 1), (0, 2), (3, 4), (3, 5)
    kept = {(int(a), int(b)) for a, b, p in zip(src, dst, res["predictions"]) if p}
    assert kept == {(1, 2), (2, 1), (2, 3), (3, 2), (4, 5), (5, 4)}
    assert _rounds(src, dst, scores, cam, 6, 0.5)[1] == 3          # (2, 3), then (1, 2), then (4, 5)


def test_hand_path_with_increasing_weights_takes_n_minus_one_rounds():
    n = 9
    pairs = [(v, v + 1) for v in range(n - 1)]
    weights = [0.55 + 0.05 * v for v in range(n - 1)]              # the last pair is the strongest: only it is mutual in round one
    cam = list(range(n))                                            # nine cameras: everything is admissible
    res, src, dst, scores = _one(n, pairs, weights, cam)
    assert res["labels"].tolist() == [0] * n and res["n_clusters"] == 1 and res["cut"].tolist() == [0] and res["predictions"].all()
    assert _rounds(src, dst, scores, cam, n, 0.5)[1] == n - 1
    # alternating cameras: only pairs can form; the walk takes (7, 8), (5, 6), (3, 4), (1, 2) and leaves 0 alone
    res, *_ = _one(n, pairs, weights, [v % 2 for v in range(n)])
    assert res["labels"].tolist() == [0, 1, 1, 3, 3, 5, 5, 7, 7] and res["cut"].tolist() == [4]


def test_hand_star_whose_leaves_share_a_camera():
    # centre 0 on camera 0, leaves 1 .. 4 on camera 1: only the heaviest leaf joins
    res, *_ = _one(5, [(0, 1), (0, 2), (0, 3), (0, 4)], [0.6, 0.9, 0.7, 0.8], [0, 1, 1, 1, 1])
    assert res["labels"].tolist() == [0, 1, 0, 3, 4] and res["n_clusters"] == 4 and res["cut"].tolist() == [3]


def test_hand_all_weights_equal_the_tie_rule_decides_everything():
    # a 4-cycle 0-1-2-3-0 plus the chord (0, 2), every weight 0.75; cameras 0, 1, 0, 1.  Order: (0,1) (0,2) (0,3) (1,2) (2,3).
    # (0,1) merges; (0,2) clashes (camera 0 twice); (0,3) clashes (camera 1 twice); (1,2) clashes; (2,3) merges.
    res, src, dst, _ = _one(4, [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2)], [0.75] * 5, [0, 1, 0, 1])
    assert res["labels"].tolist() == [0, 0, 2, 2] and res["cut"].tolist() == [3]
    # a score exactly at the threshold is active, one ulp below is not, a NaN never is, a one-directional edge is no candidate
    below = np.nextafter(np.float32(0.75), np.float32(0))
    ei = np.array([[0, 1, 1, 2, 2, 3, 0], [1, 0, 2, 1, 3, 2, 3]])
    scores = np.array([0.75, 0.75, 0.75, below, np.nan, 0.9, 0.9], dtype=np.float32)
    res = oracle.exclusive_oracle(ei, scores, [0, 1, 2, 3], [0, 4], [0, 7], 0.75)
    assert res["labels"].tolist() == [0, 0, 2, 3] and res["predictions"].tolist() == [1, 1, 0, 0, 0, 0, 0] and res["cut"].tolist() == [0]


def test_oracle_marks_a_frame_with_a_camera_id_out_of_range():
    ei = np.array([[0, 1, 2, 3], [1, 0, 3, 2]])
    res = oracle.exclusive_oracle(ei, np.full(4, 0.9, np.float32), [0, 64, 0, 63], [0, 2, 4], [0, 2, 4], 0.5)
    assert res["flags"].tolist() == [1, 0] and res["labels"].tolist() == [0, 1, 2, 2] and res["predictions"].tolist() == [0, 0, 1, 1]
    assert res["n_clusters"] == 3 and res["cut"].tolist() == [0, 0]


class _Batch:
    """What FrameResult.exclusive reads of a GraphBatch, on the host."""

    def __init__(self, cam, sizes):
        self.node_ptr = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        self.edge_ptr = [0] * (len(sizes) + 1)
        self.x = torch.zeros((len(cam), 2))
        self.edge_index = torch.zeros((2, 0), dtype=torch.int64)
        self.cam_host = np.asarray(cam, dtype=np.int64)
        self.cam_dev = torch.tensor(cam, dtype=torch.int32)
        self.node_ptr_dev = torch.tensor(self.node_ptr, dtype=torch.int32)
        self.edge_ptr_dev = torch.tensor(self.edge_ptr, dtype=torch.int32)


def test_every_value_error_comes_before_the_gpu_is_touched():
    from gnn_cca_amd.pipeline import FrameResult
    from gnn_cca_amd.postprocess import MAX_CAMERAS, MAX_FRAME_NODES, exclusive_clusters
    assert MAX_FRAME_NODES == 4096 and MAX_CAMERAS == 64
    assert "_excl" in FrameResult.__slots__ and callable(FrameResult.exclusive)
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    probs, cam = torch.full((4,), 0.9), torch.tensor([0, 1, 2], dtype=torch.int32)
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), "0.3", None, True):
        with pytest.raises(ValueError, match="threshold"):
            exclusive_clusters(ei, probs, cam, 3, [0, 3], [0, 4], at=bad)
    for bad_cam in ([0, 64, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match="camera ids"):
            exclusive_clusters(ei, probs, torch.tensor(bad_cam, dtype=torch.int32), 3, [0, 3], [0, 4])
    with pytest.raises(ValueError, match="does not match"):
        exclusive_clusters(ei, probs[:3], cam, 3, [0, 3], [0, 4])
    with pytest.raises(ValueError, match="does not match"):
        exclusive_clusters(ei, probs, cam[:2], 3, [0, 3], [0, 4])
    with pytest.raises(ValueError, match=r"G \+ 1"):
        exclusive_clusters(ei, probs, cam, 3, [0, 1, 3], [0, 4])
    with pytest.raises(ValueError, match="ascend"):
        exclusive_clusters(ei, probs, cam, 3, [0, 2], [0, 4])
    with pytest.raises(ValueError, match="ascend"):
        exclusive_clusters(ei, probs, cam, 3, [0, 3], [0, 3])
    with pytest.raises(ValueError, match="required"):
        exclusive_clusters(ei, probs, cam, 3, None, None)
    with pytest.raises(ValueError, match=r"\[2, E\]"):
        exclusive_clusters(ei.t(), probs, cam, 3, [0, 3], [0, 4])
    big = torch.zeros(4097, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 4096"):
        exclusive_clusters(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0), big, 4097, [0, 4097], [0, 0])
    # what is left is a well-formed call on host tensors: the module's usual refusal, camera 63 included
    with pytest.raises(RuntimeError, match="MI355X only"):
        exclusive_clusters(ei, probs.view(-1, 1), torch.tensor([0, 63, 5], dtype=torch.int32), 3, [0, 3], [0, 4], at=0.3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        exclusive_clusters(ei, probs, cam, 3, torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32))

    # FrameResult.exclusive: the batch's host camera ids and frame sizes are judged first
    class Pipe:
        threshold = 0.5

    for cam_ids, sizes, word in (([0, 1, 64], [3], "camera ids"), ([0, -1, 2], [2, 1], "camera ids"), ([0] * 4097, [4097], "at most 4096")):
        r = FrameResult()
        r.batch, r.probs, r._pipe = _Batch(cam_ids, sizes), torch.zeros(0), Pipe()
        with pytest.raises(ValueError, match=word):
            r.exclusive()
    r = FrameResult()
    r.batch, r.probs, r._pipe = _Batch([0, 1, 63], [2, 1]), torch.zeros(0), Pipe()
    with pytest.raises(RuntimeError, match="MI355X only"):
        r.exclusive()


def _declaration(header, name, result="int"):
    m = re.search(r"GNNCCA_API\s+" + result + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gnncca_mpn.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_the_binding_mirrors_them():
    from gnn_cca_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gnncca_mpn.h")).read()
    lib = nat.lib()
    for name, result, res, count in (("gnncca_post_exclusive_workspace_bytes", "size_t", C.c_size_t, 3),
                                     ("gnncca_post_exclusive_frames", "int", C.c_int, 18)):
        args = _declaration(header, name, result)
        got_res, argtypes = nat._SIGNATURES[name]
        assert len(args) == count == len(argtypes) and got_res is res, name
        assert name in nat.exported_symbols() and hasattr(lib, name)
    args = _declaration(header, "gnncca_post_exclusive_frames")
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "edge_index", "scores", "n_nodes", "n_edges", "cam", "node_ptr_dev", "edge_ptr_dev", "n_frames", "max_frame_nodes", "threshold",
        "predictions_out", "labels_out", "n_clusters_out", "cut_out", "flags_out", "workspace", "workspace_bytes", "stream"]
    assert nat._SIGNATURES["gnncca_post_exclusive_frames"][1][9] is C.c_double
    assert "#define GNNCCA_EXCLUSIVE_MAX_FRAME_NODES 4096" in header and nat.EXCLUSIVE_MAX_FRAME_NODES == 4096
    assert "#define GNNCCA_EXCLUSIVE_MAX_CAMERAS 64" in header and nat.EXCLUSIVE_MAX_CAMERAS == 64
    assert "#define GNNCCA_ABI_VERSION 2" in header and nat.ABI_VERSION == 2 == lib.gnncca_abi_version()
    for word in ("active", "candidates", "weight", "order", "clustering", "NaN score is never active", "camera masks are disjoint",
                 "duplicate ordered pairs"):
        assert word in header, word


def test_entry_point_refuses_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    fake = 0x10000
    n, e, g = 10, 24, 2
    ws = lib.gnncca_post_exclusive_workspace_bytes(n, e, g)
    assert ws > 0 and ws % 256 == 0 and ws >= lib.gnncca_post_workspace_bytes(n, e) + 4 * e + 8 * e
    assert lib.gnncca_post_exclusive_workspace_bytes(-1, e, g) == 0 and lib.gnncca_post_exclusive_workspace_bytes(n, e, -1) == 0

    def call(th=0.5, max_n=6, ei=fake, sc=fake, cam=fake, nptr=fake, eptr=fake, pred=fake, lab=fake, k=fake, cut=fake, fl=fake, work=fake,
             nbytes=ws, nn=n, ee=e, gg=g):
        return lib.gnncca_post_exclusive_frames(ei, sc, nn, ee, cam, nptr, eptr, gg, max_n, th, pred, lab, k, cut, fl, work, nbytes, None)

    for th in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(th=th) == nat.ERR_INVALID_ARG, th
    assert call(max_n=4097) == nat.ERR_INVALID_ARG and call(max_n=-1) == nat.ERR_INVALID_ARG and call(max_n=n + 1) == nat.ERR_INVALID_ARG
    for name in ("ei", "sc", "cam", "nptr", "eptr", "pred", "lab", "k", "cut", "fl", "work"):
        assert call(**{name: None}) == nat.ERR_INVALID_ARG, name
    assert call(nn=-1) == nat.ERR_INVALID_ARG and call(ee=-1) == nat.ERR_INVALID_ARG and call(gg=-1) == nat.ERR_INVALID_ARG
    assert call(gg=0) == nat.ERR_INVALID_ARG                       # nodes, but no frame to put them in
    assert call(nbytes=ws - 1) == nat.ERR_WORKSPACE
