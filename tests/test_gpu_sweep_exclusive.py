"""The threshold sweep over the camera-exclusive partition on the MI355X (csrc/eval_sweep_exclusive.cuh:
calibration.sweep_thresholds(partition='exclusive'), FrameResult.sweep(partition='exclusive'), gnncca_eval_sweep_exclusive) against the
loop it replaces -- per threshold postprocess.exclusive_clusters(at=t), then evaluate_frames of its predictions and labels -- and, for the
labels, against the sequential walk of tests/exclusive_oracle.py.  Every comparison is exact (NaN rows compare equal to NaN rows): the
rule compares float32 values, the scoring is the same code on the same predictions and partition, so there is no tolerance to choose."""
import copy
import types

import numpy as np
import pytest
import torch

import exclusive_oracle as oracle

pytestmark = pytest.mark.gpu


# ---- batches --------------------------------------------------------------------------------------------------------------------------
def _hand_batch(frames, seed=0):
    """frames: list of (n, src, dst, scores, cam) with frame-local ids -> a GraphBatch as evaluate_frames and sweep_thresholds take it
    (edge labels from random person ids: label 1 iff both ends carry one id), with cam_dev / cam_host, the scores on the device as
    b.scores and host copies as b.h for the oracle."""
    from gnn_cca_amd.sharding import GraphBatch
    rng = np.random.default_rng(seed)
    node_ptr, edge_ptr, ei, sc, cam, lab = [0], [0], [np.zeros((2, 0), np.int64)], [np.zeros(0, np.float32)], [np.zeros(0, np.int32)], [np.zeros(0, np.float32)]
    for n, src, dst, s, c in frames:
        v0 = node_ptr[-1]
        assert len(c) == n and len(src) == len(dst) == len(s)
        src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
        person = rng.integers(0, max(2, n // 2), size=n)
        ei.append(np.stack([src + v0, dst + v0]).reshape(2, -1))
        sc.append(np.asarray(s, np.float32).reshape(-1)), cam.append(np.asarray(c, np.int32).reshape(-1))
        lab.append((person[src] == person[dst]).astype(np.float32))
        node_ptr.append(v0 + n), edge_ptr.append(edge_ptr[-1] + len(src))
    h = types.SimpleNamespace(ei=np.concatenate(ei, axis=1), scores=np.concatenate(sc), cam=np.concatenate(cam), node_ptr=node_ptr,
                              edge_ptr=edge_ptr, n=node_ptr[-1])
    b = GraphBatch(None, torch.from_numpy(h.ei).cuda(), None, edge_ptr, node_ptr)
    b.edge_labels = torch.from_numpy(np.concatenate(lab)).cuda()
    b.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    b.edge_ptr_dev = torch.tensor(edge_ptr, dtype=torch.int32).cuda()
    b.cam_dev, b.cam_host = torch.from_numpy(h.cam).cuda(), h.cam
    b.scores, b.h = torch.from_numpy(h.scores).cuda(), h
    return b


def _pairs_frame(n, pairs, weights, cam):
    src, dst, scores = oracle.mutual_pairs(n, pairs, weights)
    return (n, src, dst, scores, cam)


def _random_frame(rng, n, cams, n_pairs, coarse=False, shuffle=False):
    """n nodes on `cams` cameras, about n_pairs random cross-camera pairs (sparse), both directions with scores of their own: k / 8 for
    k in 1 .. 7 (ties everywhere) or continuous."""
    cam = rng.integers(0, cams, size=n).astype(np.int32)
    if n < 2 or n_pairs == 0:
        return (n, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), cam)
    p = rng.integers(0, n, size=(2, n_pairs))
    p = p[:, cam[p[0]] != cam[p[1]]]
    p = np.unique(np.sort(p, axis=0), axis=1)
    src, dst = np.concatenate([p[0], p[1]]), np.concatenate([p[1], p[0]])
    order = rng.permutation(len(src)) if shuffle else np.lexsort((dst, src))
    e = len(src)
    scores = (rng.integers(1, 8, size=e) / 8.0 if coarse else rng.random(e)).astype(np.float32)
    return (n, src[order], dst[order], scores, cam)


def _complete_frame(rng, cams, per_cam_max=3):
    """`cams` cameras x 1 .. 3 detections per camera, the complete cross-camera graph, uniform scores."""
    cam = np.concatenate([np.full(int(rng.integers(1, per_cam_max + 1)), c) for c in range(cams)]).astype(np.int32)
    n = len(cam)
    src, dst = np.nonzero(cam[:, None] != cam[None, :])
    return (n, src, dst, rng.random(len(src)).astype(np.float32), cam)


# ---- the yardstick: the loop over functions this sweep does not touch --------------------------------------------------------------------
def _loop(b, ths, scores=None, cam=None, node_ptr=None, max_frame_nodes=None):
    """Per threshold exclusive_clusters(at=t) and evaluate_frames of its result -> (rows [T, G, 16], labels [T, N], cut [T, G]) on the host."""
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import exclusive_clusters
    scores = b.scores if scores is None else scores
    cam = b.cam_dev if cam is None else cam
    rows, labels, cut = [], [], []
    for t in ths:
        ex = exclusive_clusters(b.edge_index, scores, cam, int(b.node_ptr[-1]), b.node_ptr if node_ptr is None else node_ptr,
                                b.edge_ptr if node_ptr is None else b.edge_ptr_dev, at=float(t), max_frame_nodes=max_frame_nodes)
        rows.append(evaluate_frames(b, ex["predictions"], ex["labels"]))
        labels.append(ex["labels"]), cut.append(ex["cut"])
    return torch.stack(rows).cpu().numpy(), torch.stack(labels).cpu().numpy(), torch.stack(cut).cpu().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _assert_sweep_equals_loop(b, ths, where, walk=True):
    """The sweep's rows and labels equal the loop's exactly; the labels equal the numpy walk's; -> (rows, labels, cut) on the host."""
    from gnn_cca_amd.calibration import sweep_thresholds
    rows, labels = sweep_thresholds(b, b.scores, ths, return_labels=True, partition="exclusive")
    g, n = len(b.node_ptr) - 1, int(b.node_ptr[-1])
    assert rows.shape == (len(ths), g, 16) and rows.dtype == torch.float64 and labels.shape == (len(ths), n) and labels.dtype == torch.int32
    only_rows = sweep_thresholds(b, b.scores, ths, partition="exclusive")             # the same bits without the labels
    rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    assert _same(rows, only_rows.cpu().numpy()), where
    want_rows, want_labels, cut = _loop(b, ths)
    for t, th in enumerate(ths):
        bad = np.argwhere(~((rows[t] == want_rows[t]) | (np.isnan(rows[t]) & np.isnan(want_rows[t]))))
        assert _same(rows[t], want_rows[t]), (where, t, th, bad[:4].tolist())
        assert np.array_equal(labels[t], want_labels[t]), (where, t, th)
        if walk:
            h = b.h
            assert np.array_equal(labels[t], oracle.exclusive_oracle(h.ei, h.scores, h.cam, h.node_ptr, h.edge_ptr, th)["labels"]), (where, t, th)
    return rows, labels, cut


# ---- hand cases with the answer written out (tests/test_exclusive_oracle.py has the reasoning) ---------------------------------------------
HAND = [
    # two triangles joined by one strong cross pair whose cameras clash with the rest
    (6, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)], [0.6, 0.6, 0.8, 0.7, 0.6, 0.6, 0.9], [0, 1, 2, 0, 1, 2]),
    # a path with increasing weights on nine cameras
    (9, [(v, v + 1) for v in range(8)], [0.55 + 0.05 * v for v in range(8)], list(range(9))),
    # a star whose leaves share a camera: only the heaviest leaf joins
    (5, [(0, 1), (0, 2), (0, 3), (0, 4)], [0.6, 0.9, 0.7, 0.8], [0, 1, 1, 1, 1]),
    # all weights equal: the tie rule decides everything
    (4, [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2)], [0.75] * 5, [0, 1, 0, 1]),
]


def _f32(x):
    return float(np.float32(x))


def test_hand_cases_swept_between_on_and_beyond_their_weights():
    b = _hand_batch([_pairs_frame(*case) for case in HAND])
    # below every weight, between, ON a weight (the float32 itself: active), one float64 step above it (not active), beyond every weight
    ths = [0.5, _f32(0.6), float(np.nextafter(np.float64(_f32(0.6)), 1.0)), 0.65, _f32(0.75), 0.775, _f32(0.9), 0.95, 0.3]
    rows, labels, cut = _assert_sweep_equals_loop(b, ths, "hand cases")
    local = [[(labels[t][b.node_ptr[f]:b.node_ptr[f + 1]] - b.node_ptr[f]).tolist() for f in range(4)] for t in range(len(ths))]
    assert local[0] == [[0, 1, 1, 1, 4, 4], [0] * 9, [0, 1, 0, 3, 4], [0, 0, 2, 2]] and cut[0].tolist() == [4, 0, 3, 3]
    assert local[8] == local[0] and _same(rows[8], rows[0])                          # nothing lies between 0.3 and 0.5
    assert local[1][0] == [0, 1, 1, 1, 4, 4] and local[2][0] == [0, 1, 1, 1, 4, 5]   # (4, 5) at 0.6: in at the weight, out just above
    assert local[4][3] == [0, 0, 2, 2] and local[5][3] == [0, 1, 2, 3]                # all weights 0.75: on, then beyond
    assert local[6][0] == [0, 1, 2, 2, 4, 5] and local[6][2] == [0, 1, 0, 3, 4]       # only the 0.9 pairs are left
    assert local[7] == [list(range(n)) for n in (6, 9, 5, 4)] and rows[7][:, 3].sum() + rows[7][:, 4].sum() == 0
    assert rows[0][:, 15].tolist() == [3.0, 1.0, 4.0, 2.0]


def test_wave_and_block_boundaries_with_ties_everywhere():
    sizes = [1, 2, 63, 64, 65, 255, 256, 257]
    ths = [0.5, 0.05, 0.625, 0.95, 0.5, 0.3, 0.75]                                   # unsorted, a duplicate, below and above every score
    for shuffle in (False, True):
        rng = np.random.default_rng(3)
        b = _hand_batch([_random_frame(rng, n, 5, 3 * n, coarse=True, shuffle=shuffle) for n in sizes])
        assert ths[1] < b.h.scores.min() and b.h.scores.max() < ths[3]
        rows, labels, cut = _assert_sweep_equals_loop(b, ths, ("sizes 1 .. 257", shuffle))
        assert _same(rows[0], rows[4]) and np.array_equal(labels[0], labels[4])
        assert np.array_equal(labels[3], np.arange(b.h.n)) and rows[3][:, 3].sum() + rows[3][:, 4].sum() == 0
        assert (cut[1] > 0).sum() >= 4 and (cut[0] > 0).sum() >= 3                   # the cameras do clash
        assert rows[1][:, 15].sum() < rows[5][:, 15].sum() < rows[0][:, 15].sum() < rows[2][:, 15].sum() < rows[6][:, 15].sum()


def test_scoring_coverage_against_the_component_sweep():
    from gnn_cca_amd.calibration import sweep_thresholds
    rng = np.random.default_rng(12)
    b = _hand_batch([_complete_frame(rng, int(rng.integers(3, 7))) for _ in range(48)], seed=5)
    ths = [0.2, 0.35, 0.5, 0.65, 0.8, 0.9, 0.95]
    rows, labels, cut = _assert_sweep_equals_loop(b, ths, "complete frames")
    comp_rows, comp_labels = sweep_thresholds(b, b.scores, ths, return_labels=True)    # the default partition: the components
    comp_rows, comp_labels = comp_rows.cpu().numpy(), comp_labels.cpu().numpy()
    cells = cut.size
    n_cut, n_legal = int((cut > 0).sum()), int((cut == 0).sum())
    print(f"cells with cut > 0: {n_cut} of {cells}; per threshold: {(cut > 0).mean(axis=1).round(2).tolist()}")
    assert 5 * n_cut >= cells and 5 * n_legal >= cells, (n_cut, n_legal)               # neither kind can carry the test alone
    differ = 0
    for t in range(len(ths)):
        for g in range(cut.shape[1]):
            v0, v1 = b.node_ptr[g], b.node_ptr[g + 1]
            if cut[t, g] == 0:   # the components were legal: the same partition, the same predictions, the same row
                assert _same(rows[t, g], comp_rows[t, g]) and np.array_equal(labels[t, v0:v1], comp_labels[t, v0:v1]), (t, g)
            else:
                assert not np.array_equal(labels[t, v0:v1], comp_labels[t, v0:v1]), (t, g)
                assert rows[t, g, 15] > comp_rows[t, g, 15] and rows[t, g, 3] + rows[t, g, 4] < comp_rows[t, g, 3] + comp_rows[t, g, 4], (t, g)
                differ += int(not _same(rows[t, g, 7:12], comp_rows[t, g, 7:12]))
    assert differ >= n_cut // 2                                                        # the clustering scores move too
    assert len({float(r[:, 3].sum()) for r in rows}) == len(ths)                       # the decisions vary with the threshold


def test_edge_cases_of_the_rule_and_degenerate_frames():
    from gnn_cca_amd.calibration import sweep_thresholds
    from gnn_cca_amd.evaluation import evaluate_frames
    # camera ids 0 and 63 in one cluster (mask bit 63), next to a pair that shares camera 63
    f0 = _pairs_frame(4, [(0, 1), (1, 2), (2, 3)], [0.9, 0.8, 0.7], [0, 63, 63, 5])
    # a one-directional edge, a NaN score, a score exactly at a threshold and one ulp below it
    below = np.nextafter(np.float32(0.75), np.float32(0))
    f1 = (5, [0, 1, 1, 2, 2, 3, 0, 3, 4], [1, 0, 2, 1, 3, 2, 3, 4, 3], np.array([0.75, 0.75, 0.75, below, np.nan, 0.9, 0.9, 0.75, 0.8], np.float32),
          [0, 1, 2, 3, 4])
    # same-camera edges in a raw list: never admissible, whatever they weigh
    f2 = _pairs_frame(3, [(0, 1), (1, 2), (0, 2)], [0.99, 0.8, 0.9], [2, 2, 4])
    none = np.zeros(0, np.int64)
    lone = (7, none, none, np.zeros(0, np.float32), np.arange(7) % 3)
    empty = (0, none, none, np.zeros(0, np.float32), np.zeros(0, np.int32))
    b = _hand_batch([f0, lone, f1, empty, f2])
    ths = [0.75, float(below), 0.5, 0.85]
    rows, labels, cut = _assert_sweep_equals_loop(b, ths, "rule edges")
    assert labels[0].tolist() == [0, 0, 2, 3] + list(range(4, 11)) + [11, 11, 13, 14, 14] + [16, 17, 16]
    assert labels[1][11:16].tolist() == [11, 11, 11, 14, 14]                          # one ulp lower: the pair (1, 2) of f1 is a candidate
    assert labels[3][:4].tolist() == [0, 0, 2, 3] and labels[3][11:16].tolist() == [11, 12, 13, 14, 15]
    assert rows[0][:, 15].tolist() == [3.0, 7.0, 3.0, 0.0, 2.0] and cut[0].tolist() == [1, 0, 0, 0, 2]
    # no edge in the whole batch: every node its own cluster at every threshold, scored as evaluate_frames scores that partition
    b = _hand_batch([lone, empty, (1, none, none, np.zeros(0, np.float32), [5])])
    rows, labels, _ = _assert_sweep_equals_loop(b, [0.1, 0.9], "E == 0")
    want = evaluate_frames(b, torch.zeros(0, dtype=torch.int64, device="cuda"), torch.arange(8, dtype=torch.int32, device="cuda")).cpu().numpy()
    assert _same(rows[0], want) and _same(rows[1], want) and labels.tolist() == [list(range(8))] * 2
    # G = 0: well-formed empty results
    nothing = types.SimpleNamespace(node_ptr=[0], edge_ptr=[0], edge_index=torch.zeros((2, 0), dtype=torch.int64, device="cuda"),
                                    edge_labels=torch.zeros(0, device="cuda"))
    rows, labels = sweep_thresholds(nothing, torch.zeros(0, device="cuda"), [0.1, 0.2, 0.3], return_labels=True, partition="exclusive",
                                    cam=torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert rows.shape == (3, 0, 16) and rows.dtype == torch.float64 and labels.shape == (3, 0)


def test_hundreds_of_rounds_on_a_path():
    n = 300                                  # increasing weights on two alternating cameras: pairs form back to front, one per round
    pairs, weights = [(v, v + 1) for v in range(n - 1)], [0.35 + 0.002 * v for v in range(n - 1)]
    b = _hand_batch([_pairs_frame(n, pairs, weights, [v % 2 for v in range(n)])])
    rows, labels, cut = _assert_sweep_equals_loop(b, [0.3, _f32(0.35 + 0.002 * 150), 0.94], "path")
    assert labels[0].tolist() == [v - (v % 2) for v in range(n)] and cut[0].tolist() == [149]
    assert labels[1][:150].tolist() == list(range(150)) and labels[1][150:].tolist() == [v - (v % 2) for v in range(150, n)]
    assert rows[:, 0, 15].tolist() == [150.0, 225.0, 298.0]                        # at 0.94: the pairs (296, 297) and (298, 299)


def test_the_lds_maximum():
    rng = np.random.default_rng(9)
    b = _hand_batch([_random_frame(rng, 4096, 8, 6000)])                              # one 4096-node frame: 80 KiB of LDS
    rows, labels, cut = _assert_sweep_equals_loop(b, [0.3, 0.7], "4096 nodes")
    assert cut[0][0] > 0 and 1000 < rows[0][0, 15] < rows[1][0, 15] < 4096


def test_the_maximum_grid_in_t():
    rng = np.random.default_rng(2)

    def complete(cam):
        cam = np.asarray(cam, np.int32)
        src, dst = np.nonzero(cam[:, None] != cam[None, :])
        return (len(cam), src, dst, rng.random(len(src)).astype(np.float32), cam)

    b = _hand_batch([complete([0, 0, 1, 1]), complete([0, 1, 2, 0])])                 # 2 frames, 8 nodes, cameras that clash
    ths = np.linspace(0.001, 0.999, 1024)
    rows, labels, cut = _assert_sweep_equals_loop(b, ths.tolist(), "T = 1024", walk=False)
    assert rows.shape == (1024, 2, 16) and (cut > 0).any() and len({tuple(l) for l in labels.tolist()}) >= 4
    assert np.all(np.diff(rows[:, :, 15], axis=0) >= 0)                                # the partitions nest: clusters only split as t rises


def test_two_runs_give_the_same_bits_and_a_frame_does_not_depend_on_its_batch():
    from gnn_cca_amd.calibration import sweep_thresholds
    rng = np.random.default_rng(21)
    frames = [_random_frame(rng, n, 4, 4 * n, coarse=True, shuffle=(k % 2 == 1)) for k, n in enumerate([30, 7, 70, 2, 130, 18])]
    ths = [0.5, 0.25, 0.75]

    def run(fr):
        # (the labels of _hand_batch depend on the frame's place in the batch: give every frame its own)
        b = _hand_batch(fr)
        lab = np.concatenate([(np.asarray(f[1]) + np.asarray(f[2])) % 3 == 0 for f in fr]).astype(np.float32)
        b.edge_labels = torch.from_numpy(lab).cuda()
        rows, labels = sweep_thresholds(b, b.scores, ths, return_labels=True, partition="exclusive")
        return b, rows.cpu().numpy(), labels.cpu().numpy()

    b, first_rows, first_labels = run(frames)
    _, again_rows, again_labels = run(frames)
    assert first_rows.tobytes() == again_rows.tobytes() and np.array_equal(first_labels, again_labels)
    want_rows, want_labels, cut = _loop(b, ths)
    assert _same(first_rows, want_rows) and np.array_equal(first_labels, want_labels) and (cut[0] > 0).sum() >= 3
    rev, rev_rows, rev_labels = run(frames[::-1])
    g = len(frames)
    exact = [q for q in range(16) if q not in (8, 9, 10, 11)]
    for f in range(g):
        v0, v1 = b.node_ptr[f], b.node_ptr[f + 1]
        r = g - 1 - f
        w0 = rev.node_ptr[r]
        assert rev_rows[:, r].tobytes() == first_rows[:, f].tobytes() and np.array_equal(rev_labels[:, w0:w0 + v1 - v0] - w0, first_labels[:, v0:v1] - v0), f
        # The frame with every other frame gone but the largest.  (The workgroup has 64 threads while the batch's largest frame has at
        # most 64 nodes and 256 otherwise, and the scoring's fp64 sums -- the entropies behind AMI, homogeneity, completeness and V -- are
        # ordered per workgroup size, as evaluate_frames' are: all 16 columns are compared where the size is kept.)
        if f != 4:
            _, pair_rows, pair_labels = run([frames[f], frames[4]])
            assert pair_rows[:, 0].tobytes() == first_rows[:, f].tobytes() and np.array_equal(pair_labels[:, :v1 - v0], first_labels[:, v0:v1] - v0), f
        # the frame alone: the partition, the counts, P / R / F, ARI, the precisions and the cluster counts are integers and their quotients
        _, alone_rows, alone_labels = run([frames[f]])
        assert np.array_equal(alone_labels, first_labels[:, v0:v1] - v0), f
        assert alone_rows[:, 0][:, exact].tobytes() == first_rows[:, f][:, exact].tobytes(), f
        if v1 - v0 > 64:
            assert alone_rows[:, 0].tobytes() == first_rows[:, f].tobytes(), f


# ---- the raw entry point: capture, refusals on the device -----------------------------------------------------------------------------------
def _raw(b, ths, cam_dev=None, nptr=None, max_n=None, labels=True):
    """gnncca_eval_sweep_exclusive on preallocated buffers -> (call, rows, labels, keep): call() enqueues on the current stream."""
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.frames import _raw_stream
    lib = nat.lib()
    dev = b.edge_index.device
    g, e, n, t = len(b.node_ptr) - 1, int(b.edge_index.shape[1]), int(b.node_ptr[-1]), len(ths)
    cam_dev = b.cam_dev if cam_dev is None else cam_dev
    nptr = b.node_ptr_dev if nptr is None else nptr
    max_n = int(np.diff(b.node_ptr).max()) if max_n is None else max_n
    th_dev = torch.tensor(list(ths), dtype=torch.float64).cuda()
    rows = torch.empty((t, g, 16), dtype=torch.float64, device=dev)
    lab = torch.empty((t, n), dtype=torch.int32, device=dev) if labels else None
    nbytes = lib.gnncca_eval_sweep_exclusive_workspace_bytes(n, e, g, t)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call():
        st = lib.gnncca_eval_sweep_exclusive(b.edge_index.data_ptr(), b.edge_labels.data_ptr(), b.scores.data_ptr(), cam_dev.data_ptr(), n, e,
                                             nptr.data_ptr(), b.edge_ptr_dev.data_ptr(), g, max_n, th_dev.data_ptr(), t, rows.data_ptr(),
                                             lab.data_ptr() if labels else None, ws.data_ptr(), nbytes, _raw_stream(dev))
        assert st == nat.OK, st
    return call, rows, lab, (th_dev, ws, cam_dev, nptr)


def test_the_entry_point_replays_from_a_graph():
    rng = np.random.default_rng(4)
    b = _hand_batch([_random_frame(rng, n, 4, 4 * n, coarse=True) for n in (25, 9, 40, 0, 33)])
    ths = [0.5, 0.25, 0.75, 0.375, 0.625]
    call, rows, lab, keep = _raw(b, ths)
    call()                                        # warm-up: the code object is loaded before the capture
    torch.cuda.synchronize()
    eager_rows, eager_lab = rows.cpu().numpy(), lab.cpu().numpy()
    want_rows, want_labels, cut = _loop(b, ths)
    assert _same(eager_rows, want_rows) and np.array_equal(eager_lab, want_labels) and (cut > 0).any()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                 # one linear stream of four kernels: plan, plan finish, prepare, sweep
        call()
    for _ in range(2):
        rows.fill_(-7.0), lab.fill_(-7), keep[1].fill_(0xAB)     # (the workspace too: every word that is read is written first)
        graph.replay()
        torch.cuda.synchronize()
        assert rows.cpu().numpy().tobytes() == eager_rows.tobytes() and np.array_equal(lab.cpu().numpy(), eager_lab)


def test_refusals_on_the_device_leave_the_other_frames_alone():
    from gnn_cca_amd.evaluation import evaluate_frames
    rng = np.random.default_rng(8)
    b = _hand_batch([_random_frame(rng, n, 4, 4 * n) for n in (12, 9, 15, 28)])
    ths = [0.3, 0.6]
    good_rows, good_labels, _ = _assert_sweep_equals_loop(b, ths, "untouched")
    # a camera id of 64 in frame 1 and a node range of frame 3 that runs past the batch reach the kernels: frame 1 is scored as "every
    # node its own cluster, predictions 0", frame 3 gets a NaN row -- what the loop gives -- and frames 0 and 2 are as before
    cam = b.h.cam.copy()
    cam[b.node_ptr[1] + 3] = 64
    cam_dev = torch.from_numpy(cam).cuda()
    bad_ptr = list(b.node_ptr)
    bad_ptr[4] = b.h.n + 5
    nptr = torch.tensor(bad_ptr, dtype=torch.int32).cuda()
    call, rows, lab, keep = _raw(b, ths, cam_dev=cam_dev, nptr=nptr)
    lab.fill_(-7)
    call()
    rows, lab = rows.cpu().numpy(), lab.cpu().numpy()
    honest = b.node_ptr_dev
    b.node_ptr_dev = nptr                         # the loop on the same device arrays
    want_rows, want_labels, _ = _loop(b, ths, cam=cam_dev, node_ptr=nptr, max_frame_nodes=28)
    b.node_ptr_dev = honest
    assert _same(rows, want_rows)
    v1, v2, v3 = b.node_ptr[1], b.node_ptr[2], b.node_ptr[3]
    for t in range(len(ths)):
        assert np.isnan(rows[t, 3]).all() and not np.isnan(rows[t, :3]).any()
        assert _same(rows[t, [0, 2]], good_rows[t, [0, 2]]) and not _same(rows[t, 1], good_rows[t, 1])
        assert rows[t, 1, 15] == 9 and rows[t, 1, 3] + rows[t, 1, 4] == 0
        assert np.array_equal(lab[t, :v3], want_labels[t, :v3]) and lab[t, v1:v2].tolist() == list(range(v1, v2))
        assert np.array_equal(lab[t, :v1], good_labels[t, :v1]) and np.array_equal(lab[t, v2:v3], good_labels[t, v2:v3])
        assert (lab[t, v3:] == -7).all()          # a range that does not fit is not written at all
    # frame 1 alone, scored by evaluate_frames as the partition the header names
    ident = torch.arange(b.h.n, dtype=torch.int32, device="cuda")
    zero = torch.zeros(b.edge_index.shape[1], dtype=torch.int64, device="cuda")
    assert _same(rows[0, 1], evaluate_frames(b, zero, ident).cpu().numpy()[1])
    # a frame larger than the stated maximum (16 -> LDS regions of 16): a NaN row for that frame alone
    call, rows, lab, keep = _raw(b, ths, max_n=16, labels=False)
    call()
    rows = rows.cpu().numpy()
    assert np.isnan(rows[:, 3]).all() and _same(rows[:, :3], good_rows[:, :3])


# ---- through the pipeline -----------------------------------------------------------------------------------------------------------------
def _frames(rng, sizes, cams, node_dim=2048, reid_dim=256):
    sizes = np.asarray(sizes)
    n, g = int(sizes.sum()), len(sizes)
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, node_dim)).astype(np.float32),
                reid=rng.standard_normal((n, reid_dim)).astype(np.float32))


def _args(f):
    return f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"]


def _shift_bias(m, b):
    """Put the decision boundary inside the logits so that decisions vary (as tests/test_gpu_evaluation.py does)."""
    with torch.no_grad():
        med = m(b)["classified_edges"][-1].median()
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= med
        m.load_state_dict(sd)


def test_frame_result_sweep_on_both_paths_a_capped_batch_and_the_accumulator():
    import bench
    from gnn_cca_amd.calibration import SweepAccumulator
    from gnn_cca_amd.evaluation import EvalAccumulator, evaluate_frames
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.postprocess import exclusive_clusters
    rng = np.random.default_rng(17)
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    fa = _frames(rng, rng.permutation(np.concatenate([rng.integers(12, 31, size=4), rng.integers(3, 9, size=6)])), 3)
    fb = _frames(rng, [9, 22, 4, 15, 0, 11], 4)
    data = [(f, torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()) for f in (fa, fb)]
    _shift_bias(m, build_graph_batch(*_args(fa), data[0][1], data[0][2]))
    ths = [0.3, 0.5, 0.7]
    swept, cuts = [], 0
    for f, node, reid in data:
        runs = [FramePipeline(m, threshold=th)(*_args(f), node, reid) for th in ths]
        assert [r._d2h is not None for r in runs] == [False, True, False]              # 0.5: the one-call path; the others: step by step
        per_path = [r.sweep(ths, partition="exclusive") for r in runs[:2]]
        assert torch.equal(per_path[0], per_path[1]) or _same(per_path[0].cpu().numpy(), per_path[1].cpu().numpy())
        for t, r in enumerate(runs):              # rows[t] is the exclusive() of a pipeline run at ths[t], scored
            ex = r.exclusive()
            want = evaluate_frames(r.batch, ex["predictions"], ex["labels"])
            assert _same(per_path[1][t].cpu().numpy(), want.cpu().numpy()), t
            cuts += int((ex["cut"] > 0).sum())
        assert not _same(per_path[1].cpu().numpy(), runs[1].sweep(ths).cpu().numpy())   # not the component sweep's rows
        swept.append(per_path[1])
    assert cuts >= 6
    # SweepAccumulator reduces exclusive rows as it reduces any: per threshold EvalAccumulator's result on the same rows
    res = SweepAccumulator(ths).add(swept[0]).add(swept[1]).result()
    for t in range(len(ths)):
        want = EvalAccumulator().add(swept[0][t]).add(swept[1][t]).result()
        got = res["aggregates"][t]
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert got[k] == v or (np.isnan(got[k]) and np.isnan(v)), (t, k, got[k], v)
        assert (res["TP"][t], res["FP"][t], res["FN"][t], res["TN"][t]) == (want["TP"], want["FP"], want["FN"], want["TN"])
    assert res["TP"][0] + res["FP"][0] > res["TP"][2] + res["FP"][2]
    # a capped batch closed under reversal, and the directed capped list of the one-call path: the mutual pairs are the candidates
    f, node, reid = data[0]
    for kw in (dict(top_k=3, symmetric="union"), dict(top_k=3)):
        rc = FramePipeline(m, **kw)(*_args(f), node, reid)
        rows = rc.sweep(ths, partition="exclusive").cpu().numpy()
        b = rc.batch
        for t, th in enumerate(ths):
            ex = exclusive_clusters(b.edge_index, rc.probs, b.cam_dev, int(b.x.shape[0]), b.node_ptr_dev, b.edge_ptr_dev, at=th,
                                    max_frame_nodes=int(np.diff(b.node_ptr).max()))
            assert _same(rows[t], evaluate_frames(b, ex["predictions"], ex["labels"]).cpu().numpy()), (kw, t)
        ex = rc.exclusive()
        assert _same(rows[1], evaluate_frames(rc.batch, ex["predictions"], ex["labels"]).cpu().numpy()), kw
