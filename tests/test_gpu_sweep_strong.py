"""The sweep over the strongly connected clusters on the MI355X (csrc/eval_sweep_strong.cuh: calibration.sweep_thresholds / sweep_joint /
sweep_grid with partition='strong', baselines.geometry_baseline(partition='strong'), FrameResult.sweep(partition='strong'),
gnncca_eval_sweep_strong) against the loop it replaces -- per point the float64 comparisons in torch, postprocess.strong_clusters,
evaluate_frames, all older than the sweep -- bit for bit (NaN-aware) in all 16 columns and in the labels.  Nothing here has a tolerance."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sweep_strong_oracle as so  # noqa: E402

CMP = {"ge": torch.ge, "gt": torch.gt, "le": torch.le, "lt": torch.lt}
NONE = np.zeros(0, np.int64)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def _batch(edge_index, edge_labels, node_ptr, edge_ptr):
    """Host arrays -> a GraphBatch as evaluate_frames and the sweeps take it."""
    from gnn_cca_amd.sharding import GraphBatch
    node_ptr, edge_ptr = [int(v) for v in node_ptr], [int(v) for v in edge_ptr]
    b = GraphBatch(None, torch.from_numpy(np.ascontiguousarray(edge_index, dtype=np.int64).reshape(2, -1)).cuda(), None, edge_ptr, node_ptr)
    b.edge_labels = torch.from_numpy(np.ascontiguousarray(edge_labels, dtype=np.float32)).cuda()
    b.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    b.edge_ptr_dev = torch.tensor(edge_ptr, dtype=torch.int32).cuda()
    return b


def _hand_batch(frames):
    """frames: list of (n, src, dst, lab) with frame-local ids."""
    node_ptr, edge_ptr, ei, lab = [0], [0], [np.zeros((2, 0), np.int64)], [np.zeros(0, np.float32)]
    for n, src, dst, l in frames:
        v0 = node_ptr[-1]
        ei.append(np.stack([np.asarray(src, np.int64) + v0, np.asarray(dst, np.int64) + v0]).reshape(2, -1))
        lab.append(np.asarray(l, np.float32))
        node_ptr.append(v0 + n)
        edge_ptr.append(edge_ptr[-1] + len(src))
    return _batch(np.concatenate(ei, axis=1), np.concatenate(lab), node_ptr, edge_ptr)


def _random_frame(rng, n, e):
    """n nodes, about e DIRECTED edges (self loops excluded, no duplicates), most without their reverse; a seeded 0/1 label per edge."""
    if n < 2 or e == 0:
        return n, NONE, NONE, np.zeros(0, np.float32)
    pairs = rng.integers(0, n, size=(2, e))
    pairs = np.unique(pairs[:, pairs[0] != pairs[1]], axis=1)
    order = rng.permutation(pairs.shape[1])
    ident = rng.integers(0, max(n // 3, 1) + 1, size=n)
    return n, pairs[0][order], pairs[1][order], (ident[pairs[0][order]] == ident[pairs[1][order]]).astype(np.float32)


def _scores(rng, e):
    return torch.from_numpy(rng.random(e).astype(np.float32)).cuda()


def _n(b):
    return int(b.node_ptr[-1])


def _g(b):
    return len(b.node_ptr) - 1


# ---- the loop the sweep replaces ----------------------------------------------------------------------------------------------------------
def _loop(b, scores, points, keep, frame_div=None):
    """Per point: the conjunction of float64 comparisons (the thresholds of a frame are points[t] / frame_div[:, g], divided by numpy in
    float64), strong_clusters on those unpruned predictions, evaluate_frames."""
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import strong_clusters
    points = np.asarray(points, dtype=np.float64)
    e = int(b.edge_index.shape[1])
    frame_of = np.repeat(np.arange(_g(b)), np.diff(np.asarray(b.edge_ptr)))
    rows, labels = [], []
    for p in points:
        preds = torch.ones(e, dtype=torch.bool, device="cuda")
        for k, (s, c) in enumerate(zip(scores, keep)):
            th = np.full(e, p[k]) if frame_div is None else (p[k] / np.asarray(frame_div, dtype=np.float64).reshape(len(scores), -1)[k])[frame_of]
            preds &= CMP[c](s.reshape(-1).double(), torch.from_numpy(np.ascontiguousarray(th)).cuda())
        preds = preds.to(torch.int64)
        post = strong_clusters(b.edge_index, preds, _n(b), list(b.node_ptr), list(b.edge_ptr))
        rows.append(evaluate_frames(b, preds, post["labels"]))
        labels.append(post["labels"])
    return torch.stack(rows).cpu().numpy(), torch.stack(labels).cpu().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)      # NaN-aware equality of float64 rows


def _assert_equals_loop(b, scores, points, keep, where, frame_div=None):
    from gnn_cca_amd.calibration import sweep_joint
    rows, labels = sweep_joint(b, scores, points, keep, frame_div=frame_div, return_labels=True, partition="strong")
    assert rows.shape == (len(points), _g(b), 16) and rows.dtype == torch.float64
    assert labels.shape == (len(points), _n(b)) and labels.dtype == torch.int32
    rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    want_rows, want_labels = _loop(b, scores, points, keep, frame_div)
    for t in range(len(points)):
        bad = np.argwhere(~((rows[t] == want_rows[t]) | (np.isnan(rows[t]) & np.isnan(want_rows[t]))))
        assert _same(rows[t], want_rows[t]), (where, keep, t, list(points[t]), bad[:4])
        assert np.array_equal(labels[t], want_labels[t]), (where, keep, t)
    return rows, labels


def _assert_thresholds_equal_loop(b, scores, ths, keep, where):
    from gnn_cca_amd.calibration import sweep_thresholds
    rows, labels = sweep_thresholds(b, scores, ths, keep=keep, return_labels=True, partition="strong")
    want_rows, want_labels = _loop(b, [scores], [[t] for t in ths], [keep])
    rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    assert rows.shape == want_rows.shape and labels.shape == want_labels.shape and labels.dtype == np.int32
    for t in range(len(ths)):
        assert _same(rows[t], want_rows[t]), (where, keep, t, ths[t])
        assert np.array_equal(labels[t], want_labels[t]), (where, keep, t)
    return rows, labels


# ---- the golden frames --------------------------------------------------------------------------------------------------------------------
THS = [0.2, 0.35, 0.5, 0.65, 0.8]


@pytest.fixture(scope="module")
def golden():
    frames = so.golden_frames()
    h = so.golden_batch(frames)
    b = _batch(h["edge_index"], h["edge_labels"], h["node_ptr"], h["edge_ptr"])
    return frames, h, b, torch.from_numpy(h["probs"]).cuda()


def test_the_golden_frames_as_one_batch(golden):
    from gnn_cca_amd.calibration import sweep_thresholds
    frames, h, b, probs = golden
    rows, labels = _assert_thresholds_equal_loop(b, probs, THS, "ge", "golden")
    assert not np.isnan(rows).any()
    # the rule's own restatement at 0.5: the reference's partitions, nothing pruned
    for g, (name, n, ei, pr, get) in enumerate(frames):
        v0 = h["node_ptr"][g]
        assert so.po.same_partition(labels[2, v0:v0 + n], get("id_unpruned")), name
        assert rows[2, g, 3] + rows[2, g, 4] == get("pred_unpruned").sum(), name
    # ... which the components of the mutual pairs are not
    comp = sweep_thresholds(b, probs, THS, return_labels=True)[1].cpu().numpy()
    for t in range(1, 5):
        differ = sum(not so.po.same_partition(labels[t, h["node_ptr"][g]:h["node_ptr"][g + 1]], comp[t, h["node_ptr"][g]:h["node_ptr"][g + 1]])
                     for g in range(26))
        assert differ >= 15, (THS[t], differ)
    # distances instead of probabilities: 1 - p kept where <= t
    _assert_thresholds_equal_loop(b, 1.0 - probs, THS, "le", "golden 1 - p")


def test_every_golden_frame_singly_gives_its_rows_of_the_batch(golden):
    from gnn_cca_amd.calibration import sweep_thresholds
    frames, h, b, probs = golden
    whole, whole_lab = (v.cpu().numpy() for v in sweep_thresholds(b, probs, THS, return_labels=True, partition="strong"))
    again = sweep_thresholds(b, probs, THS, partition="strong").cpu().numpy()
    assert again.tobytes() == whole.tobytes()                                       # two runs: the same bits
    for g, (name, n, ei, pr, _) in enumerate(frames):
        v0, k0, k1 = h["node_ptr"][g], h["edge_ptr"][g], h["edge_ptr"][g + 1]
        one = _batch(ei, h["edge_labels"][k0:k1], [0, n], [0, k1 - k0])
        rows, labels = _assert_thresholds_equal_loop(one, probs[k0:k1], THS, "ge", name)
        assert rows[:, 0].tobytes() == whole[:, g].tobytes(), name                  # a frame's rows do not depend on the rest of its batch
        assert np.array_equal(labels + v0, whole_lab[:, v0:v0 + n]), name


# ---- the hand case ------------------------------------------------------------------------------------------------------------------------
def test_a_three_cycle_without_a_mutual_pair():
    from gnn_cca_amd.calibration import sweep_thresholds
    b = _hand_batch([(3, [0, 1, 2], [1, 2, 0], [1, 1, 0])])
    s = torch.tensor([0.9, 0.8, 0.7]).cuda()
    rows, labels = sweep_thresholds(b, s, [0.5], return_labels=True, partition="strong")
    # three predicted edges, two of them true; one cluster against one ground-truth cluster (0 - 1 - 2 over the edges with label 1)
    P = 2.0 / 3.0
    want = [P, 1.0, 2.0 * (P * 1.0) / (P + 1.0), 2, 1, 0, 0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 100.0, 1, 1]
    assert rows.cpu().numpy()[0, 0].tolist() == want and labels.cpu().numpy().tolist() == [[0, 0, 0]]
    # the components of the mutual pairs: nothing survives the pruning, three singletons
    rows, labels = sweep_thresholds(b, s, [0.5], return_labels=True)
    want = [0.0, 0.0, 0.0, 0, 0, 2, 1, 0.0, 0.0, 1.0, 0.0, 0.0, 100.0, 0.0, 1, 3]
    assert rows.cpu().numpy()[0, 0].tolist() == want and labels.cpu().numpy().tolist() == [[0, 1, 2]]
    _assert_thresholds_equal_loop(b, s, [0.5, 0.75, 0.95], "ge", "3-cycle")      # the cycle opens at 0.75: three singletons, two predicted


def test_symmetric_scores_give_the_components_sweep_bit_for_bit():
    from gnn_cca_amd.calibration import sweep_joint, sweep_thresholds
    rng = np.random.default_rng(11)
    frames, scores = [], []
    for n in (17, 0, 40, 1, 70):
        pairs = np.unique(np.sort(rng.integers(0, max(n, 1), size=(2, 3 * n)), axis=0), axis=1) if n > 1 else np.zeros((2, 0), np.int64)
        pairs = pairs[:, pairs[0] != pairs[1]]
        both = np.concatenate([pairs, pairs[::-1]], axis=1)                        # closed under reversal: the pruning sees every reverse
        val = rng.random(pairs.shape[1]).astype(np.float32)
        order = rng.permutation(both.shape[1])
        frames.append((n, both[0][order], both[1][order], (rng.random(both.shape[1]) < 0.4).astype(np.float32)))
        scores.append(np.concatenate([val, val])[order])
    b, s = _hand_batch(frames), torch.from_numpy(np.concatenate(scores)).cuda()
    ths = [0.1, 0.4, 0.6, 0.9]
    for keep in ("ge", "le"):
        strong = sweep_thresholds(b, s, ths, keep=keep, return_labels=True, partition="strong")
        comp = sweep_thresholds(b, s, ths, keep=keep, return_labels=True)
        assert strong[0].cpu().numpy().tobytes() == comp[0].cpu().numpy().tobytes() and torch.equal(strong[1], comp[1]), keep
    pts = [[0.3, 0.8], [0.5, 0.5]]
    strong = sweep_joint(b, [s, s], pts, ["gt", "lt"], return_labels=True, partition="strong")
    comp = sweep_joint(b, [s, s], pts, ["gt", "lt"], return_labels=True)
    assert strong[0].cpu().numpy().tobytes() == comp[0].cpu().numpy().tobytes() and torch.equal(strong[1], comp[1])
    assert len(set(strong[1].cpu().numpy()[0].tolist())) < _n(b)                   # something does join


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65])
def test_word_and_block_boundaries(n):
    """The word boundaries of the matrix rows (31 / 32 / 33, 64 / 65) and the switch from the 64-thread to the 256-thread block (64 / 65)."""
    rng = np.random.default_rng(100 + n)
    f = _random_frame(rng, n, 2 * n)
    b = _hand_batch([f])
    ths = [0.0, 0.3, 0.6, 2.0]
    rows, labels = _assert_thresholds_equal_loop(b, _scores(rng, len(f[1])), ths, "ge", n)
    if n >= 31:
        assert len(set(labels[0].tolist())) < n                                   # everything active: something joins
    # a ring through every node, the last edge closing it in the last word: one cluster, and none once the closing edge is off
    ring = _hand_batch([(n, np.arange(n), (np.arange(n) + 1) % n, np.ones(n, np.float32))])
    s = torch.full((n,), 0.9).cuda()
    s[n - 1] = 0.4
    rows, labels = _assert_thresholds_equal_loop(ring, s, [0.3, 0.5], "ge", ("ring", n))
    assert labels[0].tolist() == [0] * n and (n == 1 or labels[1].tolist() == list(range(n)))


def test_all_sizes_in_one_launch_and_a_giant_component_at_257():
    rng = np.random.default_rng(5)
    frames = [_random_frame(rng, n, 2 * n) for n in (1, 2, 31, 32, 33, 64, 65)]
    b = _hand_batch(frames)
    _assert_thresholds_equal_loop(b, _scores(rng, int(b.edge_index.shape[1])), [0.2, 0.5, 0.7], "ge", "sizes together")
    # 257 nodes: a ring through the even nodes and node 256 (129 members), the odd ones singletons
    members = np.concatenate([np.arange(0, 256, 2), [256]])
    src, dst = members, np.roll(members, -1)
    lab = (rng.random(len(src)) < 0.5).astype(np.float32)
    giant = _hand_batch([(257, src, dst, lab), _random_frame(rng, 9, 20)])
    s = torch.cat([torch.full((len(src),), 0.8), torch.rand(int(giant.edge_index.shape[1]) - len(src), generator=torch.Generator().manual_seed(1))]).cuda()
    rows, labels = _assert_thresholds_equal_loop(giant, s, [0.5, 0.9], "ge", "giant")
    assert np.bincount(labels[0][:257]).max() == 129 and (labels[0][1:256:2] == np.arange(1, 256, 2)).all()
    assert labels[1][:257].tolist() == list(range(257))


def test_the_largest_frame_a_ring_of_1024():
    """The full round count (a ring gains nothing from the in-place form) and the largest LDS; then frames of 1, 1024 and 32 together."""
    n = 1024
    src = np.arange(n)
    lab = (src % 3 == 0).astype(np.float32)
    ring = _hand_batch([(n, src, (src + 1) % n, lab)])
    s = torch.full((n,), 0.5).cuda()
    rows, labels = _assert_thresholds_equal_loop(ring, s, [0.25, 0.75], "ge", "ring 1024")        # every edge active; none
    assert labels[0].tolist() == [0] * n and labels[1].tolist() == list(range(n))
    assert rows[0, 0, 15] == 1 and rows[1, 0, 15] == n and rows[0, 0, 3] + rows[0, 0, 4] == n
    rng = np.random.default_rng(8)
    mixed = _hand_batch([_random_frame(rng, 1, 0), (n, src, (src + 1) % n, lab), _random_frame(rng, 32, 80)])
    s = torch.cat([torch.full((n,), 0.5), torch.rand(int(mixed.edge_index.shape[1]) - n, generator=torch.Generator().manual_seed(2))]).cuda()
    _assert_thresholds_equal_loop(mixed, s, [0.25, 0.75], "ge", "1 / 1024 / 32")


# ---- ties and special values ----------------------------------------------------------------------------------------------------------------
def test_ties_nan_negative_zero_duplicates_and_descending_thresholds():
    rng = np.random.default_rng(21)
    b = _hand_batch([_random_frame(rng, 20, 70), _random_frame(rng, 33, 120)])
    e = int(b.edge_index.shape[1])
    s = rng.random(e).astype(np.float32)
    s[::7] = np.float32(0.5)            # scores exactly on a threshold
    s[3::11] = np.nan                   # never active, under any comparator
    s[5::13] = -0.0
    s[6::13] = 0.0
    tie = float(np.float32(0.3))        # a float32 value as a float64 threshold: equal to the widened score
    s[1::17] = np.float32(0.3)
    s = torch.from_numpy(s).cuda()
    pts = [[0.5], [0.0], [tie], [0.5], [0.9], [0.1], [-0.0]]                        # duplicates, no order
    got = {}
    for keep in ("ge", "gt", "le", "lt"):
        got[keep], _ = _assert_equals_loop(b, [s], pts, [keep], "ties")
        assert _same(got[keep][0], got[keep][3]) and _same(got[keep][1], got[keep][6])          # a duplicate; -0.0 is 0.0
    predicted = lambda r: r[:, 3].sum() + r[:, 4].sum()   # noqa: E731
    for x in (0, 1, 2):                                                             # on a tie the strict and the loose comparator part
        assert predicted(got["ge"][x]) > predicted(got["gt"][x]) and predicted(got["le"][x]) > predicted(got["lt"][x]), x
    n_nan = int(torch.isnan(s).sum())
    assert n_nan > 0 and predicted(got["ge"][1]) + predicted(got["lt"][1]) == e - n_nan         # a NaN is on neither side
    _assert_thresholds_equal_loop(b, s, [0.9, 0.5, 0.5, 0.3, 0.0, -1.0], "ge", "descending")
    _assert_thresholds_equal_loop(b, s, [0.9, 0.5, 0.5, 0.3, 0.0, -1.0], "le", "descending")


# ---- the edge list --------------------------------------------------------------------------------------------------------------------------
def test_stray_edges_self_loops_duplicates_and_order():
    from gnn_cca_amd.calibration import sweep_thresholds
    rng = np.random.default_rng(33)
    frames = [_random_frame(rng, n, 3 * n) for n in (12, 30, 7)]
    clean = _hand_batch(frames)
    node_ptr = clean.node_ptr
    s_clean = rng.random(int(clean.edge_index.shape[1])).astype(np.float32)
    # per frame: its edges, then self loops, duplicates of its first edges, and in-range edges that leave the frame -- all shuffled
    ei, lab, sc, edge_ptr = [], [], [], [0]
    ce, cl = clean.edge_index.cpu().numpy(), clean.edge_labels.cpu().numpy()
    for g in range(3):
        k0, k1, v0, v1 = clean.edge_ptr[g], clean.edge_ptr[g + 1], node_ptr[g], node_ptr[g + 1]
        other = (v1 + 2) % node_ptr[-1] if g < 2 else 3                             # a node of another frame, inside [0, N)
        extra = np.array([[v0, v0 + 1, v0, other, v0 + 2], [v0, v0 + 1, other, v0 + 1, other]])
        part = np.concatenate([ce[:, k0:k1], extra, ce[:, k0:k0 + 4]], axis=1)
        part_s = np.concatenate([s_clean[k0:k1], np.full(5, 0.99, np.float32), s_clean[k0:k0 + 4]])
        part_l = np.concatenate([cl[k0:k1], np.array([1, 0, 1, 0, 1], np.float32), cl[k0:k0 + 4]])
        order = rng.permutation(part.shape[1])
        ei.append(part[:, order]), sc.append(part_s[order]), lab.append(part_l[order])
        edge_ptr.append(edge_ptr[-1] + part.shape[1])
    dirty = _batch(np.concatenate(ei, axis=1), np.concatenate(lab), node_ptr, edge_ptr)
    assert int(dirty.edge_index.min()) >= 0 and int(dirty.edge_index.max()) < node_ptr[-1]
    ths = [0.2, 0.5, 0.8]
    _, labels = _assert_thresholds_equal_loop(dirty, torch.from_numpy(np.concatenate(sc)).cuda(), ths, "ge", "dirty list")
    # none of the additions can change a partition
    want = sweep_thresholds(clean, torch.from_numpy(s_clean).cuda(), ths, return_labels=True, partition="strong")[1].cpu().numpy()
    assert np.array_equal(labels, want)


# ---- the joint form -------------------------------------------------------------------------------------------------------------------------
def _frames(rng, sizes, cams=4, node_dim=8, reid_dim=16):
    sizes = np.asarray(sizes)
    n, g = int(sizes.sum()), len(sizes)
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, node_dim)).astype(np.float32),
                reid=rng.standard_normal((n, reid_dim)).astype(np.float32))


@pytest.fixture(scope="module")
def full():
    """A full-mode batch (edge_attr [E, 4]) of 17, 0, 24 and 13 detections, and four asymmetric scores of its edges."""
    from gnn_cca_amd.graph_build import build_graph_batch
    rng = np.random.default_rng(31)
    f = _frames(rng, [17, 0, 24, 13])
    b = build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], torch.from_numpy(f["node"]).cuda(),
                          torch.from_numpy(f["reid"]).cuda())
    assert b.edge_attr.shape[1] == 4 and b.edge_index.shape[1] > 300
    extra = torch.from_numpy(rng.random((4, int(b.edge_index.shape[1]))).astype(np.float32)).cuda()
    return f, b, extra


def test_two_scores_with_divisors_and_four_scores(full):
    f, b, extra = full
    s0, s1 = b.edge_attr[:, 0], b.edge_attr[:, 2:3]                                 # strided views, read in place
    assert not s0.is_contiguous() and s0.stride(0) == 4
    noisy = s1.reshape(-1) * (1.0 + 0.2 * extra[0])                                 # an asymmetric distance: cycles without mutual pairs
    q0 = np.quantile((s0.double().cpu().numpy()), [0.2, 0.5, 0.8])
    q1 = np.quantile(noisy.double().cpu().numpy(), [0.3, 0.6, 0.9])
    div = np.stack([f["max_dist"], np.linspace(0.5, 2.0, 4)])
    frame_scale = float(np.median(f["max_dist"]))
    pts = [[a * frame_scale, c] for a in q0 for c in q1] + [[q0[1] * frame_scale, q1[1]]]
    for keep in (["lt", "lt"], ["le", "lt"], ["gt", "le"]):
        rows, labels = _assert_equals_loop(b, [s0, noisy], pts, keep, "K = 2", frame_div=div)
        assert _same(rows[4], rows[9])
    assert len({tuple(l.tolist()) for l in labels}) >= 3                            # the partitions do vary over the points
    _assert_equals_loop(b, [s0, noisy], pts[:3], ["lt", "lt"], "K = 2, no divisors")
    pts4 = [[0.2, 0.9, 0.1, 0.95], [0.5, 0.5, 0.5, 0.5], [0.0, 1.0, 0.0, 1.0], [0.1, 0.8, 0.3, 0.7]]
    rows, _ = _assert_equals_loop(b, list(extra), pts4, ["ge", "le", "gt", "lt"], "K = 4")
    assert rows[2][:, 5].sum() + rows[2][:, 6].sum() < 0.01 * b.edge_index.shape[1] and rows[1][:, 3].sum() + rows[1][:, 4].sum() > 0
    _assert_equals_loop(b, extra, pts4, ["ge", "le", "gt", "lt"], "K = 4 as one [K, E] tensor", frame_div=np.full((4, 4), 1.25))


def test_one_score_equals_sweep_thresholds_and_grid_shapes(full):
    from gnn_cca_amd.calibration import sweep_grid, sweep_joint, sweep_thresholds
    f, b, extra = full
    s = extra[1]
    ths = [0.5, -1.0, 0.25, 2.0, 0.5, 0.37]
    for keep in ("ge", "le"):
        want = sweep_thresholds(b, s, ths, keep=keep, return_labels=True, partition="strong")
        got = sweep_joint(b, [s], [[t] for t in ths], [keep], return_labels=True, partition="strong")
        assert got[0].cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes() and torch.equal(got[1], want[1]), keep
    assert sweep_thresholds(b, s.view(-1, 1), ths, partition="strong", cam="ignored").cpu().numpy().tobytes() == \
        sweep_thresholds(b, s, ths, partition="strong").cpu().numpy().tobytes()
    axes = [[0.3, 0.6, 0.9], [0.2, 0.7]]
    rows, labels = sweep_grid(b, [extra[0], extra[2]], axes, ["le", "ge"], return_labels=True, partition="strong")
    assert rows.shape == (3, 2, _g(b), 16) and labels.shape == (3, 2, _n(b))
    flat = sweep_joint(b, [extra[0], extra[2]], [[a, c] for a in axes[0] for c in axes[1]], ["le", "ge"], return_labels=True, partition="strong")
    assert rows.reshape(6, _g(b), 16).cpu().numpy().tobytes() == flat[0].cpu().numpy().tobytes() and torch.equal(labels.reshape(6, -1), flat[1])
    want_rows, _ = _loop(b, [extra[0], extra[2]], [[0.6, 0.7]], ["le", "ge"])
    assert _same(rows[1, 1].cpu().numpy(), want_rows[0])
    assert sweep_grid(b, [extra[0], extra[2]], axes, ["le", "ge"], partition="strong").shape == (3, 2, _g(b), 16)


def test_geometry_baseline_under_the_reference_rule(full):
    from gnn_cca_amd.baselines import geometry_baseline
    f, b, extra = full
    geom = float(np.quantile(b.edge_attr[:, 0].double().cpu().numpy() * np.median(f["max_dist"]), 0.3))
    reid = float(np.quantile(b.edge_attr[:, 2].double().cpu().numpy(), 0.5))
    g = _g(b)
    for kw, scores, pts, div in (({}, [b.edge_attr[:, 0]], [[geom]], f["max_dist"].reshape(1, g)),
                                 ({"reid_th": reid / 31.5, "max_dist_l2": 31.5}, [b.edge_attr[:, 0], b.edge_attr[:, 2]],
                                  [[geom, (reid / 31.5) * 31.5]], np.stack([f["max_dist"], np.ones(g)]))):
        got = geometry_baseline(b, geom, f["max_dist"], partition="strong", **kw)
        want, _ = _loop(b, scores, pts, ["lt"] * len(scores), frame_div=div)
        assert got.shape == (g, 16) and _same(got.cpu().numpy(), want[0]), kw
        assert got[:, 3].sum() + got[:, 4].sum() > 0
    # the attributes of a complete graph are symmetric: the default partition gives the same rows there
    assert _same(geometry_baseline(b, geom, f["max_dist"]).cpu().numpy(), geometry_baseline(b, geom, f["max_dist"], partition="strong").cpu().numpy())


def test_many_points():
    """T = 1024 against the loop, and T = MAX_POINTS on one 4-node frame (the grid's y extent) against the points it repeats."""
    from gnn_cca_amd.calibration import MAX_POINTS, sweep_joint, sweep_thresholds
    rng = np.random.default_rng(77)
    b = _hand_batch([_random_frame(rng, 9, 30), _random_frame(rng, 4, 9)])
    s = _scores(rng, int(b.edge_index.shape[1]))
    rows, _ = _assert_thresholds_equal_loop(b, s, np.linspace(-0.01, 1.01, 1024).tolist(), "ge", "T = 1024")
    assert len({r.tobytes() for r in rows}) > 20
    four = _hand_batch([(4, [0, 1, 2, 3, 0, 2], [1, 2, 0, 0, 3, 3], [1, 0, 1, 0, 1, 1])])
    s4 = torch.tensor([0.9, 0.8, 0.7, 0.3, 0.6, 0.2]).cuda()
    distinct = [0.1, 0.25, 0.5, 0.65, 0.75, 0.85, 0.95, 0.6]
    small, small_lab = _assert_thresholds_equal_loop(four, s4, distinct, "ge", "4 nodes")
    assert MAX_POINTS == 16384
    rows, labels = sweep_joint(four, [s4], np.tile(np.array(distinct), MAX_POINTS // 8).reshape(-1, 1), ["ge"], return_labels=True, partition="strong")
    rows, labels = rows.cpu().numpy().reshape(MAX_POINTS // 8, 8, 1, 16), labels.cpu().numpy().reshape(MAX_POINTS // 8, 8, 4)
    assert all(_same(rows[i], small) for i in range(MAX_POINTS // 8)) and (labels == small_lab[None]).all()
    assert sweep_thresholds(four, s4, distinct, partition="strong").cpu().numpy().tobytes() == small.tobytes()


# ---- degenerate input -----------------------------------------------------------------------------------------------------------------------
def test_no_edges_no_frames_and_a_frame_without_edges():
    from gnn_cca_amd.calibration import sweep_joint, sweep_thresholds
    none = torch.zeros(0).cuda()
    # E = 0: every node its own cluster, nothing predicted
    b = _hand_batch([(3, NONE, NONE, []), (0, NONE, NONE, []), (5, NONE, NONE, [])])
    rows, labels = _assert_thresholds_equal_loop(b, none, [0.5, 0.1], "ge", "E = 0")
    assert labels.tolist() == [list(range(8))] * 2 and rows[0, 0, 15] == 3 and rows[0, 2, 15] == 5
    # G = 0
    empty = _batch(np.zeros((2, 0), np.int64), [], [0], [0])
    rows, labels = sweep_thresholds(empty, none, [0.5, 0.6], return_labels=True, partition="strong")
    assert rows.shape == (2, 0, 16) and labels.shape == (2, 0)
    assert sweep_joint(empty, [none, none], [[0.5, 0.6]], ["lt", "ge"], partition="strong").shape == (1, 0, 16)
    # a frame without edges between two with edges
    rng = np.random.default_rng(3)
    b = _hand_batch([_random_frame(rng, 10, 30), (6, NONE, NONE, []), _random_frame(rng, 35, 90)])
    rows, labels = _assert_thresholds_equal_loop(b, _scores(rng, int(b.edge_index.shape[1])), [0.3, 0.6], "ge", "a frame without edges")
    assert labels[0][10:16].tolist() == list(range(10, 16))


# ---- the raw entry --------------------------------------------------------------------------------------------------------------------------
def _raw(b, scores, points_dev, n_points, cmps, max_n, rows, labels, ws, div_dev=None):
    from gnn_cca_amd import _native as nat
    from gnn_cca_amd.frames import _raw_stream
    lib = nat.lib()
    k, e = len(scores), int(b.edge_index.shape[1])
    ptrs = (C.c_void_p * k)(*[s.data_ptr() for s in scores])
    strides = (C.c_int64 * k)(*[max(int(s.stride(0)), 1) for s in scores])
    cm = (C.c_int32 * k)(*[nat.CMP[c] for c in cmps])
    return lib.gnncca_eval_sweep_strong(b.edge_index.data_ptr(), b.edge_labels.data_ptr(), ptrs, strides, cm, k, _n(b), e, b.node_ptr_dev.data_ptr(),
                                        b.edge_ptr_dev.data_ptr(), _g(b), max_n, points_dev.data_ptr(), n_points,
                                        div_dev.data_ptr() if div_dev is not None else None, rows.data_ptr(),
                                        labels.data_ptr() if labels is not None else None, ws.data_ptr(), ws.numel(), _raw_stream(rows.device))


def test_raw_entry_dirty_workspace_capture_and_a_frame_wider_than_declared():
    from gnn_cca_amd import _native as nat
    rng = np.random.default_rng(9)
    frames = [_random_frame(rng, 20, 60), _random_frame(rng, 100, 300), _random_frame(rng, 33, 100)]
    b = _hand_batch(frames)
    e, n, g = int(b.edge_index.shape[1]), _n(b), _g(b)
    s = _scores(rng, e)
    ths = [0.3, 0.6, 0.45]
    pts = torch.tensor(ths, dtype=torch.float64).cuda()
    want_rows, want_labels = _loop(b, [s], [[t] for t in ths], ["ge"])
    ws_bytes = nat.lib().gnncca_eval_sweep_strong_workspace_bytes(n, e, g)
    assert ws_bytes == nat.lib().gnncca_eval_workspace_bytes(n, e, g)

    def fresh():
        return (torch.full((3, g, 16), -7.0, dtype=torch.float64).cuda(), torch.full((3, n), -7, dtype=torch.int32).cuda(),
                torch.full((ws_bytes,), 0xFF, dtype=torch.uint8).cuda())        # a workspace of NaN bit patterns: nothing of it is read unwritten

    rows, labels, ws = fresh()
    assert _raw(b, [s], pts, 3, ["ge"], 100, rows, labels, ws) == nat.OK
    assert _same(rows.cpu().numpy(), want_rows) and np.array_equal(labels.cpu().numpy(), want_labels)
    rows2 = torch.full_like(rows, -7.0)
    assert _raw(b, [s], pts, 3, ["ge"], 100, rows2, None, ws) == nat.OK           # no labels asked: the rows alone, on the used workspace
    assert rows2.cpu().numpy().tobytes() == rows.cpu().numpy().tobytes()
    # a frame declared narrower than it is: max_frame_nodes = 60 -> capacity 64, frame 1 has 100 detections
    rows, labels, ws = fresh()
    assert _raw(b, [s], pts, 3, ["ge"], 60, rows, labels, ws) == nat.OK
    got, lab = rows.cpu().numpy(), labels.cpu().numpy()
    assert np.isnan(got[:, 1]).all() and (lab[:, 20:120] == np.arange(20, 120)).all()
    # its neighbours are scored as the loop scores them in a batch of that declared width (the scorer's block, and with it the order of
    # its float64 sums, follows the declared width: eval_frames' choice)
    k1, k2 = b.edge_ptr[1], b.edge_ptr[2]
    narrow_rows, narrow_labels = _loop(_hand_batch([frames[0], frames[2]]), [torch.cat([s[:k1], s[k2:]])], [[t] for t in ths], ["ge"])
    assert _same(got[:, 0], narrow_rows[:, 0]) and _same(got[:, 2], narrow_rows[:, 1])
    assert np.array_equal(lab[:, :20], narrow_labels[:, :20]) and np.array_equal(lab[:, 120:], narrow_labels[:, 20:] + 100)
    assert np.array_equal(lab[:, :20], want_labels[:, :20]) and np.array_equal(lab[:, 120:], want_labels[:, 120:])
    assert np.array_equal(got[:, [0, 2], 3:7], want_rows[:, [0, 2], 3:7])         # the counts do not depend on the width
    # one capture on a side stream (two kernel nodes: no memset, no wait, no allocation) and one replay
    rows, labels, ws = fresh()
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert _raw(b, [s], pts, 3, ["ge"], 100, rows, labels, ws) == nat.OK
    rows.fill_(-7.0), labels.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(rows.cpu().numpy(), want_rows) and np.array_equal(labels.cpu().numpy(), want_labels)


# ---- the pipeline and the accumulators ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """One synthetic batch and a model whose decision boundary lies inside its logits (tests/test_gpu_strong_clusters.py's recipe)."""
    import bench
    from gnn_cca_amd.graph_build import build_graph_batch
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()
    rng = np.random.default_rng(1)
    sizes = rng.integers(0, 24, size=12)
    f = _frames(rng, sizes, node_dim=2048, reid_dim=256)
    node, reid = torch.from_numpy(f["node"]).cuda(), torch.from_numpy(f["reid"]).cuda()
    b = build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
    with torch.no_grad():
        med = m(b)["classified_edges"][-1].median()
        sd = m.state_dict()
        key = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[key] -= med
        m.load_state_dict(sd)
    return m, f, node, reid


def test_pipeline_sweep_scores_its_own_operating_points(scene):
    from gnn_cca_amd.pipeline import FramePipeline
    m, f, node, reid = scene

    def run(**kw):
        r = FramePipeline(m, pruning=False, splitting=False, **kw)(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)
        torch.cuda.synchronize()
        return r

    r = run()
    other = float(np.quantile(r.probs.double().cpu().numpy(), 0.7))
    assert 0.0 < other < 1.0 and other != 0.5
    rows = r.sweep([0.5, other], partition="strong")
    assert torch.equal(rows[0], r.evaluate(final=False))
    r2 = run(threshold=other)
    assert torch.equal(r2.probs, r.probs) and not torch.equal(r2.preds, r.preds)
    assert torch.equal(rows[1], r2.evaluate(final=False))
    assert not torch.equal(rows, r.sweep([0.5, other]))                            # the default partition stays what it was: mutual pairs


def test_the_rows_go_through_both_accumulators(golden):
    from gnn_cca_amd.calibration import JointSweepAccumulator, SweepAccumulator, sweep_joint, sweep_thresholds
    frames, h, b, probs = golden
    rows = sweep_thresholds(b, probs, THS, partition="strong")
    want_rows, _ = _loop(b, [probs], [[t] for t in THS], ["ge"])
    want = torch.from_numpy(want_rows).cuda()
    got, ref = SweepAccumulator(THS).add(rows).add(rows).result(), SweepAccumulator(THS).add(want).add(want).result()
    assert got["aggregates"] == ref["aggregates"] and np.array_equal(got["F_micro"], ref["F_micro"])
    assert np.array_equal(got["TP"], 2 * want_rows[:, :, 3].sum(axis=1).astype(np.int64)) and got["TP"].max() > 0
    pts = [[t] for t in THS]
    jrows = sweep_joint(b, [probs], pts, ["ge"], partition="strong")
    got, ref = JointSweepAccumulator(pts).add(jrows).add(jrows).result(), JointSweepAccumulator(pts).add(want).add(want).result()
    assert got["frames"] == 52 and np.array_equal(got["sums"], ref["sums"]) and got["aggregates"] == ref["aggregates"]
    assert np.array_equal(got["FP"], 2 * want_rows[:, :, 4].sum(axis=1).astype(np.int64))
