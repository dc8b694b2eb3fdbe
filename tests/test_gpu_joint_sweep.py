"""The joint sweep on the MI355X (csrc/eval_sweep_joint.cuh: calibration.sweep_joint / sweep_grid / JointSweepAccumulator,
baselines.geometry_baseline) against the loop it replaces -- the conjunction of float64 torch comparisons -> prune_and_cluster ->
evaluate_frames, one point at a time -- bit for bit in all 16 columns and in the partitions; against sweep_thresholds where the two
overlap (K = 1); against the reference's own statements (tests/golden/calibration/geom_appearance.npz); and the running sums against the
numpy restatement of their order (tests/joint_sweep_oracle.py)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_sweep_oracle as jo  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "calibration", "geom_appearance.npz")
CMP = {"ge": torch.ge, "gt": torch.gt, "le": torch.le, "lt": torch.lt}


def _frames(rng, sizes, cams=4, node_dim=8, reid_dim=16):
    sizes = np.asarray(sizes)
    n, g = int(sizes.sum()), len(sizes)
    return dict(sizes=sizes, n=n, id_cam=rng.integers(0, cams, size=n), ids=rng.integers(0, 11, size=n), xw=rng.uniform(-10, 10, n),
                yw=rng.uniform(-10, 10, n), max_dist=rng.uniform(10, 90, g), node=rng.standard_normal((n, node_dim)).astype(np.float32),
                reid=rng.standard_normal((n, reid_dim)).astype(np.float32))


def _build(f):
    from gnn_cca_amd.graph_build import build_graph_batch
    return build_graph_batch(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], torch.from_numpy(f["node"]).cuda(),
                             torch.from_numpy(f["reid"]).cuda())


def _hand_batch(frames):
    """frames: list of (n, src, dst, lab) with frame-local ids -> a GraphBatch as evaluate_frames takes it."""
    from gnn_cca_amd.sharding import GraphBatch
    node_ptr, edge_ptr, ei, lab = [0], [0], [np.zeros((2, 0), np.int64)], [np.zeros(0, np.float32)]
    for n, src, dst, l in frames:
        v0 = node_ptr[-1]
        ei.append(np.stack([np.asarray(src, np.int64) + v0, np.asarray(dst, np.int64) + v0]).reshape(2, -1))
        lab.append(np.asarray(l, np.float32))
        node_ptr.append(v0 + n)
        edge_ptr.append(edge_ptr[-1] + len(src))
    b = GraphBatch(None, torch.from_numpy(np.concatenate(ei, axis=1)).cuda(), None, edge_ptr, node_ptr)
    b.edge_labels = torch.from_numpy(np.concatenate(lab)).cuda()
    b.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    b.edge_ptr_dev = torch.tensor(edge_ptr, dtype=torch.int32).cuda()
    return b


def _random_frame(rng, n, e):
    """n nodes, about e ordered pairs, three quarters of them with their reverse; edges in a random order."""
    none = np.zeros(0, np.int64)
    if n < 2:
        return n, none, none, np.zeros(0, np.float32)
    pairs = rng.integers(0, n, size=(2, e))
    pairs = pairs[:, pairs[0] != pairs[1]]
    pairs = np.unique(np.concatenate([pairs, pairs[::-1, : (3 * pairs.shape[1]) // 4]], axis=1), axis=1)
    order = rng.permutation(pairs.shape[1])
    return n, pairs[0][order], pairs[1][order], (rng.random(pairs.shape[1]) < 0.4).astype(np.float32)


def _n(b):
    return int(b.node_ptr[-1])


def _g(b):
    return len(b.node_ptr) - 1


def _loop(b, scores, points, keep, frame_div=None):
    """The loop the sweep replaces: per point, the conjunction of float64 comparisons, prune_and_cluster, evaluate_frames.  The
    thresholds of a frame are points[t] / frame_div[:, g], divided by numpy in float64."""
    from gnn_cca_amd.evaluation import evaluate_frames
    from gnn_cca_amd.postprocess import prune_and_cluster
    points = np.asarray(points, dtype=np.float64)
    e = int(b.edge_index.shape[1])
    frame_of = np.repeat(np.arange(_g(b)), np.diff(np.asarray(b.edge_ptr)))
    rows, labels = [], []
    for p in points:
        preds = torch.ones(e, dtype=torch.bool, device="cuda")
        for k, (s, c) in enumerate(zip(scores, keep)):
            th = np.full(e, p[k]) if frame_div is None else (p[k] / np.asarray(frame_div, dtype=np.float64)[k])[frame_of]
            preds &= CMP[c](s.reshape(-1).double(), torch.from_numpy(np.ascontiguousarray(th)).cuda())
        post = prune_and_cluster(b.edge_index, preds.to(torch.int64), _n(b), b.node_ptr_dev, b.edge_ptr_dev)
        rows.append(evaluate_frames(b, post["pruned"], post["labels"]))
        labels.append(post["labels"])
    return torch.stack(rows).cpu().numpy(), torch.stack(labels).cpu().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)      # NaN-aware equality of float64 rows


def _assert_joint_equals_loop(b, scores, points, keep, where, frame_div=None):
    from gnn_cca_amd.calibration import sweep_joint
    rows, labels = sweep_joint(b, scores, points, keep, frame_div=frame_div, return_labels=True)
    assert rows.shape == (len(points), _g(b), 16) and rows.dtype == torch.float64
    assert labels.shape == (len(points), _n(b)) and labels.dtype == torch.int32
    assert sweep_joint(b, scores, points, keep, frame_div=frame_div).cpu().numpy().tobytes() == rows.cpu().numpy().tobytes()
    rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    want_rows, want_labels = _loop(b, scores, points, keep, frame_div)
    for t in range(len(points)):
        bad = np.argwhere(~((rows[t] == want_rows[t]) | (np.isnan(rows[t]) & np.isnan(want_rows[t]))))
        assert _same(rows[t], want_rows[t]), (where, keep, t, points[t], bad[:4])
        assert np.array_equal(labels[t], want_labels[t]), (where, keep, t)
    return rows, labels


def _pair_extreme(b, s, which):
    """A score value at which strict and non-strict comparators must differ after pruning: the larger (which='max', for le / lt) or the
    smaller (which='min', for ge / gt) of the two scores of some mutual pair -> (the float32 score widened, the pair's frame)."""
    ei = b.edge_index.cpu().numpy()
    s = s.reshape(-1).cpu().numpy().astype(np.float64)
    where = {(int(a), int(c)): k for k, (a, c) in enumerate(ei.T)}
    mutual = [(k, where[(int(c), int(a))]) for k, (a, c) in enumerate(ei.T) if a < c and (int(c), int(a)) in where]
    k, r = mutual[len(mutual) // 3]
    v = max(s[k], s[r]) if which == "max" else min(s[k], s[r])
    return float(v), int(np.searchsorted(np.asarray(b.edge_ptr), k, side="right") - 1)


@pytest.fixture(scope="module")
def base():
    """The parent test's batch: frames of 17, 0, 24, 9 (one camera: no edge) and 13 detections on 4 cameras, full-mode attributes."""
    rng = np.random.default_rng(31)
    f = _frames(rng, [17, 0, 24, 9, 13])
    starts = np.concatenate([[0], np.cumsum(f["sizes"])])
    f["id_cam"][starts[3]:starts[4]] = 1
    b = _build(f)
    ep = b.edge_ptr
    assert ep[2] == ep[1] and ep[4] == ep[3] and b.edge_index.shape[1] > 500 and b.edge_attr.shape[1] == 4
    return types.SimpleNamespace(f=f, batch=b)


def _points2(b, s0, s1, strict_family):
    """Points of a two-score sweep: below every score, above every score, a duplicate, one threshold exactly equal to a widened score
    on each axis (the other axis then holds everywhere), ordinary ones -> (points, index of the exact point on axis 0, on axis 1)."""
    a0, a1 = (np.sort(s.reshape(-1).cpu().numpy().astype(np.float64)) for s in (s0, s1))
    lo0, hi0, lo1, hi1 = a0[0] - 0.25, a0[-1] + 0.25, a1[0] - 0.25, a1[-1] + 0.25
    which = "max" if strict_family == "l" else "min"
    open0, open1 = (hi0, hi1) if strict_family == "l" else (lo0, lo1)         # a threshold under which every score passes
    e0, _ = _pair_extreme(b, s0, which)
    e1, _ = _pair_extreme(b, s1, which)
    mid0, mid1 = (a0[len(a0) // 2] + a0[len(a0) // 2 + 1]) / 2, (a1[len(a1) // 2] + a1[len(a1) // 2 + 1]) / 2
    pts = [[mid0, mid1], [lo0, lo1], [e0, open1], [hi0, hi1], [mid0, mid1], [open0, e1], [a0[len(a0) // 4] + 1e-9, a1[(3 * len(a1)) // 4]],
           [a0[(2 * len(a0)) // 3], open1]]
    return pts, 2, 5


def test_one_score_equals_sweep_thresholds(base):
    from gnn_cca_amd.calibration import sweep_joint, sweep_thresholds
    b = base.batch
    s = b.edge_attr[:, 2]
    v = np.sort(s.cpu().numpy().astype(np.float64))
    ths = [float(v[len(v) // 2]), float(v[0]) - 1.0, float(v[len(v) // 3]), float(v[-1]) + 1.0, float(v[len(v) // 2]), 0.37]
    for keep in ("ge", "le"):
        want_rows, want_labels = sweep_thresholds(b, s, ths, keep=keep, return_labels=True)
        rows, labels = sweep_joint(b, [s], [[t] for t in ths], [keep], return_labels=True)
        assert rows.cpu().numpy().tobytes() == want_rows.cpu().numpy().tobytes(), keep        # bit for bit
        assert torch.equal(labels, want_labels), keep
        assert len({float(r[:, 3].sum() + r[:, 4].sum()) for r in rows.cpu().numpy()}) >= 4   # the decisions do vary
    # T = 1, and the [K, E] form of the scores
    one = sweep_joint(b, s.contiguous().view(1, -1), [[ths[0]]], ["le"])
    assert one.cpu().numpy().tobytes() == sweep_thresholds(b, s, [ths[0]], keep="le").cpu().numpy().tobytes()


def test_two_scores_equal_the_loop_under_all_four_comparators(base):
    from gnn_cca_amd.calibration import sweep_joint
    b = base.batch
    s0, s1 = b.edge_attr[:, 0], b.edge_attr[:, 2:3]
    assert not s0.is_contiguous() and s0.stride(0) == 4 and s1.shape == (b.edge_index.shape[1], 1) and s1.stride(0) == 4
    got = {}
    for fam, keeps in (("l", (("lt", "lt"), ("le", "le"), ("lt", "le"))), ("g", (("gt", "gt"), ("ge", "ge"), ("ge", "gt")))):
        pts, x0, x1 = _points2(b, s0, s1, fam)
        for keep in keeps:
            rows, labels = _assert_joint_equals_loop(b, [s0, s1], pts, list(keep), "edge_attr[:, 0] & [:, 2]")
            got[keep] = rows
            assert _same(rows[0], rows[4])                                                    # the duplicate
            nothing, everything = (1, 3) if fam == "l" else (3, 1)
            assert rows[nothing][:, 3].sum() + rows[nothing][:, 4].sum() == 0                 # no score passes: nothing predicted
            assert rows[everything][:, 5].sum() + rows[everything][:, 6].sum() == 0           # every score passes (a symmetric list)
            # strided views and contiguous copies give the same bits
            copies = sweep_joint(b, [s0.contiguous(), s1.contiguous()], pts, list(keep))
            assert copies.cpu().numpy().tobytes() == rows.tobytes(), keep
        # a threshold exactly equal to a widened score: the strict and the non-strict comparator differ there, on each axis
        strict, loose = got[keeps[0]], got[keeps[1]]
        for x in (x0, x1):
            assert not _same(strict[x], loose[x]), (fam, x)
            assert (strict[x][:, 3] + strict[x][:, 4]).sum() < (loose[x][:, 3] + loose[x][:, 4]).sum(), (fam, x)
    # the mixed keeps differ from the pure ones only where their own strict axis is exact
    assert _same(got[("lt", "le")][5], got[("le", "le")][5]) and _same(got[("lt", "le")][2], got[("lt", "lt")][2])
    assert _same(got[("ge", "gt")][2], got[("ge", "ge")][2]) and _same(got[("ge", "gt")][5], got[("gt", "gt")][5])


def test_a_condition_that_always_holds_changes_nothing(base):
    from gnn_cca_amd.calibration import sweep_joint
    b = base.batch
    s0, s1, s3 = b.edge_attr[:, 0], b.edge_attr[:, 2], b.edge_attr[:, 3]
    v0, v1 = (np.sort(s.cpu().numpy().astype(np.float64)) for s in (s0, s1))
    one = sweep_joint(b, [s0], [[v0[len(v0) // 2]], [v0[len(v0) // 4]]], ["lt"], return_labels=True)
    two = sweep_joint(b, [s0, s3], [[v0[len(v0) // 2], 1e300], [v0[len(v0) // 4], 1e300]], ["lt", "le"], return_labels=True)
    front = sweep_joint(b, [s3, s0], [[-1e300, v0[len(v0) // 2]], [-1e300, v0[len(v0) // 4]]], ["gt", "lt"], return_labels=True)
    for other in (two, front):
        assert other[0].cpu().numpy().tobytes() == one[0].cpu().numpy().tobytes() and torch.equal(other[1], one[1])
    pair = sweep_joint(b, [s0, s1], [[v0[len(v0) // 2], v1[len(v1) // 2]]], ["lt", "ge"], return_labels=True)
    three = sweep_joint(b, [s0, s3, s1], [[v0[len(v0) // 2], 1e300, v1[len(v1) // 2]]], ["lt", "le", "ge"], return_labels=True)
    assert three[0].cpu().numpy().tobytes() == pair[0].cpu().numpy().tobytes() and torch.equal(three[1], pair[1])
    assert pair[0][0, :, 3:5].sum() < one[0][0, :, 3:5].sum()                                 # ... while a real condition does


def test_four_scores_with_mixed_comparators_equal_the_loop(base):
    b = base.batch
    cols = [b.edge_attr[:, q] for q in range(4)]
    q = [np.sort(c.cpu().numpy().astype(np.float64)) for c in cols]
    at = lambda k, frac: float(q[k][int(frac * (len(q[k]) - 1))])
    pts = [[at(0, 0.7), at(1, 0.8), at(2, 0.1), at(3, 0.9)], [at(0, 0.5), at(1, 0.5), at(2, 0.3), at(3, 0.6)],
           [at(0, 1.0), at(1, 1.0), at(2, 0.0), at(3, 1.0)], [at(0, 0.9), at(1, 0.2), at(2, 0.0), at(3, 1.0)], [at(0, 0.0), at(1, 1.0), at(2, 0.0), at(3, 1.0)]]
    rows, _ = _assert_joint_equals_loop(b, cols, pts, ["lt", "le", "ge", "le"], "four columns")
    kept = [float(r[:, 3].sum() + r[:, 4].sum()) for r in rows]
    assert kept[4] == 0 and len(set(kept)) >= 4 and kept[2] == max(kept)                      # lt the smallest score: nothing; the decisions vary
    _assert_joint_equals_loop(b, cols, pts[:2], ["gt", "ge", "lt", "gt"], "four columns, the other way round")


def test_frame_divisors(base):
    from gnn_cca_amd.calibration import sweep_joint
    b = base.batch
    g = _g(b)
    s0, s1 = b.edge_attr[:, 0], b.edge_attr[:, 2]
    v0, v1 = (np.sort(s.cpu().numpy().astype(np.float64)) for s in (s0, s1))
    rng = np.random.default_rng(3)
    # random divisors: th / div[g] by numpy in float64
    div = rng.uniform(0.3, 7.0, size=(2, g))
    pts = [[v0[len(v0) // 2] * 2.0, v1[len(v1) // 2] * 2.0], [v0[len(v0) // 3] * 0.7, v1[-1] * 9.0], [v0[-1] * 5.0, v1[len(v1) // 4] * 3.0]]
    rows, _ = _assert_joint_equals_loop(b, [s0, s1], pts, ["lt", "le"], "random divisors", frame_div=div)
    plain, _ = _assert_joint_equals_loop(b, [s0, s1], pts, ["lt", "le"], "no divisors")
    assert not _same(rows, plain)
    # powers of two, and a point whose quotient IS a score: strict and non-strict differ in that frame, and both equal the loop
    div2 = np.array([[4.0, 0.5, 2.0, 8.0, 0.25], [2.0, 2.0, 0.125, 1.0, 16.0]])
    exact, frame = _pair_extreme(b, s0, "max")
    point = [[exact * div2[0, frame], v1[-1] * 16.0 + 1.0]]
    assert point[0][0] / div2[0, frame] == exact
    lt, _ = _assert_joint_equals_loop(b, [s0, s1], point, ["lt", "le"], "power-of-two divisors, lt", frame_div=div2)
    le, _ = _assert_joint_equals_loop(b, [s0, s1], point, ["le", "le"], "power-of-two divisors, le", frame_div=div2)
    assert lt[0, frame, 3] + lt[0, frame, 4] < le[0, frame, 3] + le[0, frame, 4]
    # divisors of one are no divisors, bit for bit; [G] stands for [1, G] when K = 1
    ones = sweep_joint(b, [s0, s1], pts, ["lt", "le"], frame_div=np.ones((2, g)), return_labels=True)
    none = sweep_joint(b, [s0, s1], pts, ["lt", "le"], return_labels=True)
    assert ones[0].cpu().numpy().tobytes() == none[0].cpu().numpy().tobytes() and torch.equal(ones[1], none[1])
    flat = sweep_joint(b, [s0], [[p[0]] for p in pts], ["lt"], frame_div=div[0])
    assert flat.cpu().numpy().tobytes() == sweep_joint(b, [s0], [[p[0]] for p in pts], ["lt"], frame_div=div[:1]).cpu().numpy().tobytes()


def test_hand_made_batches():
    from gnn_cca_amd.calibration import sweep_joint
    none = np.zeros(0, np.int64)
    # frame 0: the pair (0, 1) is active in one direction only under the second score; the pair (1, 2) in both
    b = _hand_batch([(3, [0, 1, 1, 2], [1, 0, 2, 1], [1, 1, 0, 0]), (1, none, none, none), (2, [0, 1], [1, 0], [1, 1])])
    a = torch.tensor([0.1, 0.1, 0.2, 0.2, 0.3, 0.3], device="cuda")
    c = torch.tensor([0.9, 0.2, 0.8, 0.7, 0.6, 0.6], device="cuda")
    rows, labels = _assert_joint_equals_loop(b, [a, c], [[0.5, 0.5], [0.5, 0.1], [0.15, 0.5], [0.5, 0.95]], ["lt", "gt"], "one direction only")
    assert labels.tolist() == [[0, 1, 1, 3, 4, 4], [0, 0, 0, 3, 4, 4], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]]
    assert rows[0][0, 3] + rows[0][0, 4] == 2 and rows[1][0, 3] + rows[1][0, 4] == 4 and rows[0][0, 5] == 2    # (0, 1): not kept, both ways
    # a NaN score is never active, under all four comparators, on either axis
    rng = np.random.default_rng(9)
    b = _hand_batch([_random_frame(rng, 30, 200), _random_frame(rng, 11, 60)])
    e = b.edge_index.shape[1]
    s0 = torch.from_numpy(rng.random(e).astype(np.float32)).cuda()
    s1 = torch.from_numpy(rng.random(e).astype(np.float32)).cuda()
    s0[::5] = float("nan")
    s1[3::7] = float("nan")
    ei = b.edge_index.cpu().numpy()
    for keep, pts in ((["ge", "le"], [[0.0, 1.0], [0.4, 0.7]]), (["gt", "lt"], [[-1.0, 2.0], [0.4, 0.7]]), (["le", "ge"], [[1.0, 0.0]]),
                      (["lt", "gt"], [[2.0, -1.0]])):
        rows, labels = _assert_joint_equals_loop(b, [s0, s1], pts, keep, "NaN scores")
        nan_edge = (torch.isnan(s0) | torch.isnan(s1)).cpu().numpy()
        # every other edge passes at the first point: what is missing from the predictions is the NaN edges and their reverse edges
        kept = jo.kept_edges(ei, b.edge_ptr, ~nan_edge)
        assert (rows[0][:, 3] + rows[0][:, 4]).sum() == kept.sum() < e - nan_edge.sum()
    # a frame whose node range runs past the batch on the device: a NaN row, its labels not written, the other frames unaffected
    good_rows, good_labels = sweep_joint(b, [s0, s1], [[0.4, 0.7], [0.1, 0.9]], ["ge", "le"], return_labels=True)
    honest = b.node_ptr_dev
    bad = list(b.node_ptr)
    bad[2] += 5
    b.node_ptr_dev = torch.tensor(bad, dtype=torch.int32).cuda()
    rows, labels = sweep_joint(b, [s0, s1], [[0.4, 0.7], [0.1, 0.9]], ["ge", "le"], return_labels=True)
    b.node_ptr_dev = honest
    rows, good_rows = rows.cpu().numpy(), good_rows.cpu().numpy()
    assert np.isnan(rows[:, 1]).all() and not np.isnan(rows[:, 0]).any() and rows[:, 0].tobytes() == good_rows[:, 0].tobytes()
    assert torch.equal(labels[:, :30], good_labels[:, :30])


def test_sizes_where_the_workgroup_loops_change():
    from gnn_cca_amd.calibration import MAX_POINTS, sweep_joint
    rng = np.random.default_rng(12)
    # one wave per frame (at most 64 nodes), then four; 65 and 257 detections: one past the wave and the block strides
    for sizes, where in (((1, 2, 64), "1, 2, 64"), ((65,), "65"), ((257, 2), "257, 2")):
        b = _hand_batch([_random_frame(rng, n, 6 * n) for n in sizes])
        e = b.edge_index.shape[1]
        s0 = torch.from_numpy(rng.random(e).astype(np.float32)).cuda()
        s1 = torch.from_numpy(rng.random(e).astype(np.float32)).cuda()
        rows, labels = _assert_joint_equals_loop(b, [s0, s1], [[0.2, 0.9]], ["ge", "lt"], where + ", T = 1")
        assert rows[0][:, 3:5].sum() > 0 and rows[0][:, 15].sum() < sum(sizes)                # edges are kept and nodes do merge
        _assert_joint_equals_loop(b, [s0, s1], [[0.0, 1.0], [0.6, 0.5], [0.05, 0.97]], ["ge", "le"], where)
    # the grid limit: 16384 points on one frame of two nodes
    b = _hand_batch([(2, [0, 1], [1, 0], [1, 1])])
    s = torch.tensor([0.5, 0.5], device="cuda")
    pts = np.linspace(0.0, 1.0, MAX_POINTS).reshape(-1, 1)
    rows, labels = sweep_joint(b, [s], pts, ["ge"], return_labels=True)
    assert rows.shape == (MAX_POINTS, 1, 16) and labels.shape == (MAX_POINTS, 2)
    rows, labels = rows.cpu().numpy(), labels.cpu().numpy()
    want, want_labels = _loop(b, [s], [[0.25], [0.75]], ["ge"])
    on = pts[:, 0] <= 0.5
    assert 0 < on.sum() < MAX_POINTS and on[0] and not on[-1]
    assert (rows[on] == want[0]).all() and (rows[~on] == want[1]).all() and not _same(want[0], want[1])
    assert (labels[on] == want_labels[0]).all() and (labels[~on] == want_labels[1]).all()
    with pytest.raises(ValueError, match="at most 16384"):
        sweep_joint(b, [s], np.linspace(0.0, 1.0, MAX_POINTS + 1).reshape(-1, 1), ["ge"])


def test_golden_geometry_and_appearance():
    from gnn_cca_amd.calibration import sweep_grid, sweep_joint
    z = np.load(GOLDEN)
    ei, n = z["edge_index"], int(z["n_nodes"])
    b = _hand_batch([(n, ei[0], ei[1], z["edge_labels"])])
    geom, reid = torch.from_numpy(z["geom"]).cuda(), torch.from_numpy(z["reid"]).cuda()
    geom_th, max_dist, reid_th = float(z["geom_th"]), float(z["max_dist"]), float(z["reid_th"])
    lab = z["edge_labels"]
    tol = {8: 1e-8, 9: 1e-12, 10: 1e-12, 11: 1e-12}                     # tests/test_gpu_evaluation.py's
    for scores, points, keep, div, name in (([geom, reid], [[geom_th, reid_th]], ["lt", "lt"], [[max_dist], [1.0]], "joint"),
                                            ([geom], [[geom_th]], ["lt"], [max_dist], "geom")):
        rows, labels = sweep_joint(b, scores, points, keep, frame_div=div, return_labels=True)
        row, labels = rows.cpu().numpy()[0, 0], labels.cpu().numpy()[0]
        pred, want = z[f"pred_{name}"], z[f"scores_{name}"]
        assert row[3] == ((pred == 1) & (lab == 1)).sum() and row[4] == ((pred == 1) & (lab == 0)).sum(), name
        assert row[5] == ((pred == 0) & (lab == 1)).sum() and row[6] == ((pred == 0) & (lab == 0)).sum(), name
        pairs = set(zip(labels.tolist(), z[f"id_pred_{name}"].tolist()))
        assert len(pairs) == len(set(labels.tolist())) == len(set(z[f"id_pred_{name}"].tolist())), name   # the reference's partition
        assert row[7] == want[0], (name, row[7], want[0])                                                 # ARI: exact
        for q in (8, 9, 10, 11):
            assert abs(row[q] - want[q - 7]) <= tol[q], (name, q, row[q], want[q - 7])
        assert row[14] == len(set(z["id_gt"].tolist())) and row[15] == len(set(z[f"id_pred_{name}"].tolist()))
    # the grid: rows viewed [T1, T2, G, 16], the golden's point among them, C order
    axes = [[1.0, geom_th, 5.0], [0.2, reid_th]]
    grid, glab = sweep_grid(b, [geom, reid], axes, ["lt", "lt"], frame_div=[[max_dist], [1.0]], return_labels=True)
    assert grid.shape == (3, 2, 1, 16) and glab.shape == (3, 2, n)
    at = sweep_joint(b, [geom, reid], [[geom_th, reid_th]], ["lt", "lt"], frame_div=[[max_dist], [1.0]])
    assert grid[1, 1].cpu().numpy().tobytes() == at[0].cpu().numpy().tobytes()
    flat = sweep_joint(b, [geom, reid], [[x, y] for x in axes[0] for y in axes[1]], ["lt", "lt"], frame_div=[[max_dist], [1.0]])
    assert grid.reshape(6, 1, 16).cpu().numpy().tobytes() == flat.cpu().numpy().tobytes()


def test_geometry_baseline_is_the_sweep_it_stands_for(base):
    from gnn_cca_amd.baselines import geometry_baseline
    from gnn_cca_amd.calibration import sweep_joint
    b, md = base.batch, base.f["max_dist"]
    g = _g(b)
    geom_th = float(np.median(b.edge_attr[:, 0].cpu().numpy().astype(np.float64) * np.repeat(md, np.diff(b.edge_ptr))))   # metres
    reid_th, l2 = 0.8, float(b.edge_attr[:, 2].max().item())
    rows = geometry_baseline(b, geom_th, md)
    want = sweep_joint(b, [b.edge_attr[:, 0]], [[geom_th]], ["lt"], frame_div=md.reshape(1, g))
    assert rows.shape == (g, 16) and rows.cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()
    both = geometry_baseline(b, geom_th, md, reid_th=reid_th, max_dist_l2=l2)
    want = sweep_joint(b, [b.edge_attr[:, 0], b.edge_attr[:, 2]], [[geom_th, reid_th * l2]], ["lt", "lt"], frame_div=np.stack([md, np.ones(g)]))
    assert both.cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()
    _assert_joint_equals_loop(b, [b.edge_attr[:, 0], b.edge_attr[:, 2]], [[geom_th, reid_th * l2]], ["lt", "lt"], "the baseline's call",
                              frame_div=np.stack([md, np.ones(g)]))
    kept, kept_both = rows[:, 3:5].sum().item(), both[:, 3:5].sum().item()
    assert 0 < kept_both < kept < b.edge_index.shape[1]
    assert geometry_baseline(b, geom_th, md, reid_th=reid_th).cpu().numpy().tobytes() == sweep_joint(
        b, [b.edge_attr[:, 0], b.edge_attr[:, 2]], [[geom_th, reid_th]], ["lt", "lt"], frame_div=np.stack([md, np.ones(g)]))[0].cpu().numpy().tobytes()


def test_accumulator_over_three_batches_and_determinism(base, monkeypatch):
    from gnn_cca_amd.calibration import JointSweepAccumulator, SweepAccumulator, grid_points, sweep_grid
    rng = np.random.default_rng(77)
    batches = [base.batch, _build(_frames(rng, [12, 20, 5, 16, 8, 21, 3])), _build(_frames(rng, [30, 7]))]
    axes = [[0.05, 0.2, 0.5, 2.0], [0.5, 4.0, 7.0]]
    pts, shape = grid_points(axes)
    t = len(pts)

    def run():
        acc = JointSweepAccumulator(pts)
        kept = []
        for b in batches:
            rows = sweep_grid(b, [b.edge_attr[:, 0], b.edge_attr[:, 2]], axes, ["lt", "lt"])
            assert rows.shape == (*shape, _g(b), 16)
            acc.add(rows)
            kept.append(rows.reshape(t, _g(b), 16))
        return acc, kept

    calls = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(1), real_cpu(self, *a, **k))[1])
    acc, kept = run()
    assert not calls                                                         # nothing was copied to the host so far
    res = acc.result()
    assert len(calls) == 1 and acc.result() is res and len(calls) == 1        # the one synchronisation
    monkeypatch.undo()
    host = [r.cpu().numpy() for r in kept]
    assert not any(np.isnan(h).any() for h in host)
    frames = sum(_g(b) for b in batches)
    sums, count, means = jo.accumulator_result(host)
    assert res["frames"] == count == frames == 14 and np.array_equal(res["points"], pts)
    assert res["sums"].tobytes() == sums.tobytes()                           # the contract's order: bit for bit
    sweep = SweepAccumulator(np.arange(t, dtype=np.float64))
    for r in kept:
        sweep.add(r)
    ref = sweep.result()
    cols = {"P": 0, "R": 1, "F": 2, "RI": 7, "MI": 8, "hom": 9, "com": 10, "v": 11, "prec0": 12, "prec1": 13}
    for p in range(t):
        got, want = res["aggregates"][p], ref["aggregates"][p]
        assert sorted(got) == sorted(want)
        for name, col in cols.items():
            assert got[name] == means[p, col], (p, name)                     # sum / frames, divided on the host in float64
            bound = frames * 2.0 ** -52 * max(1.0, abs(sums[p, col]))          # recursive summation of F terms, in either order
            assert abs(got[name] - want[name]) <= bound, (p, name, got[name], want[name], bound)
        for name, col in (("TP", 3), ("FP", 4), ("FN", 5), ("TN", 6)):
            assert got[name] == want[name] == int(sums[p, col]) and isinstance(got[name], int), (p, name)
    for name in ("TP", "FP", "FN", "TN", "P_micro", "R_micro", "F_micro"):
        assert np.array_equal(res[name], ref[name]) and res[name].dtype == ref[name].dtype, name
    assert len(set(res["TP"].tolist())) >= 4 and res["F_micro"].max() > 0
    assert np.array_equal(acc.best(), sweep.best()) and np.array_equal(acc.best("TN"), sweep.best("TN"))
    with pytest.raises(ValueError):
        acc.best("accuracy")
    # two runs give the same bits: the rows, and the sums
    acc2, kept2 = run()
    for a, b2 in zip(kept, kept2):
        assert a.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes()
    assert acc2.result()["sums"].tobytes() == res["sums"].tobytes()
