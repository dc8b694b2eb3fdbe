"""The ranking scores on the MI355X (csrc/rank_metrics.cuh: ranking.rank_metrics / RankMeter / PooledCurve, FrameResult.rank_metrics)
against the numpy restatement of their rule (tests/rank_metrics_oracle.py), bit for bit in all eight columns (NaN where the oracle has
NaN); and the pooled curve against the reference's own sweep (tests/golden/calibration/reid_sweep.npz, main.py:141-175)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rank_metrics_oracle as ro  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "calibration", "reid_sweep.npz")


def _hand_batch(frames):
    """frames: list of label arrays, one per frame (an edge per label, between the frame's two nodes) -> a GraphBatch as
    evaluate_frames takes it."""
    from gnn_cca_amd.sharding import GraphBatch
    node_ptr, edge_ptr, ei, lab = [0], [0], [np.zeros((2, 0), np.int64)], [np.zeros(0, np.float32)]
    for l in frames:
        v0 = node_ptr[-1]
        src = np.arange(len(l), dtype=np.int64) % 2
        ei.append(np.stack([src + v0, 1 - src + v0]).reshape(2, -1))
        lab.append(np.asarray(l, np.float32))
        node_ptr.append(v0 + 2)
        edge_ptr.append(edge_ptr[-1] + len(l))
    b = GraphBatch(None, torch.from_numpy(np.concatenate(ei, axis=1)).cuda(), None, edge_ptr, node_ptr)
    b.edge_labels = torch.from_numpy(np.concatenate(lab)).cuda()
    b.node_ptr_dev = torch.tensor(node_ptr, dtype=torch.int32).cuda()
    b.edge_ptr_dev = torch.tensor(edge_ptr, dtype=torch.int32).cuda()
    return b


def _same_bits(got, want):
    """Equal bit for bit where the oracle has a number (a zero's sign included), NaN where it has NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def _where(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in np.argwhere(bad)[:6]]


def _labels(rng, sizes, all_pos=(), all_neg=()):
    out = []
    for j, e in enumerate(sizes):
        l = (rng.random(e) < 0.3).astype(np.float32)
        if j in all_pos:
            l[:] = 1.0
        if j in all_neg:
            l[:] = 0.0
        out.append(l)
    return out


def _check(b, scores, positive, where):
    from gnn_cca_amd.ranking import rank_metrics
    rows = rank_metrics(b, [torch.from_numpy(s).cuda() for s in scores], positive)
    again = rank_metrics(b, [torch.from_numpy(s).cuda() for s in scores], positive)
    g = len(b.edge_ptr) - 1
    assert rows.shape == (len(scores), g, 8) and rows.dtype == torch.float64 and rows.is_cuda
    rows = rows.cpu().numpy()
    assert rows.tobytes() == again.cpu().numpy().tobytes(), where                       # two runs: the same bits
    low = [p == "low" for p in ([positive] * len(scores) if isinstance(positive, str) else positive)]
    want = ro.rank_rows(scores, b.edge_labels.cpu().numpy(), b.edge_ptr, low)
    assert _same_bits(rows, want), (where, _where(rows, want))
    return rows


# the sizes at which the sort or the scans can go wrong, grouped so that the batch's largest frame selects each of the three LDS
# capacities (1024, 4096, 16384 words); (sizes, frames of only positives, frames of only negatives)
BATCHES = {"1024": ((0, 1, 2, 63, 64, 65, 1023, 1024, 300, 700, 1), (8, 10), (9,)),
           "4096": ((1025, 4096, 2, 2500, 1500, 0), (3,), (4,)),
           "16384": ((4097, 16380, 65, 16384, 0, 9000, 5000), (5,), (6,))}


@pytest.mark.parametrize("name", list(BATCHES))
def test_rows_equal_the_oracle_at_every_capacity(name):
    from gnn_cca_amd import _native as nat
    sizes, all_pos, all_neg = BATCHES[name]
    rng = np.random.default_rng(len(name) + sum(sizes))
    b = _hand_batch(_labels(rng, sizes, all_pos, all_neg))
    e = int(sum(sizes))
    assert nat.lib().gnncca_rank_metrics_lds_bytes(max(sizes)) == 8 * int(name)
    cont = (rng.standard_normal(e) + 0.8 * b.edge_labels.cpu().numpy()).astype(np.float32)
    five = rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 2.0], dtype=np.float32), size=e)             # heavy ties, +0 and -0 among them
    equal = np.full(e, 0.25, dtype=np.float32)
    near = (np.float32(1.0) + rng.integers(0, 9, size=e).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    rows = _check(b, [cont, five, equal, near], ["high", "low", "high", "low"], name)
    ptr = np.asarray(b.edge_ptr)
    for j, n in enumerate(sizes):
        assert rows[0, j, 0] + rows[0, j, 1] == n and rows[2, j, 2] == min(n, 1) and rows[1, j, 2] <= 4
        if n >= 1000 and j not in all_pos + all_neg:
            assert 0.6 < rows[0, j, 4] < 0.9 and rows[2, j, 4] == 0.5 and rows[0, j, 2] > 0.99 * n, (j, rows[:, j])
    for j in all_pos:
        assert rows[0, j, 1] == 0 and np.isnan(rows[0, j, 4]) and rows[0, j, 6] == 1.0 and abs(rows[0, j, 5] - 1.0) < 1e-12
    for j in all_neg:
        assert rows[0, j, 0] == 0 and np.isnan(rows[0, j, 4:]).all()
    # +-inf are ordinary values; one NaN (in every second frame that has an edge) takes the frame's four real-valued columns
    inf = cont.copy()
    inf[rng.random(e) < 0.1] = np.inf
    inf[rng.random(e) < 0.1] = -np.inf
    nan = cont.copy()
    hit = [j for j, n in enumerate(sizes) if n > 0][::2]
    for j in hit:
        nan[ptr[j] + (sizes[j] * 2) // 3] = np.nan
    rows = _check(b, [inf, nan], "high", name + ", inf / NaN")
    _check(b, [inf, nan], ["low", "low"], name + ", inf / NaN, low")
    for j, n in enumerate(sizes):
        assert rows[1, j, 3] == (j in hit), j
        if j in hit:
            assert np.isnan(rows[1, j, 4:]).all() and rows[1, j, 0] + rows[1, j, 1] == n, j
        elif n >= 63 and j not in all_neg:
            assert not np.isnan(rows[1, j, 5:]).any(), j
    # a label that is neither 0 nor 1 is no sample
    odd = b.edge_labels.clone()
    odd[::7] = 2.0
    keep = b.edge_labels
    b.edge_labels = odd
    rows = _check(b, [cont], "high", name + ", labels of 2")
    b.edge_labels = keep
    assert rows[0, :, :2].sum() == e - len(range(0, e, 7))


def test_four_strided_scores_with_mixed_directions_equal_single_calls():
    from gnn_cca_amd.graph_build import build_graph_batch
    from gnn_cca_amd.ranking import rank_metrics
    rng = np.random.default_rng(31)
    sizes = np.asarray([17, 0, 24, 9, 13])
    n = int(sizes.sum())
    b = build_graph_batch(rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.integers(0, 11, size=n), rng.integers(0, 4, size=n), sizes,
                          rng.uniform(10, 90, len(sizes)), torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32)).cuda(),
                          torch.from_numpy(rng.standard_normal((n, 16)).astype(np.float32)).cuda())
    assert b.edge_attr.shape[1] == 4 and b.edge_index.shape[1] > 500
    cols = [b.edge_attr[:, q] for q in range(4)]
    assert all(not c.is_contiguous() and c.stride(0) == 4 for c in cols)
    positive = ["low", "high", "low", "low"]
    rows = rank_metrics(b, cols, positive)
    host = rows.cpu().numpy()
    want = ro.rank_rows([c.cpu().numpy() for c in cols], b.edge_labels.cpu().numpy(), b.edge_ptr, [p == "low" for p in positive])
    assert _same_bits(host, want), _where(host, want)
    for q in range(4):
        one = rank_metrics(b, cols[q].contiguous(), positive[q])
        assert one.shape == (1, len(sizes), 8) and _same_bits(one.cpu().numpy()[0], host[q]), q
        assert _same_bits(rank_metrics(b, b.edge_attr[:, q:q + 1], positive[q]).cpu().numpy()[0], host[q]), q      # [E, 1] with a row stride
    # a distance ranked the wrong way round: AUROC mirrors, exactly where no rounding is involved (the integer numerators add up)
    flipped = rank_metrics(b, cols[0], "high").cpu().numpy()[0]
    ok = ~np.isnan(host[0][:, 4])
    assert ok.sum() >= 3 and np.allclose(flipped[ok, 4] + host[0][ok, 4], 1.0, atol=1e-15) and np.array_equal(flipped[:, :4], host[0][:, :4])


def test_frame_result_rank_metrics_and_the_meter_over_three_batches(monkeypatch):
    import bench
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.ranking import RankMeter, rank_metrics
    rng = np.random.default_rng(17)
    m = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).cuda().eval()

    def frames(sizes, cams):
        sizes = np.asarray(sizes)
        n = int(sizes.sum())
        return ((rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.integers(0, 11, size=n), rng.integers(0, cams, size=n), sizes,
                 rng.uniform(10, 90, len(sizes))), torch.from_numpy(rng.standard_normal((n, 2048)).astype(np.float32)).cuda(),
                torch.from_numpy(rng.standard_normal((n, 256)).astype(np.float32)).cuda())

    data = [frames([12, 25, 4, 0, 18], 3), frames([9, 22, 4, 15, 11, 30], 4), frames([7, 16], 3)]
    results = [FramePipeline(m)(*a, node, reid) for a, node, reid in data[:2]] + [FramePipeline(m, top_k=3)(*data[2][0], *data[2][1:])]
    calls = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(1), real_cpu(self, *a, **k))[1])
    meter, kept = RankMeter(), []
    for r in results:
        rows = r.rank_metrics()
        meter.add(rows)
        kept.append(rows)
    assert not calls                                                                    # nothing was copied to the host so far
    res = meter.result()
    assert len(calls) == 1 and meter.result() is res and len(calls) == 1                 # the one synchronisation
    monkeypatch.undo()
    host = []
    for r, rows in zip(results, kept):
        b = r.batch
        assert rows.shape == (1, len(b.edge_ptr) - 1, 8)
        assert rows.cpu().numpy().tobytes() == rank_metrics(b, r.probs, "high").cpu().numpy().tobytes()
        want = ro.rank_rows([r.probs.reshape(-1).cpu().numpy()], b.edge_labels.cpu().numpy(), b.edge_ptr, [False])
        assert _same_bits(rows.cpu().numpy(), want), _where(rows.cpu().numpy(), want)
        host.append(rows.cpu().numpy())
    assert host[2][0, :, :2].sum() == results[2].batch.edge_index.shape[1] <= 3 * (7 + 16)         # the capped batch: its kept edges
    sums, counts = ro.meter_fold(host)
    assert res["sums"].tobytes() == sums.tobytes() and np.array_equal(res["frames"], counts)        # the contract's order: bit for bit
    assert counts[0, 0] == 13 and 0 < counts[0, 4] < 13                                  # the empty frame: counted for the counts only
    with np.errstate(invalid="ignore"):
        assert _same_bits(res["means"], sums / counts)
    # two meters over the same rows: the same bits; rows of another K are refused
    again = RankMeter()
    for rows in kept:
        again.add(rows)
    assert again.result()["sums"].tobytes() == res["sums"].tobytes()
    with pytest.raises(ValueError, match="after rows of 1"):
        again.add(torch.zeros((2, 3, 8), dtype=torch.float64, device="cuda"))


def _curve_equals_golden(res, z):
    for name in ("TP", "FP", "FN", "TN"):
        assert np.array_equal(res[name], z[name]) and res[name].dtype == np.int64, name
    for name in ("P", "R", "F"):
        assert res[name].tobytes() == np.asarray(z[name], dtype=np.float64).tobytes(), name            # bit for bit


def test_pooled_curve_reproduces_the_reference_sweep():
    from gnn_cca_amd.ranking import PooledCurve
    z = np.load(GOLDEN)
    s, lab = torch.from_numpy(z["scores"]).cuda(), torch.from_numpy(z["edge_labels"].astype(np.float32)).cuda()
    e = s.numel()
    one = PooledCurve(z["thresholds"], keep="le").add_raw(s, lab)
    res = one.result()
    _curve_equals_golden(res, z)
    assert np.array_equal(one.best("F"), np.where(z["F"] == np.max(z["F"]))[0]) and one.n_nan == (0, 0)
    cut = PooledCurve(z["thresholds"], keep="le")
    for a, c in ((0, e // 3), (e // 3, e // 3 + 1), (e // 3 + 1, e)):                              # the same data in three calls
        cut.add_raw(s[a:c], lab[a:c])
    _curve_equals_golden(cut.result(), z)
    assert np.array_equal(cut.histograms()[0], one.histograms()[0])
    want = ro.pooled_rows(ro.pooled_histograms(z["scores"], z["edge_labels"], z["thresholds"], "le")[0], "le")
    assert res["AUROC"] == want["AUROC"] and res["AP"] == want["AP"] and 0.0 <= res["AP"] <= 1.0
    # through a batch, with a strided score; a NaN is counted apart and result() refuses
    b = _hand_batch([z["edge_labels"][:100], z["edge_labels"][100:]])
    wide = torch.stack([s, s + 1.0], dim=1)
    _curve_equals_golden(PooledCurve(z["thresholds"]).add(b, wide[:, 0]).result(), z)
    bad = s.clone()
    bad[5] = float("nan")
    spoiled = PooledCurve(z["thresholds"]).add_raw(bad, lab)
    with pytest.raises(ValueError, match="NaN score"):
        spoiled.result()
    assert sum(spoiled.n_nan) == 1 and spoiled.histograms()[0].sum() == e - 1


def test_pooled_curve_with_65536_thresholds_equals_the_oracle():
    from gnn_cca_amd.ranking import PooledCurve
    rng = np.random.default_rng(50)
    e, t = 50_000, 65536
    lab = (rng.random(e) < 0.2).astype(np.float32)
    s = (rng.standard_normal(e) + 0.9 * lab).astype(np.float32)
    th = np.unique(rng.uniform(-4.0, 5.0, size=t).astype(np.float32)).astype(np.float64)           # float32 values: a score can BE a threshold
    th = np.concatenate([th, th[-1] + 1.0 + np.arange(t - len(th))])                               # (strictly increasing, 65536 of them)
    s[::97] = np.float32(th[1000])
    s[1::97] = np.float32(th[40_000])
    assert len(th) == t and (np.diff(th) > 0).all() and np.float64(s[0]) == th[1000]
    curve = PooledCurve(th, keep="ge").add_raw(torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda())
    hist, nans = ro.pooled_histograms(s, lab, th, "ge")
    got_hist, got_nans = curve.histograms()
    assert np.array_equal(got_hist, hist) and got_nans == nans == (0, 0)
    want, res = ro.pooled_rows(hist, "ge"), curve.result()
    assert res["AUROC"] == want["AUROC"] and res["AP"] == want["AP"] and 0.6 < res["AUROC"] < 0.9  # bit for bit
    for name in ("TP", "FP", "FN", "TN", "P", "R", "F"):
        assert res[name].tobytes() == want[name].tobytes(), name
    k = 30_000
    pred = s.astype(np.float64) >= th[k]
    assert res["TP"][k] == (pred & (lab == 1)).sum() and res["FP"][k] == (pred & (lab == 0)).sum()
