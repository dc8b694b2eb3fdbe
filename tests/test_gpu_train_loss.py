"""gnn_cca_amd.loss on the MI355X: the EdgeLoss kernels (csrc/loss.hip) against the reference's own compute_loss_acc (golden
tests/golden/post2_train_loss.npz, make_golden_loss.py) and against torch autograd of the restatement (tests/helpers/loss_oracle.py) on
2^21 edges; determinism; a whole training iteration with EdgeLoss + TrainMeters captured into a HIP graph; the layer-by-layer engine
with the focal criterion; the documented results and errors at the edges (no edge, CPU tensors, mismatched labels)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from test_backward_oracle import load_bwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import loss_oracle as lo  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "post2_train_loss.npz")
CRITERIA = (("BCE", None), ("BCE_weighted", 4.5), ("BCE_weighted", 9.0), ("Focal", None))


class Data:
    pass


def run_kernel(x_np, y_np, criterion, pos_weight, mode="train", meters=None):
    """EdgeLoss on the [S, E, 1] buffer's unbind (the MPN's layout), backward with g = 1 -> (loss, record, grad [S, E])."""
    from gnn_cca_amd.loss import EdgeLoss
    s, e = x_np.shape
    base = torch.from_numpy(x_np.copy()).cuda().view(s, e, 1).requires_grad_(True)
    fn = EdgeLoss(criterion, pos_weight=pos_weight, mode=mode, meters=meters)
    loss = fn({"classified_edges": list(base.unbind(0))}, torch.from_numpy(y_np.astype(np.float32)).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), fn.last.record.cpu().numpy(), base.grad.view(s, e).cpu().numpy(), fn


def test_kernel_matches_every_golden_case():
    z = np.load(GOLDEN)
    n = 0
    for key, c in lo.golden_cases(z):
        loss, rec, grad, _ = run_kernel(c["x"], c["y"], c["criterion"], c["pos_weight"], c["mode"])
        s = c["x"].shape[0]
        st = c["stats"]
        assert lo.close([rec[0], rec[1], rec[2]], [st[0], st[4], st[5]]), (key, rec[:8], st)
        assert lo.close([float(loss)], [st[0]]), key
        assert rec[3] == st[1] and rec[4] == st[2] and rec[5] == st[3], (key, rec[3:6], st[1:4])   # precisions: bit for bit
        y = c["y"]
        assert rec[6] == np.sum(y == 1) and rec[7] == np.sum(y == 0), key
        assert lo.close(rec[8:8 + 2 * s].reshape(s, 2), c["mean_prob"]), (key, rec[8:8 + 2 * s], c["mean_prob"])
        if c["grad"] is not None:
            want = c["grad"]
            assert np.array_equal(np.isnan(grad), np.isnan(want)), key
            if want.size:
                assert np.nanmax(np.abs(grad - want)) <= 1e-6 * float(np.nanmax(np.abs(want))), (key, np.nanmax(np.abs(grad - want)))
        n += 1
    assert n == 80


@pytest.mark.parametrize("criterion,pos_weight", CRITERIA)
def test_large_random_against_autograd_of_the_restatement(criterion, pos_weight):
    from gnn_cca_amd.loss import EdgeLoss
    g = torch.Generator(device="cuda").manual_seed(7)
    s, e = 3, 1 << 21
    x = (3.0 * torch.randn(s, e, 1, device="cuda", generator=g)).requires_grad_(True)
    y = (torch.rand(e, device="cuda", generator=g) < 0.15).float()
    fn = EdgeLoss(criterion, pos_weight=pos_weight)
    loss = fn({"classified_edges": list(x.unbind(0))}, y)
    (2.5 * loss).backward()
    xr = x.detach().view(s, e).clone().requires_grad_(True)
    r = lo.edge_loss(xr, y, criterion, pos_weight)
    (2.5 * r["loss"]).backward()
    rec = fn.last.record.cpu().numpy()
    assert lo.close([rec[0], rec[1], rec[2]], [float(r["loss"].detach()), r["loss_class1"], r["loss_class0"]], rtol=1e-6), rec[:3]
    assert (rec[3], rec[4], rec[5]) == (r["precision1"], r["precision0"], r["precision"])
    assert (rec[6], rec[7]) == (r["n_pos"], r["n_neg"])
    assert lo.close(rec[8:8 + 2 * s].reshape(s, 2), r["mean_prob"], rtol=1e-9)
    assert lo.close(rec[8 + 2 * s:], r["coef"], rtol=1e-6)   # per-edge terms differ from torch's by ulps
    gk, gr = x.grad.view(s, e), xr.grad.float()
    assert float((gk - gr).abs().max()) <= 1e-6 * float(gr.abs().max())


def test_two_calls_are_bitwise_identical():
    g = torch.Generator().manual_seed(3)
    x = (2.0 * torch.randn(3, 300_001, generator=g)).numpy()
    y = (torch.rand(300_001, generator=g) < 0.3).float().numpy()
    for crit, pw in CRITERIA:
        a = run_kernel(x, y, crit, pw)
        b = run_kernel(x, y, crit, pw)
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[0].numpy().tobytes() == b[0].numpy().tobytes()


def _setup():
    from gnn_cca_amd import MOTMPNet
    params, arch, sd, _, _, a = load_bwd("terrace32")
    m = MOTMPNet(copy.deepcopy(params), None, arch)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.cuda().train()
    d = Data()
    d.x, d.edge_index, d.edge_attr = (torch.from_numpy(a[k]).cuda() for k in ("x", "edge_index", "edge_attr"))
    labels = torch.from_numpy(np.asarray(a["labels"])).cuda().float()
    return m, d, labels, int(a["n_logits"])


def test_graphed_step_with_edge_loss_and_meters():
    from gnn_cca_amd.training import EdgeLoss, GraphedTrainStep, TrainMeters
    m1, d, labels, n_steps = _setup()
    m2, _, _, _ = _setup()
    m3, _, _, _ = _setup()
    o1, o2, o3 = (torch.optim.SGD(m.parameters(), lr=0.05) for m in (m1, m2, m3))
    meters = TrainMeters(capacity=16, n_steps=n_steps)
    step = GraphedTrainStep(m2, o2, EdgeLoss("BCE", meters=meters), warmup=2)
    eager = EdgeLoss("BCE")
    crit = torch.nn.BCEWithLogitsLoss()
    lam = lambda out, lab: sum(crit(t.view(-1), lab) for t in out["classified_edges"])  # noqa: E731
    rng = np.random.default_rng(0)
    l1, l2, l3, recs = [], [], [], []
    for it in range(7):  # 2 eager warm-ups, 1 captured, 4 replayed -- a different batch every time
        d.edge_attr = torch.from_numpy(rng.random(tuple(d.edge_attr.shape)).astype(np.float32)).cuda()
        o1.zero_grad()
        loss = eager(m1(d), labels)
        loss.backward()
        o1.step()
        l1.append(float(loss))
        recs.append(eager.last.record.cpu().numpy().copy())
        o3.zero_grad()
        loss3 = lam(m3(d), labels)
        loss3.backward()
        o3.step()
        l3.append(float(loss3))
        l2.append(float(step(d, labels)))
    assert len(step._graphs) == 1
    assert np.allclose(l1, l2, rtol=2e-5, atol=1e-6), (l1, l2)
    assert np.allclose(l1, l3, rtol=2e-5, atol=1e-6), (l1, l3)
    assert l1[-1] < l1[0]
    for (k, p1), (_, p2), (_, p3) in zip(m1.state_dict().items(), m2.state_dict().items(), m3.state_dict().items()):
        assert torch.allclose(p1.float(), p2.float(), rtol=1e-4, atol=1e-6), k
        assert torch.allclose(p1.float(), p3.float(), rtol=1e-4, atol=1e-6), k
    rows, overflow = meters.rows()
    assert not overflow and rows.shape[0] == 7
    for i in range(7):   # the eager EdgeLoss and the graphed one see the same weights up to the tolerance above: compare what is exact
        assert lo.close(rows[i][:3], recs[i][:3], rtol=1e-4), (i, rows[i][:8], recs[i][:8])
        assert rows[i][6] == recs[i][6] and rows[i][7] == recs[i][7]
    res = meters.result(batch_size=64)
    assert res["iterations"] == 7 and res["loss"]["count"] == 7 * 64
    assert res["loss"]["values"] == [float(np.float32(v)) for v in rows[:, 0]]
    meters.reset()
    step(d, labels)   # a replay after reset() writes row 0 again
    rows, overflow = meters.rows()
    assert rows.shape[0] == 1 and not overflow


def test_graphed_meters_rows_equal_the_eager_records_bitwise():
    """The same batches through the same weights: the rows a replayed graph appends are bit for bit the records of eager calls."""
    from gnn_cca_amd.loss import EdgeLoss, TrainMeters
    s, e = 3, 768
    x = torch.zeros(s, e, 1, device="cuda")
    y = torch.zeros(e, device="cuda")
    meters = TrainMeters(capacity=4, n_steps=s)
    fn = EdgeLoss("Focal", meters=meters)
    eager = EdgeLoss("Focal")
    rng = np.random.default_rng(1)
    batches = [((3 * rng.standard_normal((s, e, 1))).astype(np.float32), (rng.random(e) < 0.2).astype(np.float32)) for _ in range(6)]
    x.copy_(torch.from_numpy(batches[0][0]))
    y.copy_(torch.from_numpy(batches[0][1]))
    fn({"classified_edges": list(x.unbind(0))}, y)   # warm-up: row 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn({"classified_edges": list(x.unbind(0))}, y)
    want = []
    for xb, yb in batches[:3]:
        x.copy_(torch.from_numpy(xb))
        y.copy_(torch.from_numpy(yb))
        graph.replay()
        eager({"classified_edges": list(x.unbind(0))}, y)
        want.append(eager.last.record.cpu().numpy().copy())
    rows, overflow = meters.rows()
    assert not overflow and rows.shape[0] == 4
    assert rows[1:].tobytes() == np.stack(want).tobytes()
    graph.replay()   # a fifth row: past capacity -> overflow flag, nothing written
    rows2, overflow = meters.rows()
    assert overflow and rows2.tobytes() == rows.tobytes()
    with pytest.raises(RuntimeError, match="capacity"):
        meters.result()


def test_layerwise_engine_with_focal_matches_autograd_of_the_restatement():
    from gnn_cca_amd import MOTMPNet
    from gnn_cca_amd.loss import EdgeLoss
    params, arch, sd, _, _, a = load_bwd("bn_drop_mean", prefix="lw_")
    grads = []
    for use_kernel in (True, False):
        m = MOTMPNet(copy.deepcopy(params), None, arch)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m.train_engine = "layerwise"
        m = m.cuda().train()
        m.set_dropout_seed(1234)
        d = Data()
        d.x, d.edge_index, d.edge_attr = (torch.from_numpy(a[k]).cuda() for k in ("x", "edge_index", "edge_attr"))
        labels = (torch.arange(d.edge_index.shape[1], device="cuda") % 5 == 0).float()
        out = m(d)
        if use_kernel:
            loss = EdgeLoss("Focal")(out, labels)
        else:
            steps = torch.stack([t.view(-1) for t in out["classified_edges"]])
            loss = lo.edge_loss(steps, labels, "Focal")["loss"]
        loss.backward()
        assert np.isfinite(float(loss))
        grads.append({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    assert sorted(grads[0]) == sorted(grads[1]) and grads[0]
    for k in grads[0]:
        scale = max(1e-6, float(grads[1][k].abs().max()))
        assert float((grads[0][k] - grads[1][k].float()).abs().max()) <= 1e-4 * scale + 1e-7, k


def test_edges_cases_no_edge_cpu_and_mismatch():
    from gnn_cca_amd.loss import EdgeLoss
    loss, rec, grad, fn = run_kernel(np.zeros((3, 0), np.float32), np.zeros(0, np.float32), "Focal", None)
    assert np.isnan(float(loss)) and np.isnan(rec[:3]).all() and (rec[3:6] == 0).all() and (rec[6:8] == 0).all()
    assert (rec[8:14] == 0.5).all() and grad.shape == (3, 0)
    x = torch.zeros(2, 10, 1, device="cuda")
    with pytest.raises(RuntimeError, match="MI355X only"):
        EdgeLoss("BCE")({"classified_edges": list(x.cpu().unbind(0))}, torch.zeros(10))
    with pytest.raises(ValueError):
        EdgeLoss("BCE")({"classified_edges": list(x.unbind(0))}, torch.zeros(11, device="cuda"))
    with pytest.raises(ValueError):
        EdgeLoss("BCE")({"classified_edges": list(x.unbind(0))}, torch.zeros(10, device="cuda", dtype=torch.float64))
    # steps that are not one buffer are stacked: same numbers
    parts = [torch.randn(10, 1, device="cuda") for _ in range(2)]
    f1, f2 = EdgeLoss("BCE"), EdgeLoss("BCE")
    lab = (torch.arange(10, device="cuda") % 2).float()
    f1({"classified_edges": parts}, lab)
    f2({"classified_edges": list(torch.stack(parts).unbind(0))}, lab)
    assert f1.last.record.cpu().numpy().tobytes() == f2.last.record.cpu().numpy().tobytes()
