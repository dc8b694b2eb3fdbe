"""The torch restatement of the training loss (tests/helpers/loss_oracle.py) against the reference's own compute_loss_acc (goldens of
tests/golden/make_golden_loss.py); the C ABI of gnncca_edge_loss_* refuses bad arguments before any launch (no device needed); the host
reduction of TrainMeters.result() equals the reference's AverageMeter bit for bit; EdgeLoss refuses CPU tensors and bad settings."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import loss_oracle as lo  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "post2_train_loss.npz")


def bits(v):
    return struct.pack("<d", float(v))


def test_restatement_reproduces_the_reference_goldens():
    z = np.load(GOLDEN)
    n = n_grad = 0
    for key, c in lo.golden_cases(z):
        x = torch.from_numpy(c["x"].copy()).requires_grad_(True)
        r = lo.edge_loss(x, torch.from_numpy(c["y"]), c["criterion"], c["pos_weight"], mode=c["mode"])
        st = c["stats"]   # loss, precision1, precision0, precision, loss_class1, loss_class0
        assert lo.close([float(r["loss"].detach()), r["loss_class1"], r["loss_class0"]], [st[0], st[4], st[5]]), (key, r, st)
        assert [bits(r["precision1"]), bits(r["precision0"]), bits(r["precision"])] == [bits(v) for v in st[1:4]], (key, r, st)
        assert lo.close(r["mean_prob"], c["mean_prob"]), key
        if c["grad"] is not None:
            r["loss"].backward()
            g, want = x.grad.numpy(), c["grad"]
            scale = float(np.abs(want).max()) if want.size else 0.0
            assert np.array_equal(np.isnan(g), np.isnan(want)), key
            assert want.size == 0 or np.nanmax(np.abs(g - want)) <= 1e-6 * scale, (key, np.nanmax(np.abs(g - want)), scale)
            n_grad += 1
        n += 1
    assert n == 80 and n_grad >= 30
    # the corner cases are in the fixture: empty classes, no edge, a logit that sigmoid rounds to 0.5
    assert np.isnan(z["stats__allpos_s3__BCE__train"][5]) and np.isnan(z["stats__allneg_s3__Focal__train"][4])
    assert np.isnan(z["stats__e0_s3__BCE__validate"][0]) and np.all(z["mp__e0_s3__BCE__train"] == 0.5)
    assert z["x__terrace_s3"][0, 1] == np.float32(-1e-9)


def test_abi_refuses_bad_arguments_before_any_launch():
    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    assert lib.gnncca_edge_loss_workspace_bytes(0, 10) == 0 and lib.gnncca_edge_loss_workspace_bytes(3, -1) == 0
    assert lib.gnncca_edge_loss_workspace_bytes(3, 0) >= 256
    fake = 0x10000
    ws_ok = lib.gnncca_edge_loss_workspace_bytes(3, 1000)
    args = dict(logits=fake, labels=fake, s=3, e=1000, crit=0, val=0, pw=1.0, gamma=5.0, alpha=0.9, loss=fake, rec=fake, hist=None, cap=0,
                cur=None, ws=fake, wsb=ws_ok)

    def fwd(**kw):
        a = dict(args, **kw)
        return lib.gnncca_edge_loss_forward(a["logits"], a["labels"], a["s"], a["e"], a["crit"], a["val"], a["pw"], a["gamma"], a["alpha"],
                                            a["loss"], a["rec"], a["hist"], a["cap"], a["cur"], a["ws"], a["wsb"], None)

    assert fwd(s=0) == nat.ERR_INVALID_ARG
    assert fwd(e=-1) == nat.ERR_INVALID_ARG
    assert fwd(crit=3) == nat.ERR_INVALID_ARG and fwd(crit=-1) == nat.ERR_INVALID_ARG
    assert fwd(crit=1, pw=0.0) == nat.ERR_INVALID_ARG and fwd(crit=1, pw=-4.5) == nat.ERR_INVALID_ARG
    assert fwd(crit=1, pw=float("nan")) == nat.ERR_INVALID_ARG
    assert fwd(crit=2, gamma=float("nan")) == nat.ERR_INVALID_ARG
    assert fwd(wsb=ws_ok - 1) == nat.ERR_WORKSPACE
    assert fwd(logits=None) == nat.ERR_INVALID_ARG and fwd(labels=None) == nat.ERR_INVALID_ARG
    assert fwd(loss=None) == nat.ERR_INVALID_ARG and fwd(rec=None) == nat.ERR_INVALID_ARG
    assert fwd(hist=fake, cur=None) == nat.ERR_INVALID_ARG and fwd(hist=fake, cur=fake, cap=-1) == nat.ERR_INVALID_ARG
    assert fwd(s=65, wsb=1 << 30) == nat.ERR_UNSUPPORTED

    def bwd(s=3, e=1000, crit=0, pw=1.0, g=fake, rec=fake, grad=fake, logits=fake):
        return lib.gnncca_edge_loss_backward(logits, fake, s, e, crit, 0, pw, g, rec, grad, None)

    assert bwd(s=0) == nat.ERR_INVALID_ARG and bwd(e=-5) == nat.ERR_INVALID_ARG and bwd(crit=7) == nat.ERR_INVALID_ARG
    assert bwd(crit=1, pw=0.0) == nat.ERR_INVALID_ARG and bwd(g=None) == nat.ERR_INVALID_ARG and bwd(rec=None) == nat.ERR_INVALID_ARG
    assert bwd(grad=None) == nat.ERR_INVALID_ARG and bwd(logits=None) == nat.ERR_INVALID_ARG
    assert bwd(e=0, grad=None, logits=None) == nat.OK   # nothing to launch


def test_meters_reduction_equals_average_meter_bit_for_bit():
    from gnn_cca_amd.loss import record_len, reduce_history
    z = np.load(GOLDEN)
    vals = z["epoch_values"]            # [K, 6]: what each of the six meters received, in train.py:472-479's order
    mp = z["epoch_mean_probs"]          # [S, 2, K] fp32
    s, k = mp.shape[0], vals.shape[0]
    rows = np.zeros((k, record_len(s)))
    rows[:, 0], rows[:, 1], rows[:, 2] = vals[:, 0], vals[:, 1], vals[:, 2]   # the fp32 .item()s, exact in fp64
    rows[:, 3], rows[:, 4], rows[:, 5] = vals[:, 3], vals[:, 4], vals[:, 5]
    rows[:, 8:8 + 2 * s] = mp.transpose(2, 0, 1).reshape(k, 2 * s)
    out = reduce_history(rows, s, batch_size=int(z["epoch_batch_size"]))
    assert out["iterations"] == k
    for q, name in enumerate(("loss", "loss_class1", "loss_class0", "precision1", "precision0", "precision")):
        m = out[name]
        got = [m["val"], m["sum"], m["count"], m["avg"]]
        assert [bits(v) for v in got] == [bits(v) for v in z["epoch_meters"][q]], (name, got, z["epoch_meters"][q])
        assert [bits(v) for v in m["values"]] == [bits(v) for v in vals[:, q]], name
    for st in range(s):
        for c in (0, 1):
            assert out["mean_probs_epoch"][str(c)][f"step{st}"].tobytes() == z["epoch_mean_probs_history"][st, c].tobytes(), (st, c)
            assert out["mean_probs"][str(c)][f"step{st}"].tobytes() == mp[st, c].tobytes()


def test_edge_loss_refuses_cpu_tensors_and_bad_settings():
    from gnn_cca_amd.loss import EdgeLoss
    from gnn_cca_amd.training import EdgeLoss as ReExported, TrainMeters  # noqa: F401
    assert ReExported is EdgeLoss
    x = torch.zeros(3, 10, 1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        EdgeLoss("BCE")({"classified_edges": list(x.unbind(0))}, torch.zeros(10))
    with pytest.raises(ValueError):
        EdgeLoss("MSE")
    with pytest.raises(ValueError):
        EdgeLoss("BCE_weighted")
    with pytest.raises(ValueError):
        EdgeLoss("BCE_weighted", pos_weight=0.0)
    with pytest.raises(ValueError):
        EdgeLoss("BCE", mode="test")
    with pytest.raises(ValueError):
        EdgeLoss("Focal")({"classified_edges": []}, torch.zeros(10))
