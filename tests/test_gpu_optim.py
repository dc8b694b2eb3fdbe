"""gnn_cca_amd.optim on the MI355X: the FusedSGD / FusedAdam launch (csrc/optim.hip) on bare tensors -- SGD bit for bit against the fp32
restatement, SGD and Adam against torch.optim's own GPU result measured from the fp64 restatement (tests/helpers/optim_oracle.py) --
and on the model: eager, under ONE captured graph while the learning rate follows the reference's schedule, Adam's device step count
under replay, the optimizer switch, checkpoints exchanged with torch.optim in both directions, frozen parameters, and the warning
GraphedTrainStep gives for an optimizer whose learning rate the capture froze."""
import io
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from test_gpu_training_graph import _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import optim_oracle as oo  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (4,), (6,), (127,), (4096 + 1,), (2048, 128)]
STEPS = 30
ULP = 2.0 ** -23
LOSS_TOL = dict(rtol=2e-5, atol=1e-6)      # tests/test_gpu_training_graph.py: graph against eager
STATE_TOL = dict(rtol=1e-4, atol=1e-6)
SGD_HP = dict(momentum=0.9, weight_decay=1e-4)


def _crit():
    crit = torch.nn.BCEWithLogitsLoss()
    return lambda out, lab: sum(crit(t.view(-1), lab) for t in out["classified_edges"])


# ---- bare tensors, prescribed gradients ---------------------------------------------------------------------------------------------
class _Bare:
    """Seeded parameters of SHAPES on the GPU and a gradient source: 'flat' = views of one buffer at 4-float-aligned offsets (what the
    backward hands over), 'separate' = one allocation per tensor, 'packed' = views of one buffer WITHOUT padding (most of them not
    16-byte aligned: the 4-byte path)."""

    def __init__(self, layout, seed):
        self.rng = np.random.default_rng(seed)
        self.layout = layout
        self.params = [torch.from_numpy(self.rng.standard_normal(s).astype(np.float32)).cuda().requires_grad_(True) for s in SHAPES]
        sizes = [p.numel() for p in self.params]
        pad = (lambda n: (n + 3) // 4 * 4) if layout == "flat" else (lambda n: n)
        self.offs = np.concatenate([[0], np.cumsum([pad(n) for n in sizes])]).tolist()
        self.flat = torch.zeros(self.offs[-1], dtype=torch.float32, device="cuda") if layout != "separate" else None

    def set_grads(self):
        """New seeded gradients -> their numpy copies."""
        out = []
        for i, p in enumerate(self.params):
            g = self.rng.standard_normal(tuple(p.shape)).astype(np.float32)
            if self.flat is None:
                p.grad = torch.from_numpy(g).cuda()
            else:
                view = self.flat[self.offs[i]:self.offs[i] + p.numel()].view(p.shape)
                view.copy_(torch.from_numpy(g))
                p.grad = view
            out.append(g)
        return out


def _lrs(scale, seed=11):
    return (scale * (0.5 + np.random.default_rng(seed).random(STEPS))).tolist()


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("layout", ["flat", "separate", "packed"])
@pytest.mark.parametrize("variant", list(oo.SGD_VARIANTS))
def test_sgd_is_the_fp32_restatement_bit_for_bit_and_no_worse_than_torch(variant, layout):
    """After EVERY step: parameters and momentum buffers equal tests/helpers/optim_oracle.sgd_step32 bitwise; and, from the same fp32
    state, e_fused <= 2 e_torch + 2^-23 max|p| with both errors measured from the fp64 restatement."""
    from gnn_cca_amd.optim import FusedSGD
    hp = oo.SGD_VARIANTS[variant]
    lrs = oo.SHIPPED_LRS[::5] if variant == "momentum_wd" else _lrs(0.05)   # the shipped schedule drives one case
    bare = _Bare(layout, seed=5)
    opt = FusedSGD(bare.params, lr=lrs[0], **hp)
    twins = [p.detach().clone().requires_grad_(True) for p in bare.params]
    ref = torch.optim.SGD(twins, lr=lrs[0], **hp)
    p32 = [_np(p) for p in bare.params]
    b32 = [None] * len(p32)
    worst_f = worst_t = 0.0
    for k in range(STEPS):
        grads = bare.set_grads()
        # torch from the same fp32 state
        for tw, p, g, b in zip(twins, p32, grads, b32):
            tw.data.copy_(torch.from_numpy(p))
            tw.grad = torch.from_numpy(g).cuda()
            if b is not None:
                ref.state[tw]["momentum_buffer"] = torch.from_numpy(b).cuda()
        ref.param_groups[0]["lr"] = opt.param_groups[0]["lr"] = lrs[k]
        ref.step()
        opt.step()
        e_f = e_t = pmax = 0.0
        for i, (p, g, b) in enumerate(zip(p32, grads, b32)):
            want_p, want_b = oo.sgd_step32(p, g, b, lrs[k], **hp)
            p64, b64 = oo.sgd_step64(p, g, b, lrs[k], **hp)
            got_p = _np(bare.params[i])
            assert got_p.tobytes() == want_p.tobytes(), (variant, layout, k, SHAPES[i], float(np.abs(got_p - want_p).max()))
            e_f = max(e_f, float(np.abs(got_p - p64).max()))
            e_t = max(e_t, float(np.abs(_np(twins[i]) - p64).max()))
            pmax = max(pmax, float(np.abs(p64).max()))
            if hp["momentum"]:
                got_b = _np(opt.state[bare.params[i]]["momentum_buffer"])
                assert got_b.tobytes() == want_b.tobytes(), (variant, layout, k, SHAPES[i], "momentum_buffer")
                e_f = max(e_f, float(np.abs(got_b - b64).max()))
                e_t = max(e_t, float(np.abs(_np(ref.state[twins[i]]["momentum_buffer"]) - b64).max()))
            else:
                assert bare.params[i] not in opt.state or not opt.state[bare.params[i]]
            p32[i], b32[i] = want_p, want_b
        assert e_f <= 2 * e_t + ULP * pmax, (variant, layout, k, e_f, e_t, pmax)
        worst_f, worst_t = max(worst_f, e_f), max(worst_t, e_t)
    print(f"sgd {variant} {layout}: e_fused {worst_f:.3e}  e_torch {worst_t:.3e}")


@pytest.mark.parametrize("layout", ["flat", "separate", "packed"])
@pytest.mark.parametrize("variant", list(oo.ADAM_VARIANTS))
def test_adam_is_no_worse_than_torch_and_counts_its_steps(variant, layout):
    from gnn_cca_amd.optim import FusedAdam
    hp = oo.ADAM_VARIANTS[variant]
    lrs = _lrs(0.005)
    bare = _Bare(layout, seed=6)
    opt = FusedAdam(bare.params, lr=lrs[0], **hp)
    twins = [p.detach().clone().requires_grad_(True) for p in bare.params]
    ref = torch.optim.Adam(twins, lr=lrs[0], **hp)
    keys = ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if hp["amsgrad"] else [])
    worst_f = worst_t = 0.0
    for k in range(STEPS):
        grads = bare.set_grads()
        p32 = [_np(p) for p in bare.params]
        if k == 0:
            s32 = [{key: np.zeros(s, np.float32) for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")} for s in SHAPES]
        else:
            s32 = [{key: _np(opt.state[p][key]) for key in keys} for p in bare.params]
        for tw, p, g, s in zip(twins, p32, grads, s32):
            tw.data.copy_(torch.from_numpy(p))
            tw.grad = torch.from_numpy(g).cuda()
            if k > 0:
                ref.state[tw] = {"step": torch.tensor(float(k)), **{key: torch.from_numpy(s[key]).cuda() for key in keys}}
        ref.param_groups[0]["lr"] = opt.param_groups[0]["lr"] = lrs[k]
        ref.step()
        opt.step()
        e_f = e_t = pmax = 0.0
        for i, (p, g, s) in enumerate(zip(p32, grads, s32)):
            p64, m64, v64, vm64 = oo.adam_step64(p, g, s["exp_avg"], s["exp_avg_sq"], s.get("max_exp_avg_sq"), k + 1, lrs[k], **hp)
            want = dict(exp_avg=m64, exp_avg_sq=v64, max_exp_avg_sq=vm64)
            e_f = max(e_f, float(np.abs(_np(bare.params[i]) - p64).max()))
            e_t = max(e_t, float(np.abs(_np(twins[i]) - p64).max()))
            pmax = max(pmax, float(np.abs(p64).max()))
            for key in keys:
                e_f = max(e_f, float(np.abs(_np(opt.state[bare.params[i]][key]) - want[key]).max()))
                e_t = max(e_t, float(np.abs(_np(ref.state[twins[i]][key]) - want[key]).max()))
            assert float(ref.state[twins[i]]["step"]) == k + 1
        assert e_f <= 2 * e_t + ULP * pmax, (variant, layout, k, e_f, e_t, pmax)
        worst_f, worst_t = max(worst_f, e_f), max(worst_t, e_t)
    print(f"adam {variant} {layout}: e_fused {worst_f:.3e}  e_torch {worst_t:.3e}")
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(SHAPES)))
    for i in sd["state"]:
        assert float(sd["state"][i]["step"]) == STEPS and set(sd["state"][i]) == {"step", *keys}
    assert opt.step_counts() == [[STEPS] * len(SHAPES)]


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _batches(d, n, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.random(tuple(d.edge_attr.shape)).astype(np.float32)).cuda() for _ in range(n)]


def _eager_iter(m, opt, loss_fn, d, labels):
    opt.zero_grad()
    loss = loss_fn(m(d), labels)
    loss.backward()
    opt.step()
    return float(loss.detach())


def _assert_same_state(m1, m2, what, **tol):
    tol = tol or STATE_TOL
    for (k, p1), (_, p2) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.allclose(p1.float(), p2.float(), **tol), (what, k, float((p1.float() - p2.float()).abs().max()))


def test_model_trains_eagerly_like_torch_sgd():
    """Seven eager iterations, a new batch each: FusedSGD's model equals torch.optim.SGD's.  (Fails if the optimizer does not bump the
    parameters' version counters: the next forward would use the packed weights of the previous iteration.)"""
    from gnn_cca_amd.optim import FusedSGD
    loss_fn = _crit()
    m1, d, labels = _setup()
    m2, _, _ = _setup()
    o1 = torch.optim.SGD(m1.parameters(), lr=0.05, **SGD_HP)
    o2 = FusedSGD(m2.parameters(), lr=0.05, **SGD_HP)
    l1, l2 = [], []
    for ea in _batches(d, 7):
        d.edge_attr = ea
        l1.append(_eager_iter(m1, o1, loss_fn, d, labels))
        l2.append(_eager_iter(m2, o2, loss_fn, d, labels))
    assert np.allclose(l1, l2, **LOSS_TOL), (l1, l2)
    assert l1[-1] < l1[0]
    _assert_same_state(m1, m2, "eager")
    assert o2.step(lambda: 1.25) == 1.25     # a closure is called and its value returned (train.py:494)


def _scheduled_run(make_opt, graphed, constant=False, iters=12):
    """The reference's schedule in small: the warm-up list scaled by 5 set before iterations 2, 4, 6, 8; from iteration 8 a
    StepLR(step_size=2, gamma=0.1) stepped every iteration.  -> (model, losses, the step object or None, the learning rates used)"""
    from gnn_cca_amd.training import GraphedTrainStep
    loss_fn = _crit()
    m, d, labels = _setup()
    warm = [5 * v for v in oo.WARMUP_LRS]
    opt = make_opt(m.parameters(), warm[0])
    step = GraphedTrainStep(m, opt, loss_fn, warmup=2) if graphed else None
    sched, losses, used = None, [], []
    for it, ea in enumerate(_batches(d, iters)):
        d.edge_attr = ea
        if not constant:
            if it in (2, 4, 6, 8):
                opt.param_groups[0]["lr"] = warm[it // 2]
            if it == 8:
                sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.1)
        used.append(opt.param_groups[0]["lr"])
        losses.append(float(step(d, labels)) if graphed else _eager_iter(m, opt, loss_fn, d, labels))
        if sched is not None:
            sched.step()
    return m, losses, step, used


def test_one_graph_follows_the_learning_rate_schedule():
    from gnn_cca_amd.optim import FusedSGD
    torch_sgd = lambda ps, lr: torch.optim.SGD(ps, lr=lr, **SGD_HP)  # noqa: E731
    fused_sgd = lambda ps, lr: FusedSGD(ps, lr=lr, **SGD_HP)  # noqa: E731
    ma, la, _, used_a = _scheduled_run(torch_sgd, graphed=False)
    mc, _, _, used_c = _scheduled_run(torch_sgd, graphed=False, constant=True)
    assert len(set(used_a)) >= 6 and len(set(used_c)) == 1 and used_c[0] == used_a[0]
    # sensitivity: training at the constant first rate (what a frozen capture does) must be far outside the tolerance, or this test is blind
    seen = 0.0
    for (k, pa), (_, pc) in zip(ma.state_dict().items(), mc.state_dict().items()):
        pa, pc = pa.float(), pc.float()
        seen = max(seen, float(((pa - pc).abs() / (STATE_TOL["atol"] + STATE_TOL["rtol"] * pc.abs())).max()))
    print(f"schedule sensitivity: constant-rate run is {seen:.1f} x the tolerance away")
    assert seen > 100, f"the schedule moves the weights by only {seen:.1f} x the tolerance: this test could not see a frozen learning rate"
    mb, lb, step, used_b = _scheduled_run(fused_sgd, graphed=True)
    assert used_b == used_a
    assert len(step._graphs) == 1
    assert np.allclose(la, lb, **LOSS_TOL), (la, lb)
    _assert_same_state(ma, mb, "schedule under one graph")


def test_adam_under_one_graph_advances_its_step_count():
    from gnn_cca_amd.optim import FusedAdam
    from gnn_cca_amd.training import GraphedTrainStep
    loss_fn = _crit()
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    runs = {}
    for name in ("single", "foreach", "fused"):
        m, d, labels = _setup()
        if name == "fused":
            opt = FusedAdam(m.parameters(), **hp)
            step = GraphedTrainStep(m, opt, loss_fn, warmup=2)
        else:
            opt = torch.optim.Adam(m.parameters(), foreach=(name == "foreach"), **hp)
        losses = []
        for ea in _batches(d, 8):
            d.edge_attr = ea
            losses.append(float(step(d, labels)) if name == "fused" else _eager_iter(m, opt, loss_fn, d, labels))
        runs[name] = (m, losses, opt)
    assert len(step._graphs) == 1
    sd = runs["fused"][2].state_dict()["state"]
    assert len(sd) == len(list(runs["fused"][0].parameters())) and all(float(s["step"]) == 8 for s in sd.values())
    # two legitimate torch evaluations of the same training: their deviation is the scale of "equal" here
    dev_loss = float(np.abs(np.asarray(runs["single"][1]) - np.asarray(runs["foreach"][1])).max())
    s1, s2, sf = (runs[k][0].state_dict() for k in ("single", "foreach", "fused"))
    dev = max(float((s1[k].float() - s2[k].float()).abs().max()) for k in s1)
    print(f"adam: torch foreach=False against foreach=True: losses {dev_loss:.3e}, state {dev:.3e}")
    lf, l1 = np.asarray(runs["fused"][1]), np.asarray(runs["single"][1])
    assert np.all(np.abs(lf - l1) <= np.maximum(4 * dev_loss, LOSS_TOL["atol"] + LOSS_TOL["rtol"] * np.abs(l1))), (lf, l1, dev_loss)
    for k in s1:
        a, b = sf[k].float(), s1[k].float()
        bound = torch.clamp(STATE_TOL["atol"] + STATE_TOL["rtol"] * b.abs(), min=4 * dev)
        assert bool(((a - b).abs() <= bound).all()), (k, float((a - b).abs().max()), dev)
    print(f"adam: fused against foreach=False: state {max(float((sf[k].float() - s1[k].float()).abs().max()) for k in s1):.3e}")


def test_optimizer_switch_drops_the_graphs():
    """main_training.py:353-363: Adam for the first iterations, then a fresh SGD."""
    from gnn_cca_amd.optim import FusedAdam, FusedSGD
    from gnn_cca_amd.training import GraphedTrainStep
    loss_fn = _crit()
    m1, d, labels = _setup()
    m2, _, _ = _setup()
    o1 = torch.optim.Adam(m1.parameters(), lr=1e-3)
    step = GraphedTrainStep(m2, FusedAdam(m2.parameters(), lr=1e-3), loss_fn, warmup=2)
    l1, l2 = [], []
    for it, ea in enumerate(_batches(d, 7)):
        d.edge_attr = ea
        if it == 3:
            assert len(step._graphs) == 1
            old = [e[0] for e in step._graphs.values()]
            o1 = torch.optim.SGD(m1.parameters(), lr=0.05, **SGD_HP)
            step.set_optimizer(FusedSGD(m2.parameters(), lr=0.05, **SGD_HP))
            assert len(step._graphs) == 0 and len(step._seen) == 0
        l1.append(_eager_iter(m1, o1, loss_fn, d, labels))
        l2.append(float(step(d, labels)))
    assert len(step._graphs) == 1 and all(e[0] is not old[0] for e in step._graphs.values())
    assert isinstance(step.optimizer, FusedSGD)
    assert np.allclose(l1, l2, **LOSS_TOL), (l1, l2)
    _assert_same_state(m1, m2, "optimizer switch")


@pytest.mark.parametrize("kind,direction", [("sgd", "fused_to_torch"), ("sgd", "torch_to_fused"), ("adam", "fused_to_torch"),
                                            ("adam", "torch_to_fused")])
def test_checkpoints_are_interchangeable_with_torch(kind, direction):
    from gnn_cca_amd.optim import FusedAdam, FusedSGD
    loss_fn = _crit()
    if kind == "sgd":
        make = {"fused": lambda ps: FusedSGD(ps, lr=0.05, **SGD_HP), "torch": lambda ps: torch.optim.SGD(ps, lr=0.05, **SGD_HP)}
    else:
        make = {"fused": lambda ps: FusedAdam(ps, lr=1e-3, amsgrad=True), "torch": lambda ps: torch.optim.Adam(ps, lr=1e-3, amsgrad=True)}
    first, second = direction.split("_to_")
    m1, d, labels = _setup()
    m2, _, _ = _setup()
    o1 = make[first](m1.parameters())
    batches = _batches(d, 6)
    for ea in batches[:3]:
        d.edge_attr = ea
        _eager_iter(m1, o1, loss_fn, d, labels)
    m2.load_state_dict(m1.state_dict())
    o2 = make[second](m2.parameters())
    # through a file image, as save_checkpoint / torch.load do (main_training.py:422-433); handing the live dictionary over would
    # make the two optimizers share their state tensors -- with two torch optimizers as well
    image = io.BytesIO()
    torch.save({"optimizer_state_dict": o1.state_dict()}, image)
    image.seek(0)
    o2.load_state_dict(torch.load(image)["optimizer_state_dict"])
    l1, l2 = [], []
    for ea in batches[3:]:
        d.edge_attr = ea
        l1.append(_eager_iter(m1, o1, loss_fn, d, labels))
        l2.append(_eager_iter(m2, o2, loss_fn, d, labels))
    assert np.allclose(l1, l2, **LOSS_TOL), (l1, l2)
    _assert_same_state(m1, m2, f"{kind} {direction}")
    sd1, sd2 = o1.state_dict(), o2.state_dict()
    assert [set(g) for g in sd1["param_groups"]] == [set(g) for g in sd2["param_groups"]]
    assert sd1["param_groups"][0]["params"] == sd2["param_groups"][0]["params"]
    assert sorted(sd1["state"]) == sorted(sd2["state"]) and len(sd1["state"]) > 0
    for i in sd1["state"]:
        assert set(sd1["state"][i]) == set(sd2["state"][i]), i
        for key, v in sd1["state"][i].items():
            assert tuple(v.shape) == tuple(sd2["state"][i][key].shape), (i, key)
            if key == "step":
                assert float(v) == float(sd2["state"][i][key]) == 6
    want = {"momentum_buffer"} if kind == "sgd" else {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    assert set(sd1["state"][0]) == want


@pytest.mark.parametrize("graphed", [False, True])
def test_frozen_parameters_are_skipped(graphed):
    from gnn_cca_amd.optim import FusedSGD
    from gnn_cca_amd.training import GraphedTrainStep
    loss_fn = _crit()
    m, d, labels = _setup()
    for p in m.classifier.parameters():
        p.requires_grad_(False)
    frozen = [(p, p.detach().clone()) for p in m.classifier.parameters()]
    moving = [(p, p.detach().clone()) for p in m.parameters() if p.requires_grad]
    assert frozen and moving
    opt = FusedSGD(m.parameters(), lr=0.05, **SGD_HP)     # (weight decay alone would move a parameter that is not skipped)
    step = GraphedTrainStep(m, opt, loss_fn, warmup=2)
    for ea in _batches(d, 5):
        d.edge_attr = ea
        if graphed:
            step(d, labels)
        else:
            _eager_iter(m, opt, loss_fn, d, labels)
    torch.cuda.synchronize()
    assert not graphed or len(step._graphs) == 1
    for p, was in frozen:
        assert torch.equal(p.detach(), was) and (p not in opt.state or not opt.state[p])
    assert all(not torch.equal(p.detach(), was) for p, was in moving)
    assert all("momentum_buffer" in opt.state[p] for p, _ in moving)
    assert len(opt.state_dict()["state"]) == len(moving)


def test_graphed_step_warns_when_the_capture_froze_the_learning_rate():
    from gnn_cca_amd.training import GraphedTrainStep
    loss_fn = _crit()
    m, d, labels = _setup()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    step = GraphedTrainStep(m, opt, loss_fn, warmup=2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(4):
            step(d, labels)
    assert len(step._graphs) == 1
    assert not [w for w in caught if "FusedSGD" in str(w.message)]     # nothing while the learning rate is the captured one
    opt.param_groups[0]["lr"] = 0.005
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        a = float(step(d, labels))
        b = float(step(d, labels))
    mine = [w for w in caught if issubclass(w.category, UserWarning) and "FusedSGD" in str(w.message)]
    assert len(mine) == 1 and "learning rate" in str(mine[0].message), [str(w.message) for w in caught]
    assert np.isfinite(a) and np.isfinite(b) and len(step._graphs) == 1
