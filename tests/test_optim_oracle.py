"""The float64 restatements of SGD and Adam (tests/helpers/optim_oracle.py) against torch.optim on CPU float64 tensors; the learning rates
of the shipped training config as a list; the C ABI of gnncca_optim_* refuses bad arguments before any launch (no device needed);
FusedSGD / FusedAdam refuse what they do not implement."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import optim_oracle as oo  # noqa: E402

STEPS, N = 30, 1000


def _lrs(seed):
    return (0.05 * (0.5 + np.random.default_rng(seed).random(STEPS))).tolist()


def test_shipped_learning_rates_are_the_configs():
    assert np.array_equal(np.asarray(oo.WARMUP_LRS), np.linspace(0, 0.01, 6, endpoint=False)[1:])
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=0.01, momentum=0.9, weight_decay=1e-4)    # the optimizer main_training.py:353-363 builds after the warm-up
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=40, gamma=0.1)
    after = []
    for _ in range(145):
        after.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert len(oo.SHIPPED_LRS) == 150
    assert np.allclose(oo.SHIPPED_LRS[5:], after, rtol=1e-12, atol=0)
    assert sorted(set(oo.SHIPPED_LRS[5:]), reverse=True) == [0.01, 0.001, 0.0001, 0.00001]


@pytest.mark.parametrize("variant", list(oo.SGD_VARIANTS) + ["momentum_wd_shipped_lrs"])
def test_sgd_restatement_equals_torch_in_float64(variant):
    shipped = variant.endswith("_shipped_lrs")
    hp = oo.SGD_VARIANTS[variant.replace("_shipped_lrs", "")]
    lrs = oo.SHIPPED_LRS[::5] if shipped else _lrs(1)   # every fifth epoch of the shipped schedule: warm-up, 0.01, and all three decays
    assert len(lrs) == STEPS and (not shipped or {0.01, 0.001, 0.0001, 0.00001} <= set(lrs))
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(N)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=lrs[0], **hp)
    p, buf, worst = p0.copy(), None, 0.0
    for k in range(STEPS):
        g = rng.standard_normal(N)
        opt.param_groups[0]["lr"] = lrs[k]
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, buf = oo.sgd_step64(p, g, buf, lrs[k], **hp)
        worst = max(worst, float(np.abs(tp.detach().numpy() - p).max()))
        if hp["momentum"]:
            worst = max(worst, float(np.abs(opt.state[tp]["momentum_buffer"].numpy() - buf).max()))
    print(f"sgd {variant}: max |restatement - torch| = {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("variant", list(oo.ADAM_VARIANTS))
def test_adam_restatement_equals_torch_in_float64(variant):
    hp = oo.ADAM_VARIANTS[variant]
    lrs = (np.asarray(_lrs(2)) * 0.1).tolist()
    rng = np.random.default_rng(8)
    p0 = rng.standard_normal(N)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=lrs[0], **hp)
    p, m, v, vm, worst = p0.copy(), np.zeros(N), np.zeros(N), np.zeros(N), 0.0
    for k in range(STEPS):
        g = rng.standard_normal(N)
        opt.param_groups[0]["lr"] = lrs[k]
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v, vm = oo.adam_step64(p, g, m, v, vm, k + 1, lrs[k], **hp)
        st = opt.state[tp]
        worst = max(worst, float(np.abs(tp.detach().numpy() - p).max()), float(np.abs(st["exp_avg"].numpy() - m).max()),
                    float(np.abs(st["exp_avg_sq"].numpy() - v).max()))
        if hp["amsgrad"]:
            worst = max(worst, float(np.abs(st["max_exp_avg_sq"].numpy() - vm).max()))
        assert float(st["step"]) == k + 1
    print(f"adam {variant}: max |restatement - torch| = {worst:.3e}")
    assert worst <= 1e-12


def test_float32_sgd_restatement_tracks_the_float64_one():
    """The fp32 operation-order restatement is the same rule: after one step from the same fp32 state it is within a few roundings."""
    rng = np.random.default_rng(3)
    for name, hp in oo.SGD_VARIANTS.items():
        p = rng.standard_normal(N).astype(np.float32)
        buf = None
        for k in range(5):
            g = rng.standard_normal(N).astype(np.float32)
            p64, b64 = oo.sgd_step64(p, g, buf, 0.05, **hp)
            p, buf = oo.sgd_step32(p, g, buf, 0.05, **hp)
            assert p.dtype == np.float32
            assert np.abs(p - p64).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(p64).max()), (name, k)
            if buf is not None:
                assert np.abs(buf - b64).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(b64).max()), (name, k)


def test_abi_refuses_bad_arguments_before_any_launch():
    import ctypes as C

    from gnn_cca_amd import _native as nat
    lib = nat.lib()
    assert lib.gnncca_optim_block_bytes(-1) == 0
    assert lib.gnncca_optim_block_bytes(0) >= nat.OPTIM_BLOCK_STEPS_OFFSET
    assert lib.gnncca_optim_block_bytes(40) >= nat.OPTIM_BLOCK_STEPS_OFFSET + 4 * 40
    fake = 0x10000
    bad = nat.ERR_INVALID_ARG

    def hyper(block=fake, rule=nat.OPTIM_SGD, lr=0.01, wd=0.0, a=0.9, b=0.0, c=0.0, flag=0):
        return lib.gnncca_optim_set_hyper(block, rule, lr, wd, a, b, c, flag, None)

    assert hyper(block=None) == bad
    assert hyper(rule=2) == bad and hyper(rule=-1) == bad                                   # an unknown rule
    assert hyper(lr=-0.1) == bad and hyper(lr=float("nan")) == bad and hyper(wd=-1e-4) == bad
    assert hyper(a=-0.9) == bad and hyper(a=float("inf")) == bad                            # SGD momentum
    assert hyper(a=0.0, flag=1) == bad and hyper(a=0.9, b=0.5, flag=1) == bad               # Nesterov needs momentum, no dampening
    adam = dict(rule=nat.OPTIM_ADAM, a=0.9, b=0.999, c=1e-8)
    assert hyper(**dict(adam, a=1.0)) == bad and hyper(**dict(adam, a=-0.1)) == bad         # beta1 in [0, 1)
    assert hyper(**dict(adam, b=1.0)) == bad and hyper(**dict(adam, b=float("nan"))) == bad
    assert hyper(**dict(adam, c=-1e-8)) == bad and hyper(**dict(adam, lr=-1.0)) == bad

    def arr(kind, vals):
        return (kind * len(vals))(*vals)

    def sgd(block=fake, n_slots=2, n=2, params=(fake, fake), grads=(fake, fake), bufs=(fake, fake), numel=(8, 3), slots=(0, 1)):
        return lib.gnncca_optim_sgd_step(block, n_slots, n, arr(C.c_void_p, params) if params is not None else None,
                                         arr(C.c_void_p, grads) if grads is not None else None,
                                         arr(C.c_void_p, bufs) if bufs is not None else None,
                                         arr(C.c_int64, numel) if numel is not None else None,
                                         arr(C.c_int32, slots) if slots is not None else None, None)

    assert sgd(block=None) == bad and sgd(n=-1) == bad and sgd(n_slots=-1) == bad
    assert sgd(params=None) == bad and sgd(grads=None) == bad and sgd(numel=None) == bad and sgd(slots=None) == bad
    assert sgd(params=(fake, None)) == bad and sgd(grads=(None, fake)) == bad
    assert sgd(numel=(8, -1)) == bad
    assert sgd(slots=(0, 2)) == bad and sgd(slots=(-1, 1)) == bad and sgd(slots=(1, 1)) == bad
    assert sgd(n=0, params=None, grads=None, bufs=None, numel=None, slots=None) == nat.OK      # nothing to launch
    assert sgd(numel=(0, 0), params=(None, None), grads=(None, None)) == nat.OK               # empty tensors: nothing to launch

    def adam_step(m=(fake, fake), v=(fake, fake), vm=None, **kw):
        a = dict(block=fake, n_slots=2, n=2, params=(fake, fake), grads=(fake, fake), numel=(8, 3), slots=(0, 1))
        a.update(kw)
        return lib.gnncca_optim_adam_step(a["block"], a["n_slots"], a["n"], arr(C.c_void_p, a["params"]), arr(C.c_void_p, a["grads"]),
                                          arr(C.c_void_p, m) if m is not None else None, arr(C.c_void_p, v) if v is not None else None,
                                          arr(C.c_void_p, vm) if vm is not None else None, arr(C.c_int64, a["numel"]),
                                          arr(C.c_int32, a["slots"]), None)

    assert adam_step(block=None) == bad and adam_step(m=None) == bad and adam_step(v=None) == bad
    assert adam_step(m=(fake, None)) == bad and adam_step(v=(None, fake)) == bad
    assert adam_step(numel=(-2, 3)) == bad and adam_step(slots=(0, 5)) == bad
    assert adam_step(numel=(0, 0)) == nat.OK


def test_fused_optimizers_refuse_what_they_do_not_implement():
    from gnn_cca_amd.optim import FusedAdam, FusedSGD
    from gnn_cca_amd.training import FusedAdam as A2, FusedSGD as S2
    assert A2 is FusedAdam and S2 is FusedSGD            # re-exported next to GraphedTrainStep
    assert issubclass(FusedSGD, torch.optim.Optimizer) and issubclass(FusedAdam, torch.optim.Optimizer)
    cpu = [torch.zeros(4, requires_grad=True)]
    for cls in (FusedSGD, FusedAdam):
        with pytest.raises(ValueError, match="MI355X only"):
            cls(cpu, lr=0.1)
        with pytest.raises(ValueError, match="maximize"):
            cls(cpu, lr=0.1, maximize=True)
        with pytest.raises(ValueError, match="differentiable"):
            cls(cpu, lr=0.1, differentiable=True)
        with pytest.raises(ValueError, match="[Ii]nvalid learning rate"):
            cls(cpu, lr=-1.0)
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        FusedAdam(cpu, decoupled_weight_decay=True)
    with pytest.raises(ValueError, match="beta"):
        FusedAdam(cpu, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="momentum"):
        FusedSGD(cpu, lr=0.1, momentum=-0.5)
    with pytest.raises(ValueError, match="Nesterov"):
        FusedSGD(cpu, lr=0.1, nesterov=True)
    # the parameter-group keys are torch's: part of what makes the state_dict()s interchangeable
    import inspect
    p = torch.zeros(1, requires_grad=True)
    for cls, ref in ((FusedSGD, torch.optim.SGD([p], lr=0.1)), (FusedAdam, torch.optim.Adam([p], lr=0.1))):
        assert {k for k in inspect.signature(cls.__init__).parameters if k not in ("self", "params")} == set(ref.defaults)
