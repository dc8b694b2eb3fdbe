"""Restatements of the two update rules gnn_cca_amd.optim implements, written from the rules as the optimizers' documentation states
them (not from torch's source):

  * `sgd_step64` / `adam_step64`: numpy float64 -- the yardstick every fp32 evaluation (the HIP kernel's, torch's) is measured against;
  * `sgd_step32`: numpy float32, ONE numpy operation per device operation, in the order the header of csrc/optim.hip documents -- the
    kernel's SGD result is this bit for bit (multiplications and additions only, each correctly rounded, no contraction).

State is passed and returned explicitly; `buf is None` / `t == 1` is a tensor's first step.
"""
import numpy as np

SGD_VARIANTS = {
    "plain": dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
    "momentum": dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False),
    "momentum_wd": dict(momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False),
    "nesterov": dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=True),
    "dampening": dict(momentum=0.9, dampening=0.5, weight_decay=0.0, nesterov=False),
}
ADAM_VARIANTS = {
    "plain": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False),
    "wd": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False),
    "amsgrad": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=True),
}

# The learning rates of the shipped config_training.yaml, one per epoch: five warm-up epochs np.linspace(0, 0.01, 6, endpoint=False)[1:]
# (main_training.py:220-256), then 0.01 under StepLR(step_size=40, gamma=0.1) for the 145 epochs that remain (main_training.py:349-370).
WARMUP_LRS = [0.0016666666666666668, 0.0033333333333333335, 0.005, 0.006666666666666667, 0.008333333333333333]
SHIPPED_LRS = WARMUP_LRS + [0.01] * 40 + [0.001] * 40 + [0.0001] * 40 + [0.00001] * 25


def sgd_step64(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """One SGD step in float64 -> (p, buf).  buf: the momentum buffer, None before the tensor's first step (it then becomes the
    gradient itself, weight decay included -- NOT momentum * 0 + (1 - dampening) * g)."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g.copy() if buf is None else momentum * np.asarray(buf, np.float64) + (1.0 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


def adam_step64(p, g, m, v, vmax, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
    """One Adam step in float64 -> (p, m, v, vmax).  t: the number of this step, from 1; m, v, vmax: zeros before the first."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    b1, b2 = betas
    if weight_decay != 0:
        g = g + weight_decay * p
    m = b1 * np.asarray(m, np.float64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, np.float64) + (1.0 - b2) * g * g
    u = v
    if amsgrad:
        vmax = np.maximum(np.asarray(vmax, np.float64), v)
        u = vmax
    denom = np.sqrt(u) / np.sqrt(1.0 - b2 ** t) + eps
    return p - (lr / (1.0 - b1 ** t)) * m / denom, m, v, vmax


def sgd_step32(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """The kernel's SGD step, operation for operation, in numpy float32 -> (p, buf) (csrc/optim.hip's header names t1 .. t5)."""
    f = np.float32
    p, g = np.asarray(p, f), np.asarray(g, f)
    lr32, wd, mom = f(lr), f(weight_decay), f(momentum)   # the fp64 hyperparameters, rounded once
    omd = f(1.0 - float(dampening))                        # the subtraction in fp64, then rounded
    assert p.dtype == f and g.dtype == f
    if wd != 0:
        t1 = wd * p
        g = g + t1
    if mom != 0:
        if buf is None:
            buf = g.copy()
        else:
            t2 = mom * np.asarray(buf, f)
            t3 = omd * g
            buf = t2 + t3
        if nesterov:
            t4 = mom * buf
            g = g + t4
        else:
            g = buf
    t5 = lr32 * g
    p = p - t5
    assert p.dtype == f and (buf is None or buf.dtype == f)
    return p, buf
