"""The constant-velocity Kalman filter of gnn_cca_amd.smoothing (TrackSmoother) restated with numpy scalars, for the tests: plain Python
loops over the frames of a batch, every scalar operation one np.float64 operation in the order the rule gives.  The links are an INPUT:
matched_prev / matched_gap as a linker oracle (tests/tracking_time_oracle.py link_timed, or any other) returns them.

The rule.  The two ground-plane axes are independent and share one 2 x 2 covariance (a, b, c) = (var pos, cov pos / vel, var vel).
q: process noise intensity, finite and >= 0; r: measurement variance, finite and > 0; vel_var: initial velocity variance, finite and > 0;
per_detection: the measurement variance of a cluster is re = r / float64(size) when True, else re = r.  For cluster a of frame t with
measurement z = pos(a):
  Birth (matched_gap(a) == -1):  p = z, v = (0, 0), (a, b, c) = (re, 0, vel_var), age = 0, nis = 0.
  Link to cluster m = matched_prev(a) of frame t - 1 - k, k = matched_gap(a):  dt = float64(k + 1) without time stamps, with them
  dt = T[t] - T[t - 1 - k] (frames counted among frames PRESENT, as the linker counts them); from that cluster's filtered state
  (p, v, a, b, c, age), one fp64 operation per operator as written, left to right, no FMA:
    dt2 = dt*dt;  dt3 = dt2*dt
    pp  = p + dt*v                               (per axis)
    a_  = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0
    b_  = (b + dt*c) + (q*dt2)/2.0
    c_  = c + q*dt
    s   = a_ + re
    k1  = a_/s;  k2 = b_/s
    i   = z - pp                                 (per axis)
    p'  = pp + k1*i;  v' = v + k2*i              (per axis)
    a'  = a_ - k1*a_;  b' = b_ - k1*b_;  c' = c_ - k2*b_
    nis = (ix*ix + iy*iy)/s
    age' = age + 1
Non-finite inputs propagate; rows at or beyond a frame's count, and every row of a refused frame (count < 0), are zero with age = -1.
The rule is causal along predecessor links only: the result does not depend on how a sequence is cut into calls; the carried state is
the filtered state of the rows of the last max_gap + 1 frames (and their times, when the calls have time stamps).  No fixture files."""
import numpy as np

MAX_GAP = 8
HEADER_BYTES = 64
F = np.float64


def new_state():
    """No frame seen yet.  `frames`: the last min(M + 1, frames seen) frames, oldest first, each a dict(count, rows (the frame's node
    count: its row capacity in the device state), x float64 [count, 7] = (px, py, vx, vy, a, b, c), age int32 [count], time)."""
    return dict(frames=[])


def check_params(q, r, vel_var):
    for name, v, low_ok in (("process_noise", q, True), ("measurement_noise", r, False), ("vel_var", vel_var, False)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{name} must be a finite number, not {v!r}")
        if v < 0 or (v == 0 and not low_ok):
            raise ValueError(f"{name} must be {'>= 0' if low_ok else '> 0'}, not {v!r}")


def step(x, age, z, dt, q, re):
    """One link: the predecessor's filtered state x = (px, py, vx, vy, a, b, c) and age, the measurement z, the elapsed time dt ->
    (the new state, nis, the new age).  Every line is the rule's, one operation per operator, left to right."""
    px, py, vx, vy, a, b, c = (F(v) for v in x)
    zx, zy, dt, q, re = F(z[0]), F(z[1]), F(dt), F(q), F(re)
    with np.errstate(all="ignore"):
        dt2 = dt * dt
        dt3 = dt2 * dt
        ppx = px + dt * vx
        ppy = py + dt * vy
        a_ = ((a + (F(2.0) * dt) * b) + dt2 * c) + (q * dt3) / F(3.0)
        b_ = (b + dt * c) + (q * dt2) / F(2.0)
        c_ = c + q * dt
        s = a_ + re
        k1 = a_ / s
        k2 = b_ / s
        ix = zx - ppx
        iy = zy - ppy
        npx = ppx + k1 * ix
        npy = ppy + k1 * iy
        nvx = vx + k2 * ix
        nvy = vy + k2 * iy
        na = a_ - k1 * a_
        nb = b_ - k1 * b_
        nc = c_ - k2 * b_
        nis = (ix * ix + iy * iy) / s
    return np.array([npx, npy, nvx, nvy, na, nb, nc], F), nis, int(age) + 1


def smooth(summ, node_ptr, links, q, r, vel_var, per_detection=False, max_gap=0, times=None, state=None):
    """summ: the summaries dict (count [G], size [N], pos [N, 2]); links: dict(matched_prev [N], matched_gap [N]) of the linker oracle for
    the same batch; times: None or one time per frame of the batch (the state's frames then carry theirs).
    -> (dict(pos [N, 2], vel [N, 2], cov [N, 3], nis [N], age [N]), the state to carry)."""
    check_params(q, r, vel_var)
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [0, {MAX_GAP}], not {max_gap!r}")
    node_ptr = np.asarray(node_ptr, np.int64)
    g, n = len(node_ptr) - 1, int(node_ptr[-1])
    state = state if state is not None else new_state()
    hist = state["frames"]
    h = len(hist)
    if times is not None:
        times = [F(v) for v in times]
        if len(times) != g:
            raise ValueError(f"the batch has {g} frames, times has {len(times)} entries")
    if hist and g and (hist[-1]["time"] is None) != (times is None):
        raise ValueError("a state written with time stamps is not continued without them, nor the reverse")
    pos, vel, cov = np.zeros((n, 2), F), np.zeros((n, 2), F), np.zeros((n, 3), F)
    nis, age = np.zeros(n, F), np.full(n, -1, np.int32)
    frames = list(hist)
    for t in range(g):
        v0, rows = int(node_ptr[t]), int(node_ptr[t + 1] - node_ptr[t])
        c = max(int(summ["count"][t]), 0)
        fx, fage = np.zeros((c, 7), F), np.zeros(c, np.int32)
        for a in range(c):
            row = v0 + a
            z = np.asarray(summ["pos"][row], F)
            with np.errstate(all="ignore"):
                re = F(r) / F(int(summ["size"][row])) if per_detection else F(r)
            k = int(links["matched_gap"][row])
            if k < 0:   # birth
                fx[a] = (z[0], z[1], 0.0, 0.0, re, 0.0, vel_var)
                fage[a], nis[row] = 0, 0.0
            else:
                fb = frames[h + t - 1 - k]
                m = int(links["matched_prev"][row])
                dt = F(k + 1) if times is None else times[t] - (fb["time"] if h + t - 1 - k < h else times[t - 1 - k])
                fx[a], nis[row], fage[a] = step(fb["x"][m], fb["age"][m], z, dt, q, re)
            pos[row], vel[row], cov[row], age[row] = fx[a, 0:2], fx[a, 2:4], fx[a, 4:7], fage[a]
        frames.append(dict(count=c, rows=rows, x=fx, age=fage, time=None if times is None else times[t]))
    out = dict(pos=pos, vel=vel, cov=cov, nis=nis, age=age)
    if g == 0:
        return out, state
    return out, dict(frames=frames[-(max_gap + 1):])


def state_image(state):
    """The bytes of the device state the oracle's state stands for: a 64-byte header (int32 n_frames, int32 count[9], zeros), then with
    C = the sum of the frames' rows: fp64 [C][7] (px, py, vx, vy, a, b, c), then int32 age [C]; rows at or beyond a frame's count are
    zero with age -1.  -> uint8 [64 + 60 C]."""
    frames = state["frames"]
    head = np.zeros(HEADER_BYTES // 4, np.int32)
    head[0] = len(frames)
    cap = sum(f["rows"] for f in frames)
    x, age = np.zeros((cap, 7), F), np.full(cap, -1, np.int32)
    row = 0
    for j, f in enumerate(frames):
        head[1 + j] = f["count"]
        x[row:row + f["count"]], age[row:row + f["count"]] = f["x"], f["age"]
        row += f["rows"]
    return np.concatenate([head.view(np.uint8), x.reshape(-1).view(np.uint8), age.view(np.uint8)])
