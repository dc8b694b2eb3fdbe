"""The rule of gnn_cca_amd.kalman (KalmanLinker) restated with numpy, for the tests.  It reuses the pair tables and the best-partner choice
of tests/tracking_oracle.py with the positions PREDICTED BY THE FILTER passed in as the previous-frame positions, and the link rule of
tests/track_smooth_oracle.py (`step`) for every commit; the frames (outside), the levels (inside), the masks, the variance gate, the
filtered states and the carried history are plain Python loops.

The rule.  Frames outside, levels k = 0 .. max_gap inside, as in tests/tracking_motion_oracle.py.  dt = float64(k + 1); with time stamps
dt = T[t] - T[t - 1 - k], and a table with not (dt > 0 and dt <= max_dt) is skipped whole (max_dt: None = max_gap + 1).  Every cluster
carries a filtered state x = (px, py, vx, vy, a, b, c) and an age.
  Candidates and prediction: at level k the clusters b of frame t - 1 - k that have no successor; b stands at pred(b) = p(b) + dt * v(b),
    one multiplication and one addition per component, from the FILTERED position and velocity.
  Pair rule: the shared one between the RAW pos(a) and pred(b): d = sqrt(dx*dx + dy*dy), gate = max_step * dt, the cosine term and max_cos
    unchanged, cost = d / gate + lam * dcos.  With max_nis a pair is admissible only if also (dx*dx + dy*dy) / s <= max_nis, s = a_ + r,
    a_ = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0, dt2 = dt*dt, dt3 = dt2*dt: the operations of track_smooth_oracle.step in its order.  A
    NaN is admissible with nobody.
  Matching: mutual best, ties to the smaller index, a shorter gap wins.  Commit: x(a), nis(a), age(a) = step(x(b), age(b), pos(a), dt, q, r).
  Births: a cluster without a predecessor starts as (z, 0, 0, r, 0, vel_var), age 0, nis 0.  Ids as the motion walk hands them out.
Consequences: the result does not depend on how a sequence is cut into calls, and track_smooth_oracle.smooth fed the links returns the
same trajectories.  No fixture files: every case is generated from a seed or written out by hand."""
import math

import numpy as np

import track_smooth_oracle as ts
import tracking_oracle as to
import tracking_time_oracle as tt

MAX_GAP = 8
F = np.float64


def new_state():
    """No frame seen yet.  `frames`: the last min(M + 1, frames seen) frames, oldest first, each a dict(count, rows, pos (raw), x float64
    [count, 7], age, nis, emb, track, succ, time (None without time stamps))."""
    return dict(frames=[], next_id=0)


def check_params(q, r, vel_var, max_nis):
    ts.check_params(q, r, vel_var)
    if max_nis is not None and (isinstance(max_nis, (bool, np.bool_)) or not isinstance(max_nis, (int, float, np.integer, np.floating))
                                or not math.isfinite(max_nis) or not max_nis > 0):
        raise ValueError(f"max_nis must be None or a finite number > 0, not {max_nis!r}")


def predicted_var(a, b, c, dt, q):
    """a_ of track_smooth_oracle.step: the same operations in the same order."""
    a, b, c, dt, q = F(a), F(b), F(c), F(dt), F(q)
    with np.errstate(all="ignore"):
        dt2 = dt * dt
        dt3 = dt2 * dt
        return ((a + (F(2.0) * dt) * b) + dt2 * c) + (q * dt3) / F(3.0)


def _walk(summ, node_ptr, max_step, q, r, vel_var, lam, max_cos, max_gap, max_nis, times, state, max_dt=None, visit=None):
    """The rule -> (the combined frame list [history + batch], every batch frame with pred: per cluster None or (gap, rank of the partner
    in its own frame), and its filtered x, age, nis; the number of history frames).  visit(dict) sees every table that is not skipped."""
    check_params(q, r, vel_var, max_nis)
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [0, {MAX_GAP}], not {max_gap!r}")
    if max_dt is not None and (isinstance(max_dt, bool) or not math.isfinite(max_dt) or not max_dt > 0):
        raise ValueError(f"max_dt must be None or a finite number > 0, not {max_dt!r}")
    max_dt = F(max_gap + 1 if max_dt is None else max_dt)
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    g = len(node_ptr) - 1
    hist = [dict(f, succ=np.array(f["succ"], bool)) for f in state["frames"]]
    h = len(hist)
    if hist and g and (hist[-1]["time"] is None) != (times is None):
        raise ValueError("a state written with time stamps is not continued without them, nor the reverse")
    if times is not None:
        times = tt.check_times(times, g, hist[-1]["time"] if hist else None)
    frames = list(hist)
    for f in range(g):
        v0, rows = int(node_ptr[f]), int(node_ptr[f + 1] - node_ptr[f])
        c = max(int(summ["count"][f]), 0)
        frames.append(dict(count=c, rows=rows, pos=np.array(summ["pos"][v0:v0 + c], F).reshape(c, 2), x=np.zeros((c, 7), F),
                           age=np.zeros(c, np.int32), nis=np.zeros(c, F),
                           emb=np.array(summ["emb"][v0:v0 + c], np.float32).reshape(c, np.shape(summ["emb"])[1]), succ=np.zeros(c, bool),
                           pred=[None] * c, time=None if times is None else F(times[f])))
    for t in range(g):       # a frame's filtered states are final before any later frame looks at them
        fa = frames[h + t]
        for k in range(max_gap + 1):
            s_ = h + t - 1 - k
            if s_ < 0:
                continue
            fb = frames[s_]
            if times is None:
                dt = F(k + 1)
            else:
                dt = fa["time"] - fb["time"]   # one fp64 subtraction
                if not (dt > 0 and dt <= max_dt):
                    continue                   # the table is skipped whole
            gate = F(max_step) * dt
            ia = np.array([a for a in range(fa["count"]) if fa["pred"][a] is None], np.int64)
            ib = np.array([b for b in range(fb["count"]) if not fb["succ"][b]], np.int64)
            if not len(ia) or not len(ib):
                continue
            with np.errstate(all="ignore"):
                where = fb["x"][ib, 0:2] + dt * fb["x"][ib, 2:4]   # one multiplication, one addition per component
                d, dcos, cost, ok = to.pair_tables(fa["pos"][ia], fa["emb"][ia], where, fb["emb"][ib], gate, lam, max_cos)
                dx = fa["pos"][ia][:, None, 0] - where[None, :, 0]
                dy = fa["pos"][ia][:, None, 1] - where[None, :, 1]
                svar = np.array([predicted_var(fb["x"][b, 4], fb["x"][b, 5], fb["x"][b, 6], dt, q) + F(r) for b in ib], F)
                nis = (dx * dx + dy * dy) / svar[None, :]
                if max_nis is not None:
                    ok = ok & (nis <= max_nis)   # (a NaN compares false)
            if visit is not None:
                visit(dict(k=k, t=t, d=d, dcos=dcos, cost=cost, ok=ok, dt=dt, nis=nis, s=svar, ia=ia, ib=ib))
            fwd, bwd = to._best(cost, ok), to._best(cost.T, ok.T)   # ia, ib ascend: the smaller position is the smaller rank
            for i, j in enumerate(fwd):
                if j >= 0 and bwd[j] == i:
                    a, b = int(ia[i]), int(ib[j])
                    fa["pred"][a] = (k, b)
                    fb["succ"][b] = True
                    fa["x"][a], fa["nis"][a], fa["age"][a] = ts.step(fb["x"][b], fb["age"][b], fa["pos"][a], dt, q, r)
        for a in range(fa["count"]):
            if fa["pred"][a] is None:   # a birth
                fa["x"][a] = (fa["pos"][a, 0], fa["pos"][a, 1], 0.0, 0.0, r, 0.0, vel_var)
                fa["age"][a], fa["nis"][a] = 0, 0.0
    return frames, h


def link_kalman(summ, node_ptr, max_step, q, r, vel_var, lam=1.0, max_cos=None, max_gap=0, max_nis=None, times=None, state=None,
                max_dt=None):
    """-> (dict(cluster_track [N], node_track [N], matched_prev [N], matched_gap [N], velocity [N, 2] (the filtered one), next_id, and
    the trajectories pos [N, 2], vel [N, 2], cov [N, 3], nis [N], age [N]), the state to carry)."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    n, g = len(summ["rank"]), len(node_ptr) - 1
    state = state if state is not None else new_state()
    frames, h = _walk(summ, node_ptr, max_step, q, r, vel_var, lam, max_cos, max_gap, max_nis, times, state, max_dt)
    cluster_track, node_track = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    matched_prev, matched_gap = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    pos, vel, cov = np.zeros((n, 2), F), np.zeros((n, 2), F), np.zeros((n, 3), F)
    nis, age = np.zeros(n, F), np.full(n, -1, np.int32)
    next_id = int(state["next_id"])
    for t in range(g):
        v0, v1 = int(node_ptr[t]), int(node_ptr[t + 1])
        f = frames[h + t]
        c = f["count"]
        track = np.zeros(c, np.int64)
        for a in range(c):
            if f["pred"][a] is None:
                track[a] = next_id
                next_id += 1
            else:
                k, b = f["pred"][a]
                track[a] = frames[h + t - 1 - k]["track"][b]
                matched_prev[v0 + a], matched_gap[v0 + a] = b, k
        f["track"] = track
        cluster_track[v0:v0 + c] = track
        pos[v0:v0 + c], vel[v0:v0 + c], cov[v0:v0 + c] = f["x"][:, 0:2], f["x"][:, 2:4], f["x"][:, 4:7]
        nis[v0:v0 + c], age[v0:v0 + c] = f["nis"], f["age"]
        for v in range(v0, v1):
            rk = int(summ["rank"][v])
            if 0 <= rk < c:
                node_track[v] = track[rk]
    out = dict(cluster_track=cluster_track, node_track=node_track, matched_prev=matched_prev, matched_gap=matched_gap, velocity=vel.copy(),
               next_id=next_id, pos=pos, vel=vel, cov=cov, nis=nis, age=age)
    if g == 0:
        return out, state
    return out, dict(frames=frames[-(max_gap + 1):], next_id=next_id)


def level_tables(summ, node_ptr, max_step, q, r, vel_var, lam=1.0, max_cos=None, max_gap=0, max_nis=None, times=None, state=None,
                 max_dt=None):
    """Every table the rule looks at (the skipped ones are not among them), as a list of dicts: k, t, d, dcos, cost, ok [A, B], dt, nis
    [A, B] (d^2 / s, whether or not max_nis gates by it), s [B], ia, ib (the ranks of the rows and columns in their frames)."""
    seen = []
    _walk(summ, node_ptr, max_step, q, r, vel_var, lam, max_cos, max_gap, max_nis, times, state if state is not None else new_state(), max_dt,
          seen.append)
    return seen


def margins(summ, node_ptr, max_step, q, r, vel_var, lam, max_cos, max_gap, max_nis=None, times=None, state=None, max_dt=None):
    """What the decisions of the rule hang on, over every table: (best versus second-best admissible cost over every row and column with
    at least two admissible entries, |d - gate|, |dcos - max_cos|, |nis - max_nis| inside the distance gate); inf where there is nothing
    to compare."""
    gaps = [np.inf] * 4
    for tab in level_tables(summ, node_ptr, max_step, q, r, vel_var, lam, max_cos, max_gap, max_nis, times, state, max_dt):
        gate = F(max_step) * tab["dt"]
        gaps[1] = min(gaps[1], float(np.abs(tab["d"] - gate).min()))
        if max_cos is not None:
            gaps[2] = min(gaps[2], float(np.abs(tab["dcos"] - max_cos).min()))
        if max_nis is not None and (tab["d"] <= gate).any():
            gaps[3] = min(gaps[3], float(np.abs(tab["nis"] - max_nis)[tab["d"] <= gate].min()))
        for table in (np.where(tab["ok"], tab["cost"], np.inf), np.where(tab["ok"], tab["cost"], np.inf).T):
            for row in table:
                fin = np.sort(row[np.isfinite(row)])
                if len(fin) >= 2:
                    gaps[0] = min(gaps[0], float(fin[1] - fin[0]))
    return tuple(gaps)


def points(frames, emb_dim=0):
    """frames: per frame a list of (x, y) -> the summaries of one-node clusters."""
    counts = [len(f) for f in frames]
    n = sum(counts)
    pos = np.array([p for f in frames for p in f], F).reshape(n, 2)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32), pos=pos,
                emb=np.zeros((n, emb_dim), np.float32), node_ptr=node_ptr)


# The hand-written variance-gate case.  Track X walks 0.5 per frame along y = 0 over frames 0 .. 4, track Y is born in frame 4 at (0, 10).
# Frame 5 shows a detection 0.9 beside where X is expected, (2.5, 0.9), and one 0.9 beside Y, (0.9, 10): both inside the distance gate 1.0.
GATE = dict(max_step=1.0, q=0.0, r=0.01, vel_var=1.0, lam=0.0, max_cos=None, max_gap=0, max_nis=9.0)


def gate_case():
    return points([[(0.5 * t, 0.0)] for t in range(4)] + [[(2.0, 0.0), (0.0, 10.0)], [(2.5, 0.9), (0.9, 10.0)]])


def check_gate_case(out, tables):
    """The numbers of the case from the oracle's tables (so that it is not vacuous), and what the rule makes of them in `out`."""
    last = [t for t in tables if t["t"] == 5]
    assert len(last) == 1 and last[0]["ia"].tolist() == [0, 1] and last[0]["ib"].tolist() == [0, 1]
    d, nis, s = last[0]["d"], last[0]["nis"], last[0]["s"]
    # both 0.9 away, inside the distance gate 1.0 (X's zero-velocity prior leaves its prediction about 1.5e-3 short of x = 2.5, which
    # adds about 1e-6 to an offset of 0.9 along y)
    assert abs(d[0, 0] - 0.9) < 1e-5 and abs(d[1, 1] - 0.9) < 1e-12 and d[0, 0] <= 1.0 and d[0, 1] > 5 and d[1, 0] > 5
    assert s[0] < 0.03 and nis[0, 0] > 27.0          # X: five collinear frames, a small predicted variance: 0.81 / s is far above 9
    assert s[1] == 1.0 + 0.01 + 0.01 and abs(nis[1, 1] - 0.81 / 1.02) < 1e-12   # Y: born a frame ago, s = r + vel_var + r
    assert not last[0]["ok"][0, 0] and last[0]["ok"][1, 1]
    assert out["cluster_track"].tolist() == [0, 0, 0, 0, 0, 1, 2, 1]            # X's detection starts a track, Y's continues Y
    assert out["matched_gap"].tolist() == [-1, 0, 0, 0, 0, -1, -1, 0] and out["age"].tolist() == [0, 1, 2, 3, 4, 0, 0, 1]
    assert out["nis"][7] == nis[1, 1] and out["nis"][7] <= 9.0
