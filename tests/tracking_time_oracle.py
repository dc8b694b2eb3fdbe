"""The linking rules of gnn_cca_amd.tracking with a TIME STAMP per frame (FrameLinker(...)(x, times=...)) restated with numpy, for the
tests: one walk, frames outside and levels inside, for every mode -- mutual best or the min-cost assignment, with or without the velocity
prediction.  It reuses the pair tables and the best-partner choice of tests/tracking_oracle.py and the assignment of
tests/tracking_assign_oracle.py; the frames, the levels, the masks, the times and the carried history are plain Python loops.

The rule.
  Time stamps.  A timed call gives one fp64 time per frame of the batch, in units of the nominal frame period: finite, strictly
    increasing, the first strictly greater than the last time of the previous call.  T[f] is the time of frame f over the combined list
    (the carried history, then the batch).
  Level order.  For frame t at level k the other frame is still s = t - 1 - k, counted in frames PRESENT; a shorter gap still wins, and
    the history still holds the last max_gap + 1 frames.
  Elapsed time.  dt = T[t] - T[s], one fp64 subtraction, replaces float64(k + 1) everywhere: gate = max_step * dt; with motion
    pred(b) = pos(b) + dt * vel(b) and vel(a) = (pos(a) - pos(b)) / dt -- each one operation, in the order of the untimed code, no FMA.
  Skipped tables.  A table with not (dt > 0 and dt <= max_dt) has no admissible pair and is skipped whole.  max_dt is None (max_gap + 1:
    a hole of one frame period consumes one unit of max_gap) or a finite number > 0.
  Everything else is the mode's own rule, unchanged: masks, the cosine term, max_cos, cost = d / gate + lam * dcos, ties, mutual best or
    the assignment with miss_cost, the numbering of fresh ids, and matched_gap (still the level k).
  Consequence.  With T = 0, 1, 2, ... continuing across calls dt is exactly k + 1 and every output equals the untimed oracles'.

Frames outside, levels inside is the order the velocities need; without motion it gives the levels-outside result of the gap oracles (a
table (k, t) depends only on tables (k' < k, t' < t) and (k' < k, t), whatever chooses the pairs inside a table, and a skipped table is an
empty one).  No fixture files: every case is generated from a seed or written out by hand."""
import math

import numpy as np

import tracking_assign_oracle as ta
import tracking_oracle as to

MAX_GAP = 8


def new_state():
    """No frame seen yet.  `frames`: the last min(M + 1, frames seen) frames, oldest first, each a dict(count, pos, vel, emb, track, succ,
    time)."""
    return dict(frames=[], next_id=0)


def check_times(times, g, last=None):
    """-> float64 [g]; ValueError unless `times` has g finite real entries, strictly increasing, the first after `last`."""
    seq = list(times)
    if len(seq) != g:
        raise ValueError(f"the batch has {g} frames, times has {len(seq)} entries")
    for v in seq:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"every time must be a finite real number, not {v!r}")
    t = np.array([float(v) for v in seq], np.float64)
    if (np.diff(t) <= 0).any():
        raise ValueError("times must be strictly increasing")
    if g and last is not None and not t[0] > last:
        raise ValueError(f"the first time, {t[0]}, is not after the previous call's last, {last}")
    return t


def _walk(summ, node_ptr, times, max_step, lam, max_cos, max_gap, state, max_dt=None, matching="mutual", miss_cost=None, motion=False,
          visit=None):
    """The rule: frames in order, levels 0 .. M inside each.  -> (pred: per batch row None or (gap, rank of the partner in its own frame),
    the combined frame list [history + batch] with their final succ flags, velocities and times, the number of history frames).
    visit(k, t, d, dcos, cost, ok, dt) sees every table that is not skipped."""
    if matching not in ta.MATCHINGS:
        raise ValueError(f"matching must be 'mutual' or 'optimal', not {matching!r}")
    if motion and matching == "optimal":
        raise ValueError("there is no motion under matching='optimal'")
    if miss_cost is not None and (matching != "optimal" or not math.isfinite(miss_cost) or not miss_cost > 0):
        raise ValueError(f"miss_cost must be None or, with matching='optimal', a finite number > 0, not {miss_cost!r}")
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [0, {MAX_GAP}], not {max_gap!r}")
    if max_dt is not None and (isinstance(max_dt, bool) or not math.isfinite(max_dt) or not max_dt > 0):
        raise ValueError(f"max_dt must be None or a finite number > 0, not {max_dt!r}")
    max_dt = np.float64(max_gap + 1 if max_dt is None else max_dt)
    pairs = ta.pairs_optimal if matching == "optimal" else ta.pairs_mutual
    miss = ta.default_miss_cost(lam, max_cos) if miss_cost is None else float(miss_cost)
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    g = len(node_ptr) - 1
    hist = [dict(f, succ=np.array(f["succ"], bool)) for f in state["frames"]]
    h = len(hist)
    times = check_times(times, g, hist[-1]["time"] if hist else None)
    frames = list(hist)
    for q in range(g):
        v0 = int(node_ptr[q])
        c = max(int(summ["count"][q]), 0)
        frames.append(dict(count=c, pos=np.array(summ["pos"][v0:v0 + c], np.float64).reshape(c, 2), vel=np.zeros((c, 2), np.float64),
                           emb=np.array(summ["emb"][v0:v0 + c], np.float32).reshape(c, np.shape(summ["emb"])[1]), succ=np.zeros(c, bool),
                           time=np.float64(times[q])))
    if matching == "optimal" and max([f["count"] for f in frames] + [int(np.diff(node_ptr).max()) if g else 0]) > ta.MAX_OPTIMAL_FRAME_NODES:
        raise ValueError(f"matching='optimal' takes frames of at most {ta.MAX_OPTIMAL_FRAME_NODES} detections")
    pred = [[None] * frames[h + q]["count"] for q in range(g)]
    for t in range(g):       # a frame's velocities are final before any later frame looks at them
        fa = frames[h + t]
        for k in range(max_gap + 1):
            s = h + t - 1 - k   # counted in frames present
            if s < 0:
                continue
            fb = frames[s]
            dt = fa["time"] - fb["time"]   # one fp64 subtraction
            if not (dt > 0 and dt <= max_dt):
                continue                   # the table is skipped whole
            gate = np.float64(max_step) * dt
            ia = np.array([a for a in range(fa["count"]) if pred[t][a] is None], np.int64)
            ib = np.array([b for b in range(fb["count"]) if not fb["succ"][b]], np.int64)
            if not len(ia) or not len(ib):
                continue
            where = fb["pos"][ib]
            if motion:
                with np.errstate(invalid="ignore", over="ignore"):
                    where = fb["pos"][ib] + dt * fb["vel"][ib]   # one multiplication, one addition per component
            with np.errstate(invalid="ignore", over="ignore"):
                d, dcos, cost, ok = to.pair_tables(fa["pos"][ia], fa["emb"][ia], where, fb["emb"][ib], gate, lam, max_cos)
            if visit is not None:
                visit(k, t, d, dcos, cost, ok, dt)
            for i, j in pairs(cost, ok, miss):   # ia, ib ascend: the smaller position is the smaller rank
                a, b = int(ia[i]), int(ib[j])
                pred[t][a] = (k, b)
                fb["succ"][b] = True
                if motion:
                    fa["vel"][a] = (fa["pos"][a] - fb["pos"][b]) / dt   # one subtraction, one division per component
    return pred, frames, h


def link_timed(summ, node_ptr, times, max_step, lam=1.0, max_cos=None, max_gap=0, state=None, max_dt=None, matching="mutual", miss_cost=None,
               motion=False):
    """-> (dict(cluster_track [N], node_track [N], matched_prev [N], matched_gap [N], velocity [N, 2] (zero without motion), next_id),
    new state)."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    n, g = len(summ["rank"]), len(node_ptr) - 1
    state = state if state is not None else new_state()
    pred, frames, h = _walk(summ, node_ptr, times, max_step, lam, max_cos, max_gap, state, max_dt, matching, miss_cost, motion)
    cluster_track, node_track = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    matched_prev, matched_gap = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    velocity = np.zeros((n, 2), np.float64)
    next_id = int(state["next_id"])
    for t in range(g):
        v0, v1 = int(node_ptr[t]), int(node_ptr[t + 1])
        f = frames[h + t]
        track = np.zeros(f["count"], np.int64)
        for c in range(f["count"]):
            if pred[t][c] is None:
                track[c] = next_id
                next_id += 1
            else:
                k, b = pred[t][c]
                track[c] = frames[h + t - 1 - k]["track"][b]
                matched_prev[v0 + c], matched_gap[v0 + c] = b, k
        f["track"] = track
        cluster_track[v0:v0 + f["count"]] = track
        velocity[v0:v0 + f["count"]] = f["vel"]
        for v in range(v0, v1):
            rk = int(summ["rank"][v])
            if 0 <= rk < f["count"]:
                node_track[v] = track[rk]
    out = dict(cluster_track=cluster_track, node_track=node_track, matched_prev=matched_prev, matched_gap=matched_gap, velocity=velocity,
               next_id=next_id)
    if g == 0:
        return out, state
    return out, dict(frames=frames[-(max_gap + 1):], next_id=next_id)


def margins_timed(summ, node_ptr, times, max_step, lam, max_cos, max_gap, state=None, max_dt=None, matching="mutual", miss_cost=None,
                  motion=False):
    """What the decisions of the rule hang on, over every table that is not skipped: (best versus second-best admissible cost over every
    row and column with at least two admissible entries, |d - gate|, |dcos - max_cos|); inf where there is nothing to compare."""
    gaps = [np.inf, np.inf, np.inf]

    def visit(k, t, d, dcos, cost, ok, dt):
        gate = np.float64(max_step) * dt
        gaps[1] = min(gaps[1], float(np.abs(d - gate).min()))
        if max_cos is not None:
            gaps[2] = min(gaps[2], float(np.abs(dcos - max_cos).min()))
        for table in (np.where(ok, cost, np.inf), np.where(ok, cost, np.inf).T):
            for row in table:
                fin = np.sort(row[np.isfinite(row)])
                if len(fin) >= 2:
                    gaps[0] = min(gaps[0], float(fin[1] - fin[0]))

    _walk(summ, node_ptr, times, max_step, lam, max_cos, max_gap, state if state is not None else new_state(), max_dt, matching, miss_cost,
          motion, visit)
    return tuple(gaps)


def level_tables(summ, node_ptr, times, max_step, lam, max_cos, max_gap, state=None, max_dt=None, matching="mutual", miss_cost=None,
                 motion=False):
    """Every table the rule looks at (the skipped ones are not among them), as a list of (k, t, d, dcos, cost, ok, dt)."""
    seen = []
    _walk(summ, node_ptr, times, max_step, lam, max_cos, max_gap, state if state is not None else new_state(), max_dt, matching, miss_cost,
          motion, lambda *a: seen.append(a))
    return seen


def drop_frames(summ, drop):
    """The sequence without the frames of `drop` -> (the shorter sequence, the indices of the frames that survive: their times)."""
    ptr = np.asarray(summ["node_ptr"], np.int64)
    keep = [q for q in range(len(ptr) - 1) if q not in set(drop)]
    rows = np.concatenate([np.arange(ptr[q], ptr[q + 1]) for q in keep] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = {k: summ[k][rows] for k in ("rank", "size", "n_cams", "pos", "emb", "person") if k in summ}
    out["count"] = summ["count"][keep]
    out["node_ptr"] = np.concatenate([[0], np.cumsum(np.diff(ptr)[keep])]).astype(np.int64)
    return out, np.array(keep, np.float64)
