"""The motion rule of gnn_cca_amd.tracking (FrameLinker(motion='velocity')) restated with numpy, for the tests.  It reuses the pair tables
and the best-partner choice of tests/tracking_oracle.py with the PREDICTED positions passed in as the previous-frame positions; the
frames (outside), the levels (inside), the masks, the velocities and the carried history are plain Python loops.  With motion=False
nothing is predicted and the loops are the gap rule in frames-outside order.  No fixture files: every case is generated from a seed or
written out by hand."""
import numpy as np

import tracking_oracle as to

MAX_GAP = 8


def new_state():
    """No frame seen yet.  `frames`: the last min(M + 1, frames seen) frames, oldest first, each a dict(count, pos, vel, emb, track, succ)."""
    return dict(frames=[], next_id=0)


def _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state, motion, visit=None):
    """The rule: frames in order, levels 0 .. M inside each.  -> (pred: per batch row None or (gap, rank of the partner in its own frame),
    the combined frame list [history + batch] with their final succ flags and velocities, the number of history frames).
    visit(k, t, d, dcos, cost, ok) sees every table."""
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [0, {MAX_GAP}], not {max_gap!r}")
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    g = len(node_ptr) - 1
    hist = [dict(f, succ=np.array(f["succ"], bool)) for f in state["frames"]]
    h = len(hist)
    frames = list(hist)
    for q in range(g):
        v0 = int(node_ptr[q])
        c = max(int(summ["count"][q]), 0)
        frames.append(dict(count=c, pos=np.array(summ["pos"][v0:v0 + c], np.float64).reshape(c, 2), vel=np.zeros((c, 2), np.float64),
                           emb=np.array(summ["emb"][v0:v0 + c], np.float32).reshape(c, np.shape(summ["emb"])[1]), succ=np.zeros(c, bool)))
    pred = [[None] * frames[h + q]["count"] for q in range(g)]
    for t in range(g):       # a frame's velocities are final before any later frame looks at them
        fa = frames[h + t]
        for k in range(max_gap + 1):
            steps = np.float64(k + 1)
            gate = np.float64(max_step) * steps
            s = h + t - 1 - k
            if s < 0:
                continue
            fb = frames[s]
            ia = np.array([a for a in range(fa["count"]) if pred[t][a] is None], np.int64)
            ib = np.array([b for b in range(fb["count"]) if not fb["succ"][b]], np.int64)
            if not len(ia) or not len(ib):
                continue
            where = fb["pos"][ib]
            if motion:
                with np.errstate(invalid="ignore", over="ignore"):
                    where = fb["pos"][ib] + steps * fb["vel"][ib]   # one multiplication, one addition per component
            with np.errstate(invalid="ignore", over="ignore"):
                d, dcos, cost, ok = to.pair_tables(fa["pos"][ia], fa["emb"][ia], where, fb["emb"][ib], gate, lam, max_cos)
            if visit is not None:
                visit(k, t, d, dcos, cost, ok)
            fwd, bwd = to._best(cost, ok), to._best(cost.T, ok.T)   # ia, ib ascend: the smaller position is the smaller rank
            for i, j in enumerate(fwd):
                if j >= 0 and bwd[j] == i:
                    a, b = int(ia[i]), int(ib[j])
                    pred[t][a] = (k, b)
                    fb["succ"][b] = True
                    if motion:
                        fa["vel"][a] = (fa["pos"][a] - fb["pos"][b]) / steps   # one subtraction, one division per component
    return pred, frames, h


def link_motion(summ, node_ptr, max_step, lam=1.0, max_cos=None, max_gap=0, state=None, motion=True):
    """-> (dict(cluster_track [N], node_track [N], matched_prev [N], matched_gap [N], velocity [N, 2], next_id), new state)."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    n, g = len(summ["rank"]), len(node_ptr) - 1
    state = state if state is not None else new_state()
    pred, frames, h = _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state, motion)
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


def margins_motion(summ, node_ptr, max_step, lam, max_cos, max_gap, state=None, motion=True):
    """tracking_oracle.margins over every (frame, level) table of the rule, gate_k in place of max_step and the predicted positions in
    place of the previous ones: (best versus second-best admissible cost over every row and column with at least two admissible
    entries, |d - gate_k|, |dcos - max_cos|); inf where there is nothing to compare."""
    gaps = [np.inf, np.inf, np.inf]

    def visit(k, t, d, dcos, cost, ok):
        gate = np.float64(max_step) * np.float64(k + 1)
        gaps[1] = min(gaps[1], float(np.abs(d - gate).min()))
        if max_cos is not None:
            gaps[2] = min(gaps[2], float(np.abs(dcos - max_cos).min()))
        for table in (np.where(ok, cost, np.inf), np.where(ok, cost, np.inf).T):
            for row in table:
                fin = np.sort(row[np.isfinite(row)])
                if len(fin) >= 2:
                    gaps[0] = min(gaps[0], float(fin[1] - fin[0]))

    _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state if state is not None else new_state(), motion, visit)
    return tuple(gaps)


def level_tables(summ, node_ptr, max_step, lam, max_cos, max_gap, state=None, motion=True):
    """Every table the rule looks at, as a list of (k, t, d, dcos, cost, ok): for tests that count ties or pairs exactly on a gate."""
    seen = []
    _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state if state is not None else new_state(), motion, lambda *a: seen.append(a))
    return seen


def switches(person, track, node_ptr):
    """Identity switches of `track` against `person` (both per row, one row per detection): over a person's rows in frame order, the
    number of times the track differs from the one of that person's previous row."""
    node_ptr = np.asarray(node_ptr, np.int64)
    last, n_sw = {}, 0
    for q in range(len(node_ptr) - 1):
        for v in range(int(node_ptr[q]), int(node_ptr[q + 1])):
            p, t = int(person[v]), int(track[v])
            if p in last and last[p] != t:
                n_sw += 1
            last[p] = t
    return n_sw


def cross_sequence(rng, g, persons, r, speed=(0.3, 0.6), noise=0.05, p_hide=0.0, max_hide=1, arena=6.0):
    """People crossing each other: everybody walks a straight line at a constant speed drawn from `speed` (units per frame), from a start
    point towards a target point, both uniform in the arena, the whole walk shifted back by half the sequence so that the start point is
    reached in the middle of it.  Nobody bounces, nobody enters or leaves; the detected position is the true one plus normal noise; the
    order of the rows is permuted per frame.  With probability p_hide per visible frame a person who has been seen goes undetected for
    1 .. max_hide frames and keeps walking.  -> the summaries dict of tracking_gap_oracle.hide_sequence (one single-node cluster per
    detected person), with `person`: int64 [N], who each row is."""
    start, target = rng.uniform(0, arena, size=(persons, 2)), rng.uniform(0, arena, size=(persons, 2))
    way = target - start
    step = way / np.linalg.norm(way, axis=1, keepdims=True) * rng.uniform(speed[0], speed[1], size=(persons, 1))
    look = rng.standard_normal((persons, r)).astype(np.float32)
    hidden, seen_before = np.zeros(persons, np.int64), np.zeros(persons, bool)
    pos_rows, emb_rows, who, counts = [], [], [], []
    for q in range(g):
        seen = 0
        for p in rng.permutation(persons):
            at = start[p] + (q - g / 2.0) * step[p] + rng.normal(0, noise, size=2)
            emb = (look[p] + 0.05 * rng.standard_normal(r).astype(np.float32)).astype(np.float32)
            if seen_before[p] and hidden[p] == 0 and rng.random() < p_hide:
                hidden[p] = int(rng.integers(1, max_hide + 1))
            if hidden[p] > 0:
                hidden[p] -= 1
                continue
            pos_rows.append(at)
            emb_rows.append(emb)
            who.append(int(p))
            seen_before[p] = True
            seen += 1
        counts.append(seen)
    n = sum(counts)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32),
                pos=np.array(pos_rows, np.float64).reshape(n, 2), emb=np.array(emb_rows, np.float32).reshape(n, r), node_ptr=node_ptr,
                person=np.array(who, np.int64).reshape(n))
