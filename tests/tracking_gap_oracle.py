"""The gap-tolerant linking rule of gnn_cca_amd.tracking (FrameLinker(max_gap=M)) restated with numpy, for the tests.  It reuses the pair
tables and the best-partner choice of tests/tracking_oracle.py, so level 0 is that oracle's rule word for word; the levels, the masks
and the carried history are plain Python loops.  No fixture files: every case is generated from a seed or written out by hand."""
import numpy as np

import tracking_oracle as to

MAX_GAP = 8


def new_state():
    """No frame seen yet.  `frames`: the last min(M + 1, frames seen) frames, oldest first, each a dict(count, pos, emb, track, succ)."""
    return dict(frames=[], next_id=0)


def _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state, visit=None):
    """The levels of the rule.  -> (pred: per batch row None or (gap, rank of the partner in its own frame), the combined frame list
    [history + batch] with their final succ flags, the number of history frames).  visit(k, t, d, dcos, cost, ok) sees every table."""
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [0, {MAX_GAP}], not {max_gap!r}")
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    g = len(node_ptr) - 1
    hist = [dict(f, succ=np.array(f["succ"], bool)) for f in state["frames"]]
    h = len(hist)
    frames = list(hist)
    for q in range(g):
        v0 = int(node_ptr[q])
        k = max(int(summ["count"][q]), 0)
        frames.append(dict(count=k, pos=np.array(summ["pos"][v0:v0 + k], np.float64).reshape(k, 2),
                           emb=np.array(summ["emb"][v0:v0 + k], np.float32).reshape(k, np.shape(summ["emb"])[1]), succ=np.zeros(k, bool)))
    pred = [[None] * frames[h + q]["count"] for q in range(g)]
    for k in range(max_gap + 1):
        gate = np.float64(max_step) * np.float64(k + 1)
        for t in range(g):   # (independent of each other within a level: every cluster is in one (A-frame, B-frame) pair)
            s = h + t - 1 - k
            if s < 0:
                continue
            fa, fb = frames[h + t], frames[s]
            ia = np.array([a for a in range(fa["count"]) if pred[t][a] is None], np.int64)
            ib = np.array([b for b in range(fb["count"]) if not fb["succ"][b]], np.int64)
            if not len(ia) or not len(ib):
                continue
            d, dcos, cost, ok = to.pair_tables(fa["pos"][ia], fa["emb"][ia], fb["pos"][ib], fb["emb"][ib], gate, lam, max_cos)
            if visit is not None:
                visit(k, t, d, dcos, cost, ok)
            fwd, bwd = to._best(cost, ok), to._best(cost.T, ok.T)   # ia, ib ascend: the smaller position is the smaller rank
            for i, j in enumerate(fwd):
                if j >= 0 and bwd[j] == i:
                    pred[t][int(ia[i])] = (k, int(ib[j]))
                    fb["succ"][ib[j]] = True
    return pred, frames, h


def link_gap(summ, node_ptr, max_step, lam=1.0, max_cos=None, max_gap=0, state=None):
    """-> (dict(cluster_track [N], node_track [N], matched_prev [N], matched_gap [N], next_id), new state)."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    n, g = len(summ["rank"]), len(node_ptr) - 1
    state = state if state is not None else new_state()
    pred, frames, h = _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state)
    cluster_track, node_track = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    matched_prev, matched_gap = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
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
        for v in range(v0, v1):
            rk = int(summ["rank"][v])
            if 0 <= rk < f["count"]:
                node_track[v] = track[rk]
    out = dict(cluster_track=cluster_track, node_track=node_track, matched_prev=matched_prev, matched_gap=matched_gap, next_id=next_id)
    if g == 0:
        return out, state
    return out, dict(frames=frames[-(max_gap + 1):], next_id=next_id)


def margins_gap(summ, node_ptr, max_step, lam, max_cos, max_gap, state=None):
    """tracking_oracle.margins over every (level, frame) table of the rule, gate_k in place of max_step: (best versus second-best
    admissible cost over every row and column with at least two admissible entries, |d - gate_k|, |dcos - max_cos|); inf where there
    is nothing to compare."""
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

    _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state if state is not None else new_state(), visit)
    return tuple(gaps)


def level_tables(summ, node_ptr, max_step, lam, max_cos, max_gap, state=None):
    """Every table the rule looks at, as a list of (k, t, d, dcos, cost, ok): for tests that count ties or pairs exactly on a gate."""
    seen = []
    _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state if state is not None else new_state(), lambda *a: seen.append(a))
    return seen


def hide_sequence(rng, g, persons, r, noise=0.05, p_leave=0.15, p_enter=0.3, p_hide=0.1, max_hide=1, arena=20.0, empty=(), max_alive=70,
                  lattice=False):
    """tracking_oracle.walk_sequence plus occlusions: a person who is alive keeps moving every frame but, with probability p_hide per
    visible frame, goes undetected for 1 .. max_hide frames -- from the frame AFTER the first one that shows the person: nobody is
    occluded before having been seen.  In the frames of `empty` nobody is detected (everybody still moves, hidden spells run on).
    -> the same summaries dict (one single-node cluster per DETECTED person), plus `person`: int64 [N], who each row is."""
    alive = []   # [pos, emb, frames still hidden, person number, seen before]
    born = [0]

    def person():
        p = rng.integers(0, int(arena), size=2).astype(np.float64) if lattice else rng.uniform(0, arena, size=2)
        born[0] += 1
        return [p, rng.standard_normal(r).astype(np.float32), 0, born[0] - 1, False]

    for _ in range(persons):
        alive.append(person())
    pos_rows, emb_rows, who, counts = [], [], [], []
    for q in range(g):
        alive = [a for a in alive if rng.random() >= p_leave]
        while rng.random() < p_enter and len(alive) < max_alive:
            alive.append(person())
        order = rng.permutation(len(alive))
        alive = [alive[i] for i in order]
        seen = 0
        for a in alive:
            a[0] = a[0] + (rng.integers(-1, 2, size=2).astype(np.float64) if lattice else rng.normal(0, noise, size=2))
            look = (a[1] + 0.05 * rng.standard_normal(r).astype(np.float32)).astype(np.float32)
            if a[4] and a[2] == 0 and rng.random() < p_hide:
                a[2] = int(rng.integers(1, max_hide + 1))
            if a[2] > 0:
                a[2] -= 1
                continue
            if q in empty:
                continue
            pos_rows.append(a[0].copy())
            emb_rows.append(look)
            who.append(a[3])
            a[4] = True
            seen += 1
        counts.append(seen)
    n = sum(counts)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32),
                pos=np.array(pos_rows, np.float64).reshape(n, 2), emb=np.array(emb_rows, np.float32).reshape(n, r), node_ptr=node_ptr,
                person=np.array(who, np.int64).reshape(n))


def frames_of(summ, lo, hi):
    """Frames lo .. hi of a sequence as a sequence of its own (node_ptr starts at 0 again)."""
    ptr = np.asarray(summ["node_ptr"], np.int64)
    v0, v1 = int(ptr[lo]), int(ptr[hi])
    out = {k: summ[k][v0:v1] for k in ("rank", "size", "n_cams", "pos", "emb") if k in summ}
    out["count"], out["node_ptr"] = summ["count"][lo:hi], ptr[lo:hi + 1] - v0
    return out
