"""The rules of gnn_cca_amd.tracking restated with numpy, for the tests: plain loops for the sums (one addition per member, in ascending
node id), float64 throughout the matching.  No fixture files: every case is generated from a seed or written out by hand."""
import numpy as np

MAX_FRAME_NODES = 4096


def summaries(labels, node_ptr, xw, yw, cam, embeds=None, max_frame_nodes=MAX_FRAME_NODES):
    """-> dict(count [G], rank [N], size [N], n_cams [N], pos [N, 2], emb [N, R]) as gnncca_cluster_summaries defines them."""
    labels, node_ptr = np.asarray(labels, dtype=np.int64), np.asarray(node_ptr, dtype=np.int64)
    xw, yw, cam = np.asarray(xw, dtype=np.float64), np.asarray(yw, dtype=np.float64), np.asarray(cam)
    n, g = len(labels), len(node_ptr) - 1
    r = 0 if embeds is None else embeds.shape[1]
    emb_in = None if embeds is None else np.asarray(embeds, dtype=np.float32)
    count, rank = np.zeros(g, np.int32), np.zeros(n, np.int32)
    size, n_cams = np.zeros(n, np.int32), np.zeros(n, np.int32)
    pos, emb = np.zeros((n, 2), np.float64), np.zeros((n, r), np.float32)
    for q in range(g):
        v0, v1 = int(node_ptr[q]), int(node_ptr[q + 1])
        if v0 < 0 or v1 < v0 or v1 > n:
            count[q] = -1
            continue
        lab = labels[v0:v1]
        ok = v1 - v0 <= max_frame_nodes and bool(np.all((lab >= v0) & (lab < v1)))
        ok = ok and bool(np.all(labels[lab] == lab))
        if not ok:
            count[q] = -1
            rank[v0:v1] = -1
            continue
        roots = np.unique(lab)   # ascending
        count[q] = len(roots)
        index = {int(root): c for c, root in enumerate(roots)}
        members = [[] for _ in roots]
        for v in range(v0, v1):
            c = index[int(labels[v])]
            rank[v] = c
            members[c].append(v)
        for c, mem in enumerate(members):
            row = v0 + c
            sx, sy = np.float64(0.0), np.float64(0.0)
            acc = np.zeros(r, np.float32)
            for v in mem:
                sx = sx + xw[v]
                sy = sy + yw[v]
                if r:
                    acc = acc + emb_in[v]
            size[row], n_cams[row] = len(mem), len({int(cam[v]) for v in mem})
            pos[row, 0], pos[row, 1] = sx / np.float64(len(mem)), sy / np.float64(len(mem))
            if r:
                emb[row] = acc / np.float32(len(mem))
    return dict(count=count, rank=rank, size=size, n_cams=n_cams, pos=pos, emb=emb)


def pair_tables(pos_a, emb_a, pos_b, emb_b, max_step, lam=1.0, max_cos=None):
    """d, dcos, cost, admissible as [A, B] float64 / bool tables for the clusters a of the current and b of the previous frame.  Without
    embeddings in the rule (lam == 0 and no max_cos) dcos is None and cost = d / max_step."""
    pos_a, pos_b = np.asarray(pos_a, np.float64).reshape(-1, 2), np.asarray(pos_b, np.float64).reshape(-1, 2)
    na_, nb_ = len(pos_a), len(pos_b)
    dx = pos_a[:, None, 0] - pos_b[None, :, 0]
    dy = pos_a[:, None, 1] - pos_b[None, :, 1]
    d = np.sqrt(dx * dx + dy * dy)
    ok = d <= max_step
    need = lam != 0 or max_cos is not None
    if not need:
        return d, None, d / max_step, ok
    ea, eb = np.asarray(emb_a, np.float64).reshape(na_, -1), np.asarray(emb_b, np.float64).reshape(nb_, -1)
    dot, na, nb = np.zeros((na_, nb_)), np.zeros((na_, 1)), np.zeros((1, nb_))
    for k in range(ea.shape[1]):   # a plain loop: one addition per column
        dot = dot + ea[:, k, None] * eb[None, :, k]
        na = na + ea[:, k, None] * ea[:, k, None]
        nb = nb + eb[None, :, k] * eb[None, :, k]
    with np.errstate(divide="ignore", invalid="ignore"):
        dcos = 1.0 - dot / (np.sqrt(na) * np.sqrt(nb))
    dcos = np.where((na == 0) | (nb == 0), 1.0, dcos)
    cost = d / max_step + lam * dcos
    if max_cos is not None:
        ok = ok & (dcos <= max_cos)
    return d, dcos, cost, ok


def _best(cost, ok):
    """Per row the admissible column of smallest cost, ties to the smaller column; -1 without one."""
    out = np.full(cost.shape[0], -1, np.int64)
    if cost.shape[1]:
        c = np.where(ok, cost, np.inf)
        arg = np.argmin(c, axis=1)   # the first minimum: the smaller index
        has = ok.any(axis=1)
        out[has] = arg[has]
    return out


def match(pos_a, emb_a, pos_b, emb_b, max_step, lam=1.0, max_cos=None):
    """matched[a] = b iff fwd[a] == b and bwd[b] == a, else -1."""
    _, _, cost, ok = pair_tables(pos_a, emb_a, pos_b, emb_b, max_step, lam, max_cos)
    fwd, bwd = _best(cost, ok), _best(cost.T, ok.T)
    return np.array([b if b >= 0 and bwd[b] == a else -1 for a, b in enumerate(fwd)], dtype=np.int64).reshape(-1)


def new_state():
    return dict(count=0, pos=np.zeros((0, 2)), emb=np.zeros((0, 0), np.float32), track=np.zeros(0, np.int64), next_id=0)


def link(summ, node_ptr, max_step, lam=1.0, max_cos=None, state=None):
    """-> (dict(cluster_track [N], node_track [N], matched_prev [N], next_id), new state).  `summ`: the dict `summaries` returns."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    n, g = len(summ["rank"]), len(node_ptr) - 1
    state = dict(state) if state is not None else new_state()
    cluster_track, node_track = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    matched_prev = np.full(n, -1, np.int32)
    next_id = int(state["next_id"])
    prev_pos, prev_emb, prev_track = state["pos"][:state["count"]], state["emb"][:state["count"]], state["track"][:state["count"]]
    for q in range(g):
        v0, v1 = int(node_ptr[q]), int(node_ptr[q + 1])
        k = max(int(summ["count"][q]), 0)
        pos, emb = summ["pos"][v0:v0 + k], summ["emb"][v0:v0 + k]
        m = match(pos, emb, prev_pos, prev_emb, max_step, lam, max_cos) if k and len(prev_pos) else np.full(k, -1, np.int64)
        track = np.zeros(k, np.int64)
        for c in range(k):
            if m[c] >= 0:
                track[c] = prev_track[m[c]]
            else:
                track[c] = next_id
                next_id += 1
        cluster_track[v0:v0 + k], matched_prev[v0:v0 + k] = track, m
        for v in range(v0, v1):
            rk = int(summ["rank"][v])
            if 0 <= rk < k:
                node_track[v] = track[rk]
        prev_pos, prev_emb, prev_track = pos, emb, track
    if g:
        state = dict(count=len(prev_track), pos=np.array(prev_pos), emb=np.array(prev_emb), track=np.array(prev_track), next_id=next_id)
    return dict(cluster_track=cluster_track, node_track=node_track, matched_prev=matched_prev, next_id=next_id), state


def margins(summ, node_ptr, max_step, lam, max_cos, state=None):
    """The smallest gaps of a sequence, on the oracle's own numbers: (best versus second-best admissible cost over every row and column
    with at least two admissible entries, |d - max_step| over all pairs, |dcos - max_cos| over all pairs).  inf where
    there is nothing to compare."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    state = state if state is not None else new_state()
    prev_pos, prev_emb = state["pos"][:state["count"]], state["emb"][:state["count"]]
    gap_cost = gap_d = gap_cos = np.inf
    for q in range(len(node_ptr) - 1):
        v0 = int(node_ptr[q])
        k = max(int(summ["count"][q]), 0)
        pos, emb = summ["pos"][v0:v0 + k], summ["emb"][v0:v0 + k]
        if k and len(prev_pos):
            d, dcos, cost, ok = pair_tables(pos, emb, prev_pos, prev_emb, max_step, lam, max_cos)
            gap_d = min(gap_d, float(np.abs(d - max_step).min()))
            if max_cos is not None:
                gap_cos = min(gap_cos, float(np.abs(dcos - max_cos).min()))
            for table in (np.where(ok, cost, np.inf), np.where(ok, cost, np.inf).T):
                for row in table:
                    fin = np.sort(row[np.isfinite(row)])
                    if len(fin) >= 2:
                        gap_cost = min(gap_cost, float(fin[1] - fin[0]))
        prev_pos, prev_emb = pos, emb
    return gap_cost, gap_d, gap_cos


def walk_sequence(rng, g, persons, r, noise=0.05, p_leave=0.15, p_enter=0.3, arena=20.0, max_alive=70, lattice=False, empty=()):
    """A synthetic sequence of g frames given as per-frame SUMMARIES (one cluster per person, positions moved by noise, births and
    deaths): -> (summ dict with count, rank, pos, emb, node_ptr).  Every cluster is a single node, so rank is 0 .. count - 1 per frame.
    lattice=True: integer coordinates, integer steps (exact distances, exact ties).  empty: frames in which nobody is detected."""
    alive = []   # (pos, emb)

    def person():
        p = rng.integers(0, int(arena), size=2).astype(np.float64) if lattice else rng.uniform(0, arena, size=2)
        return [p, rng.standard_normal(r).astype(np.float32)]

    for _ in range(persons):
        alive.append(person())
    pos_rows, emb_rows, counts = [], [], []
    for q in range(g):
        if q in empty:
            counts.append(0)
            continue
        alive = [a for a in alive if rng.random() >= p_leave]
        while rng.random() < p_enter and len(alive) < max_alive:
            alive.append(person())
        order = rng.permutation(len(alive))
        alive = [alive[i] for i in order]
        for a in alive:
            a[0] = a[0] + (rng.integers(-1, 2, size=2).astype(np.float64) if lattice else rng.normal(0, noise, size=2))
            pos_rows.append(a[0].copy())
            emb_rows.append((a[1] + 0.05 * rng.standard_normal(r).astype(np.float32)).astype(np.float32))
        counts.append(len(alive))
    n = sum(counts)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rank = np.concatenate([np.arange(c) for c in counts]).astype(np.int32) if n else np.zeros(0, np.int32)
    return dict(count=np.array(counts, np.int32), rank=rank, size=np.ones(n, np.int32), n_cams=np.ones(n, np.int32),
                pos=np.array(pos_rows, np.float64).reshape(n, 2), emb=np.array(emb_rows, np.float32).reshape(n, r), node_ptr=node_ptr)
