"""FrameLinker(matching='optimal') of gnn_cca_amd.tracking restated for the tests: the min-cost assignment of one (level, frame pair) table
as the shortest-augmenting-path loops the kernel runs (the ALGORITHM is the contract: an optimum's total is unique, its pairs need not be),
a copy of tracking_gap_oracle's _walk / link_gap with the matcher as a parameter, and a brute-force optimum for small tables.  Levels,
gates, masks, cost and the ids are tracking_gap_oracle's; only the choice of pairs inside a table differs.  No fixture files."""
import math

import numpy as np

import tracking_gap_oracle as tg
import tracking_oracle as to

MAX_OPTIMAL_FRAME_NODES = 128
MATCHINGS = ("mutual", "optimal")


def default_miss_cost(lam, max_cos):
    """The dearest an admissible pair can be: d / gate <= 1, dcos <= max_cos (2 without one)."""
    return 1.0 + float(lam) * (float(max_cos) if max_cos is not None else 2.0)


def assign(w, ok):
    """w float64 [n, m], ok bool [n, m] (the edges) -> (col: per row its column or -1, the tree steps of the busiest row).  Rows are
    inserted in order over m + n columns; column m + i is row i's own `stay unlinked` column (0 for row i, no edge for any other row).
    Every operation is an elementwise fp64 one; the one reduction is the first minimum in ascending column order."""
    n, m = np.shape(w)
    nc, inf, none = m + n, math.inf, -1
    # no edge = +inf: (inf - u) - v = inf is never < minv, which is all `not an edge` has to mean
    full = [[float(w[i][j]) if ok[i][j] else inf for j in range(m)] + [0.0 if r == i else inf for r in range(n)] for i in range(n)]
    u, v, p = [0.0] * n, [0.0] * nc, [none] * nc
    most = 0
    for i in range(n):
        minv, way, used = [inf] * nc, [none] * nc, [False] * nc
        i0, j0, steps = i, none, 0
        while True:
            steps += 1
            assert steps <= min(n, m) + 1, (steps, n, m)   # the bound the kernel's loop is launched with
            delta, j1 = inf, none
            row, ui = full[i0], u[i0]
            for j in range(nc):
                if used[j]:
                    continue
                cur = (row[j] - ui) - v[j]
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                if minv[j] < delta:   # strict: a tie goes to the smaller column, real columns before the unlinked ones
                    delta, j1 = minv[j], j
            assert j1 != none and math.isfinite(delta)   # (row i0's own unlinked column is free whenever i0 is in the tree)
            u[i] += delta
            for j in range(nc):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            used[j1] = True
            if p[j1] == none:
                break
            i0, j0 = p[j1], j1
        most = max(most, steps)
        j = j1
        while True:   # flip the path back along way
            jp = way[j]
            p[j] = i if jp == none else p[jp]
            if jp == none:
                break
            j = jp
    col = np.full(n, -1, np.int64)
    for j in range(m):
        if p[j] != none:
            col[p[j]] = j
    return col, most


def total(w, col):
    return math.fsum(float(w[i][j]) for i, j in enumerate(col) if j >= 0)


def brute_force(w, ok):
    """The smallest sum of w over one-to-one sets of edges (the empty set: 0), by enumeration: for tables of up to about 6 x 6."""
    n, m = np.shape(w)

    def go(i, taken):
        if i == n:
            return 0.0
        best = go(i + 1, taken)
        for j in range(m):
            if ok[i][j] and not taken >> j & 1:
                best = min(best, float(w[i][j]) + go(i + 1, taken | 1 << j))
        return best

    return go(0, 0)


def pairs_mutual(cost, ok, miss_cost=None):
    fwd, bwd = to._best(cost, ok), to._best(cost.T, ok.T)
    return [(i, int(j)) for i, j in enumerate(fwd) if j >= 0 and bwd[j] == i]


def pairs_optimal(cost, ok, miss_cost):
    edge = ok & ~np.isnan(cost)   # in this mode a pair whose cost is NaN is not admissible
    with np.errstate(invalid="ignore"):
        col, _ = assign(cost - np.float64(miss_cost), edge)
    return [(i, int(j)) for i, j in enumerate(col) if j >= 0]


def _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state, matching="mutual", miss_cost=None, visit=None):
    """tracking_gap_oracle._walk with the choice of pairs as a parameter (everything else word for word)."""
    if matching not in MATCHINGS:
        raise ValueError(f"matching must be 'mutual' or 'optimal', not {matching!r}")
    if miss_cost is not None and (matching != "optimal" or not math.isfinite(miss_cost) or not miss_cost > 0):
        raise ValueError(f"miss_cost must be None or, with matching='optimal', a finite number > 0, not {miss_cost!r}")
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or not 0 <= max_gap <= tg.MAX_GAP:
        raise ValueError(f"max_gap must be an integer in [0, {tg.MAX_GAP}], not {max_gap!r}")
    pairs = pairs_optimal if matching == "optimal" else pairs_mutual
    miss = default_miss_cost(lam, max_cos) if miss_cost is None else float(miss_cost)
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
    if matching == "optimal" and max([f["count"] for f in frames] + [int(np.diff(node_ptr).max()) if g else 0]) > MAX_OPTIMAL_FRAME_NODES:
        raise ValueError(f"matching='optimal' takes frames of at most {MAX_OPTIMAL_FRAME_NODES} detections")
    pred = [[None] * frames[h + q]["count"] for q in range(g)]
    for k in range(max_gap + 1):
        gate = np.float64(max_step) * np.float64(k + 1)
        for t in range(g):
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
            for i, j in pairs(cost, ok, miss):   # ia, ib ascend: the smaller position is the smaller rank
                pred[t][int(ia[i])] = (k, int(ib[j]))
                fb["succ"][ib[j]] = True
    return pred, frames, h


def link_gap(summ, node_ptr, max_step, lam=1.0, max_cos=None, max_gap=0, state=None, matching="mutual", miss_cost=None):
    """tracking_gap_oracle.link_gap over the _walk above -> (dict(cluster_track, node_track, matched_prev, matched_gap, next_id), state)."""
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    n, g = len(summ["rank"]), len(node_ptr) - 1
    state = state if state is not None else tg.new_state()
    pred, frames, h = _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state, matching, miss_cost)
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


def level_tables(summ, node_ptr, max_step, lam, max_cos, max_gap, state=None, matching="optimal", miss_cost=None):
    """Every table the rule looks at under `matching`, as a list of (k, t, d, dcos, cost, ok)."""
    seen = []
    _walk(summ, node_ptr, max_step, lam, max_cos, max_gap, state if state is not None else tg.new_state(), matching, miss_cost,
          lambda *a: seen.append(a))
    return seen
