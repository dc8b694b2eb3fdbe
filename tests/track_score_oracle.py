"""The scoring rule of gnn_cca_amd.tracking.TrackScorer restated with plain Python / numpy loops, for the tests and tools/time_track_score.py.
Everything is integer until result(), which uses Python ints, true division and math.fsum in a fixed order -- the same operations as the
product's host reduction, so the two agree bit for bit.  No fixture files: every case is generated from a seed or written out by hand."""
import itertools
import math

import numpy as np

TRACK_LIMIT = 2 ** 40


def new_state():
    """Nothing scored yet.  last: stream (p, c) -> its latest scored track; n: (p, t) -> scored detections of person p with track t."""
    return dict(last={}, n={}, scored=0, ignored=0, switches=0)


def add(state, ids, cam, node_track, node_ptr, max_ids, max_cams):
    """Scores the frames node_ptr[q] .. node_ptr[q + 1] in order, advancing `state` in place -> switched int32 [N] (-1: not scored)."""
    ids, cam, node_track = np.asarray(ids), np.asarray(cam), np.asarray(node_track)
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    switched = np.full(len(ids), -1, np.int32)
    for q in range(len(node_ptr) - 1):
        winner = {}   # (p, c) -> the largest valid node id of this frame
        for i in range(int(node_ptr[q]), int(node_ptr[q + 1])):
            p, c, t = int(ids[i]), int(cam[i]), int(node_track[i])
            if 0 <= p < max_ids and 0 <= c < max_cams and 0 <= t < TRACK_LIMIT:
                winner[(p, c)] = i   # (i ascends: a later one replaces an earlier one)
        for i in sorted(winner.values()):
            p, c, t = int(ids[i]), int(cam[i]), int(node_track[i])
            prev = state["last"].get((p, c))
            switched[i] = int(prev is not None and prev != t)
            state["switches"] += int(switched[i])
            state["last"][(p, c)] = t
            state["n"][(p, t)] = state["n"].get((p, t), 0) + 1
            state["scored"] += 1
        state["ignored"] += int(node_ptr[q + 1]) - int(node_ptr[q]) - len(winner)
    return switched


def counts(state):
    """scored, ignored, switches, pairs: what TrackScorer.counts holds."""
    return [state["scored"], state["ignored"], state["switches"], len(state["n"])]


def idtp_brute(table):
    """The largest total of `table` (a dense non-negative integer matrix) over one-to-one assignments of rows to columns, by trying every
    permutation: for small tables only."""
    table = np.asarray(table, dtype=np.int64)
    if table.shape[0] > table.shape[1]:
        table = table.T
    r, c = table.shape
    return max(sum(int(table[i, perm[i]]) for i in range(r)) for perm in itertools.permutations(range(c), r)) if r else 0


def idtp(cells):
    """The same maximum from scipy's rectangular assignment solver on the dense matrix of the non-zero cells."""
    from scipy.optimize import linear_sum_assignment
    persons, tracks = sorted({p for p, _, _ in cells}), sorted({t for _, t, _ in cells})
    pi, ti = {p: i for i, p in enumerate(persons)}, {t: i for i, t in enumerate(tracks)}
    dense = np.zeros((len(persons), len(tracks)), np.int64)
    for p, t, n in cells:
        dense[pi[p], ti[t]] = n
    rr, cc = linear_sum_assignment(dense, maximize=True)
    return int(dense[rr, cc].sum())


def result(state):
    """The dict TrackScorer.result() returns."""
    cells = [(p, t, n) for (p, t), n in sorted(state["n"].items())]   # ascending (p, t)
    total = sum(n for _, _, n in cells)
    if total == 0:
        raise ValueError("nothing was scored")
    row, col = {}, {}
    for p, t, n in cells:
        row[p] = row.get(p, 0) + n
        col[t] = col.get(t, 0) + n
    best_of_p = {p: max(n for q, _, n in cells if q == p) for p in row}
    best_of_t = {t: max(n for _, u, n in cells if u == t) for t in col}
    mt = pt = ml = 0
    for p in row:
        share = best_of_p[p] / row[p]
        if share >= 0.8:
            mt += 1
        elif share <= 0.2:
            ml += 1
        else:
            pt += 1
    top = idtp(cells)
    return {"detections": total, "ignored": state["ignored"], "ids": len(row), "tracks": len(col), "pairs": len(cells),
            "IDSW": state["switches"], "IDTP": top, "IDF1": top / total,
            "AssA": math.fsum(n * n / (row[p] + col[t] - n) for p, t, n in cells) / total,
            "purity": sum(best_of_t.values()) / total, "coverage": sum(best_of_p.values()) / total, "MT": mt, "PT": pt, "ML": ml,
            "tracks_per_id": len(cells) / len(row)}


def score(ids, cam, node_track, node_ptr, max_ids, max_cams):
    """One sequence from a fresh state -> (switched, counts, result dict)."""
    st = new_state()
    sw = add(st, ids, cam, node_track, node_ptr, max_ids, max_cams)
    return sw, counts(st), result(st)
