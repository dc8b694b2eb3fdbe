"""The camera-exclusive clustering rule in plain numpy (include/gnncca_mpn.h, gnncca_post_exclusive_frames): the SEQUENTIAL WALK, written
for reading, not for speed.  Per frame g with nodes node_ptr[g] .. node_ptr[g + 1] and edges edge_ptr[g] .. edge_ptr[g + 1]:

  1. active      edge k is active iff float64(scores[k]) >= th (a NaN is never active).
  2. candidates  the unordered pair {i, j} is a candidate iff edges (i, j) and (j, i) both exist in the frame and both are active.
  3. weight      w = min(scores[i -> j], scores[j -> i]), an exact float32.
  4. order       descending w; ties to the smaller lo = min(i, j), then to the smaller hi.
  5. clustering  every node its own cluster with camera mask 1 << cam; walk the candidates in order, merge the two clusters of a candidate
                 iff they differ and their masks are disjoint; the merged mask is the OR.
  6. outputs     labels[v] = smallest batch-global node id of v's cluster; predictions[k] = 1 iff k belongs to a candidate pair and
                 labels[src] == labels[dst]; n_clusters = the batch total; cut[g] = candidate pairs of frame g between two clusters;
                 flags[g] = 1 where a camera id of the frame lies outside [0, 64): every node its own cluster, predictions 0, cut 0.
"""
import numpy as np

MAX_CAMERAS = 64


def candidates(src, dst, scores, k0, k1, v0, v1, th):
    """The candidate pairs of one frame: list of (w float32, lo, hi, k_lo_hi, k_hi_lo) with batch-global node ids, unordered."""
    s64 = scores.astype(np.float64)
    where = {}
    for k in range(k0, k1):
        where.setdefault((int(src[k]), int(dst[k])), k)
    out = []
    for (i, j), k in where.items():
        if not (i < j and v0 <= i and j < v1):
            continue
        r = where.get((j, i))
        if r is None:
            continue
        if s64[k] >= th and s64[r] >= th:          # (False for a NaN)
            out.append((np.float32(min(scores[k], scores[r])), i, j, k, r))
    return out


def sort_candidates(cands):
    return sorted(cands, key=lambda c: (-float(c[0]), c[1], c[2]))


def exclusive_oracle(edge_index, scores, cam, node_ptr, edge_ptr, th):
    """edge_index int [2, E], scores float32 [E], cam int [N], node_ptr / edge_ptr [G + 1], th in (0, 1) ->
    dict(labels int32 [N], predictions int64 [E], n_clusters int, cut int32 [G], flags int32 [G])."""
    if not 0.0 < float(th) < 1.0:
        raise ValueError("th must lie strictly between 0 and 1")
    edge_index = np.asarray(edge_index)
    src, dst = edge_index[0], edge_index[1]
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    cam = np.asarray(cam)
    n, e, g = int(node_ptr[-1]), len(scores), len(node_ptr) - 1
    if len(src) != e or len(cam) != n or len(edge_ptr) != g + 1:
        raise ValueError("lengths disagree")
    labels = np.arange(n, dtype=np.int32)
    preds = np.zeros(e, dtype=np.int64)
    cut, flags = np.zeros(g, dtype=np.int32), np.zeros(g, dtype=np.int32)
    for f in range(g):
        v0, v1, k0, k1 = int(node_ptr[f]), int(node_ptr[f + 1]), int(edge_ptr[f]), int(edge_ptr[f + 1])
        if ((cam[v0:v1] < 0) | (cam[v0:v1] >= MAX_CAMERAS)).any():
            flags[f] = 1
            continue
        cluster = {v: [v] for v in range(v0, v1)}          # root (smallest member) -> members
        root = {v: v for v in range(v0, v1)}
        mask = {v: 1 << int(cam[v]) for v in range(v0, v1)}
        cands = sort_candidates(candidates(src, dst, scores, k0, k1, v0, v1, float(th)))
        for _w, i, j, _k, _r in cands:
            a, b = root[i], root[j]
            if a == b or (mask[a] & mask[b]):
                continue
            a, b = min(a, b), max(a, b)
            for v in cluster[b]:
                root[v] = a
            cluster[a] += cluster.pop(b)
            mask[a] |= mask.pop(b)
        for v in range(v0, v1):
            labels[v] = root[v]
        for _w, i, j, k, r in cands:
            if root[i] == root[j]:
                preds[k] = preds[r] = 1
            else:
                cut[f] += 1
    return {"labels": labels, "predictions": preds, "n_clusters": int((labels == np.arange(n)).sum()), "cut": cut, "flags": flags}


def plain_components(edge_index, scores, node_ptr, edge_ptr, th):
    """What prune_and_cluster gives at threshold th: (labels int32 [N], pruned int64 [E]) -- the connected components of the candidate
    pairs, a node's label the smallest node id of its component."""
    edge_index = np.asarray(edge_index)
    src, dst = edge_index[0], edge_index[1]
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    n = int(node_ptr[-1])
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    pruned = np.zeros(len(scores), dtype=np.int64)
    for f in range(len(node_ptr) - 1):
        for _w, i, j, k, r in candidates(src, dst, scores, int(edge_ptr[f]), int(edge_ptr[f + 1]), int(node_ptr[f]), int(node_ptr[f + 1]), float(th)):
            pruned[k] = pruned[r] = 1
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(n)], dtype=np.int32), pruned


def one_per_camera(labels, cam):
    """True iff no cluster of `labels` holds two nodes of one camera."""
    pairs = set()
    for l, c in zip(np.asarray(labels).tolist(), np.asarray(cam).tolist()):
        if (l, c) in pairs:
            return False
        pairs.add((l, c))
    return True


def mutual_pairs(n, pairs, weights):
    """A frame-local edge list from unordered pairs: both directions, grouped by source as build_graph_batch lays edges out.
    -> (src, dst, scores float32) with scores[i -> j] = scores[j -> i] = weights[pair]."""
    both = sorted([(i, j, w) for (i, j), w in zip(pairs, weights)] + [(j, i, w) for (i, j), w in zip(pairs, weights)])
    if not both:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    s, d, w = zip(*both)
    return np.asarray(s, np.int64), np.asarray(d, np.int64), np.asarray(w, np.float32)
