"""numpy statement of gnn_cca_amd.rerank (the checker, not the product path): all-pairs distances per frame, the eight steps of
k-reciprocal re-ranking (libs/utils.py:578-644 of the reference, Zhong et al.) and the rank-R selection of eval_RANK
(inference.py:454-481), each with a `dtype` argument.  float64 is the measure every result is held against; float32 performs the
reference's own roundings, one operation at a time.

Ties and sum orders are part of the contract and are written out here: a ranking breaks ties to the smaller index (a stable sort), the
sums of steps 5 and 7 run over ascending column index, the sum of step 6 in rank order."""
import numpy as np


def half(k1):
    """h of step 3: int(np.around(k1 / 2.)) + 1 -- numpy rounds a half to the even neighbour."""
    return int(np.around(k1 / 2.)) + 1


def frame_distances(x, node_ptr, dtype=np.float64):
    """-> list of [n_g, n_g] matrices: sqrt of the sum of squared differences of the float32 rows `x`, over k ascending."""
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    out = []
    for g in range(len(node_ptr) - 1):
        f = x[node_ptr[g]:node_ptr[g + 1]]
        n = f.shape[0]
        acc = np.zeros((n, n), dtype=dtype)
        for k in range(f.shape[1]):
            d = f[:, None, k] - f[None, :, k]
            acc = acc + d * d
        out.append(np.sqrt(acc))
    return out


def _seq_sum(values, dtype):
    s = dtype(0)
    for v in values:
        s = dtype(s + v)
    return s


def rerank(D, k1=20, k2=6, lam=0.3, dtype=np.float64, debug=False):
    """Steps 1-8 on one frame's float32 matrix D -> [n, n] in `dtype`; with debug=True also a dict: O, rank (the full ranking [n, n]),
    prefix (how many of its entries are defined: min(max(k1 + 1, k2), n)), expansion (bool [n, n], X(i)), support (bool [n, n],
    V'[i] != 0), accepted / rejected / enlarged (how often the 2/3 test said yes, said no, and a yes added something to X(i))."""
    dtype = np.dtype(dtype).type
    D = np.asarray(D, dtype=np.float32)
    n = D.shape[0]
    K, h = k1 + 1, half(k1)
    # 1. normalise
    sq = (D.astype(dtype) * D.astype(dtype)).astype(dtype)
    cmax = sq.max(axis=0) if n else sq.sum(axis=0)
    O = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        if cmax[i] > 0:
            O[i, :] = sq[:, i] / cmax[i]
    # 2. rank: ascending, ties to the smaller index
    rank = np.stack([np.argsort(O[i], kind="stable") for i in range(n)]) if n else np.zeros((0, 0), dtype=np.int64)
    # 3. reciprocal sets
    FK, FH = np.zeros((n, n), dtype=bool), np.zeros((n, n), dtype=bool)
    for i in range(n):
        FK[i, rank[i, :min(K, n)]] = True
        FH[i, rank[i, :min(h, n)]] = True
    RK, RH = FK & FK.T, FH & FH.T
    # 4. expansion (against the ORIGINAL R_K(i)); the integer form of the reference's a > 2./3*b
    X = RK.copy()
    accepted = rejected = enlarged = 0
    for i in range(n):
        for c in np.flatnonzero(RK[i]):
            a, b = int((RH[c] & RK[i]).sum()), int(RH[c].sum())
            if 3 * a > 2 * b:
                accepted += 1
                enlarged += int((RH[c] & ~X[i]).any())
                X[i] |= RH[c]
            else:
                rejected += 1
    # 5. weights, the denominator summed over ascending column index
    V = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        idx = np.flatnonzero(X[i])
        w = np.exp(-O[i, idx]).astype(dtype)
        V[i, idx] = w / _seq_sum(w, dtype)
    # 6. query expansion, summed in rank order
    if k2 != 1:
        kq = min(k2, n)
        Vq = np.zeros_like(V)
        for i in range(n):
            s = np.zeros(n, dtype=dtype)
            for m in rank[i, :kq]:
                s = (s + V[m]).astype(dtype)
            Vq[i] = s / dtype(kq)
        V = Vq
    # 7. Jaccard, summed over ascending column index
    S = np.zeros((n, n), dtype=dtype)
    for c in range(n):
        S = (S + np.minimum(V[:, None, c], V[None, :, c])).astype(dtype)
    J = (dtype(1) - S / (dtype(2) - S)).astype(dtype)
    # 8. the python floats 1 - lam and lam, rounded once to `dtype` as numpy rounds them
    out = (J * dtype(1.0 - float(lam)) + O * dtype(float(lam))).astype(dtype)
    if not debug:
        return out
    return out, dict(O=O, rank=rank, prefix=min(max(K, k2), n), expansion=X, support=V != 0, accepted=accepted, rejected=rejected,
                     enlarged=enlarged)


def rerank_frames(mats, k1=20, k2=6, lam=0.3, dtype=np.float64):
    return [rerank(D, k1, k2, lam, dtype) for D in mats]


def select(D, cam, rank):
    """sel bool [n, n]: sel[i, j] iff j is among the min(rank, deg_i) cross-camera detections with the smallest D[i, .], ties to the smaller id."""
    D, cam = np.asarray(D), np.asarray(cam)
    n = D.shape[0]
    sel = np.zeros((n, n), dtype=bool)
    for i in range(n):
        cand = np.flatnonzero(cam != cam[i])
        order = cand[np.argsort(D[i, cand], kind="stable")]
        sel[i, order[:rank]] = True
    return sel


def rank_predictions(mats, node_ptr, cam, edge_index, rank=1):
    """-> int64 [E]: edge (i, j) is 1 iff j is selected by i or i by j, inside one frame."""
    edge_index = np.asarray(edge_index)
    frame_of = np.repeat(np.arange(len(node_ptr) - 1), np.diff(node_ptr))
    sels = [select(mats[g], np.asarray(cam)[node_ptr[g]:node_ptr[g + 1]], rank) for g in range(len(node_ptr) - 1)]
    pred = np.zeros(edge_index.shape[1], dtype=np.int64)
    for k, (a, b) in enumerate(edge_index.T.tolist()):
        g = frame_of[a]
        if frame_of[b] != g:
            continue
        la, lb = a - node_ptr[g], b - node_ptr[g]
        pred[k] = int(sels[g][la, lb] or sels[g][lb, la])
    return pred


def rank_gap(D, cam, rank):
    """The smallest gap at the rank-R boundary over the rows of D: the distance of the first unselected cross-camera candidate minus that
    of the last selected one (inf where a row selects all its candidates)."""
    D, cam = np.asarray(D, dtype=np.float64), np.asarray(cam)
    gap = np.inf
    for i in range(D.shape[0]):
        d = np.sort(D[i, cam != cam[i]])
        if 0 < rank < len(d):
            gap = min(gap, d[rank] - d[rank - 1])
    return gap
