"""Numpy restatement of the two backwards of the graph build (csrc/graph_grads.cuh), in fp32 or fp64.  TEST INFRASTRUCTURE.

`edges_backward` is written the way the kernel computes -- per frame, grad_r = C r + diag(alpha) r + 1e-6 beta 1^T, the slot of an edge and
of its reverse derived from the plan (src_order, edge_ptr, camera ranks), never by searching the edge list -- so that pinning it to the
reference's autograd (tests/test_graph_grads_oracle.py) checks the kernel's algebra and index arithmetic on the CPU.
`normalize_backward` is gx = (gy - y sum_rows(gy y)) / nrm of y = x / max(||x[:, c]||, 1e-12).
"""
import numpy as np


def normalize(x, dtype):
    x = np.asarray(x, dtype=dtype)
    nrm = np.maximum(np.sqrt((x * x).sum(axis=0, dtype=dtype)), dtype(1e-12))
    return (x / nrm).astype(dtype)


def normalize_backward(x, gy, dtype):
    x, gy = np.asarray(x, dtype=dtype), np.asarray(gy, dtype=dtype)
    nrm = np.maximum(np.sqrt((x * x).sum(axis=0, dtype=dtype)), dtype(1e-12))
    y = x / nrm
    s = (gy * y).sum(axis=0, dtype=dtype)
    return ((gy - y * s) / nrm).astype(dtype)


def plan(id_cam, graph_sizes):
    """(graph_ptr, src_order, edge_ptr) as gnncca_plan_frames lays them out: sources frame by frame, cameras ascending inside a frame,
    node ids ascending inside a camera; a source's targets are the frame's nodes of the other cameras in ascending id."""
    id_cam = np.asarray(id_cam)
    sizes = np.asarray(graph_sizes, dtype=np.int64)
    graph_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    src_order, edge_ptr = [], [0]
    for g in range(len(sizes)):
        gs, ge = graph_ptr[g], graph_ptr[g + 1]
        cams = id_cam[gs:ge]
        order = gs + np.argsort(cams, kind="stable")
        for i in order:
            src_order.append(int(i))
            edge_ptr.append(edge_ptr[-1] + int((cams != id_cam[i]).sum()))
    return graph_ptr, np.asarray(src_order, dtype=np.int64), np.asarray(edge_ptr, dtype=np.int64)


def forward_attrs(r, id_cam, graph_sizes, dtype):
    """(edge_index [2, E], emb [E], cos [E]) of the normalised table r in the reference's edge order."""
    r = np.asarray(r, dtype=dtype)
    graph_ptr, src_order, edge_ptr = plan(id_cam, graph_sizes)
    id_cam = np.asarray(id_cam)
    graph_of = np.repeat(np.arange(len(graph_sizes)), np.asarray(graph_sizes, dtype=np.int64))
    rows, cols = [], []
    for i in src_order:
        gs, ge = graph_ptr[graph_of[i]], graph_ptr[graph_of[i] + 1]
        tg = np.arange(gs, ge)[id_cam[gs:ge] != id_cam[i]]
        rows.append(np.full(len(tg), i)), cols.append(tg)
    row = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    col = np.concatenate(cols).astype(np.int64) if cols else np.zeros(0, np.int64)
    a, b = r[row], r[col]
    diff = (a - b) + dtype(1e-6)
    emb = np.sqrt((diff * diff).sum(axis=1, dtype=dtype))
    na = np.maximum(np.sqrt((a * a).sum(axis=1, dtype=dtype)), dtype(1e-8))
    nb = np.maximum(np.sqrt((b * b).sum(axis=1, dtype=dtype)), dtype(1e-8))
    cos = (a * b).sum(axis=1, dtype=dtype) / (na * nb)
    return np.stack([row, col]), emb.astype(dtype), cos.astype(dtype)


def edges_backward(r, emb, cos, g_emb, g_cos, id_cam, graph_sizes, dtype):
    """grad_r [N, R] from the upstream gradients of the emb / cos columns (all [E], the forward's edge order)."""
    r = np.asarray(r, dtype=dtype)
    emb, cos, g_emb, g_cos = (np.asarray(v, dtype=dtype) for v in (emb, cos, g_emb, g_cos))
    id_cam = np.asarray(id_cam)
    graph_ptr, src_order, edge_ptr = plan(id_cam, graph_sizes)
    n = r.shape[0]
    pos = np.empty(n, dtype=np.int64)
    pos[src_order] = np.arange(n)
    nrm = np.maximum(np.sqrt((r * r).sum(axis=1, dtype=dtype)), dtype(1e-8))
    out = np.zeros_like(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        p_all = np.where(emb != 0, g_emb / emb, dtype(0)).astype(dtype)
    for g in range(len(graph_sizes)):
        gs, ge = int(graph_ptr[g]), int(graph_ptr[g + 1])
        ng = ge - gs
        if ng == 0:
            continue
        cams = id_cam[gs:ge]
        idx = np.arange(gs, ge)
        # slot of (i -> j): edge_ptr[pos_i] + (j - gs) - #(nodes of i's camera below j)
        same_below = np.stack([np.concatenate([[0], np.cumsum(cams == cams[t])[:-1]]) for t in range(ng)])   # [i][j]
        slot = edge_ptr[pos[idx]][:, None] + (idx - gs)[None, :] - same_below
        valid = cams[:, None] != cams[None, :]
        slot = np.where(valid, slot, 0)
        P = np.where(valid, p_all[slot] if len(p_all) else 0, 0).astype(dtype)           # P[i][j] = p of (i -> j); P.T = p of the reverse
        Q = np.where(valid, g_cos[slot] if len(g_cos) else 0, 0).astype(dtype)
        QC = np.where(valid, (g_cos * cos)[slot] if len(g_cos) else 0, 0).astype(dtype)
        ps = P + P.T
        ni = nrm[gs:ge]
        Cm = (Q + Q.T) / (ni[:, None] * ni[None, :]) - ps
        alpha = ps.sum(axis=1, dtype=dtype) - (QC + QC.T).sum(axis=1, dtype=dtype) / (ni * ni)
        beta = (P - P.T).sum(axis=1, dtype=dtype)
        rg = r[gs:ge]
        out[gs:ge] = Cm @ rg + alpha[:, None] * rg + dtype(1e-6) * beta[:, None]
    return out.astype(dtype)


def graph_build_backward(a, dtype, g_x=None, g_ea=None, g_reid=None, normalize_inputs=True):
    """(d_node, d_reid) of a fixture-shaped dict `a` (raw embeddings, id_cam, graph_sizes, modes): the whole chain in `dtype`."""
    node_raw, reid_raw = np.asarray(a["node_embeds_raw"], dtype=dtype), np.asarray(a["reid_embeds_raw"], dtype=dtype)
    g_x = np.asarray(a["g_x"] if g_x is None else g_x, dtype=dtype)
    g_ea = np.asarray(a["g_edge_attr"] if g_ea is None else g_ea, dtype=dtype)
    if g_reid is None and "g_reid" in a:
        g_reid = a["g_reid"]
    r = normalize(reid_raw, dtype) if normalize_inputs else reid_raw
    d_r = np.zeros_like(r)
    if not bool(a["only_dist"]) and g_ea.shape[0] > 0:
        _, emb, cos = forward_attrs(r, a["id_cam"], a["graph_sizes"], dtype)
        ce = 0 if bool(a["only_appearance"]) else 2
        d_r = edges_backward(r, emb, cos, g_ea[:, ce], g_ea[:, ce + 1], a["id_cam"], a["graph_sizes"], dtype)
    if g_reid is not None:
        d_r = d_r + np.asarray(g_reid, dtype=dtype)
    if not normalize_inputs:
        return g_x, d_r
    return normalize_backward(node_raw, g_x, dtype), normalize_backward(reid_raw, d_r, dtype)
