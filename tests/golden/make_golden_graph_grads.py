#!/usr/bin/env python3
"""Golden vectors for the BACKWARD of SURVEY.md 8f row N1 (graph construction + edge attributes): the gradients of random upstream
gradients on `x`, `edge_attr` (and, in one case, the normalised reid table) with respect to the RAW embeddings, produced by torch
autograd through the REFERENCE's own statements.  Run in the build container only (needs the reference checkout):

    python tests/golden/make_golden_graph_grads.py

Like make_golden_graph.py (whose stand-ins and frame generator it imports) this reads inference.py:189-279 AT RUN TIME and executes
the lines unmodified on synthetic frames -- here with requires_grad on the raw embeddings, once in fp32 and once in fp64; nothing of
the reference's text is stored, only numbers: inputs, upstream gradients, d_node{32,64}, d_reid{32,64} -> tests/golden/graph_grads/*.npz
(a subdirectory: test_gpu_graph_build.py globs tests/golden/graph_*.npz for forward cases).

A frame whose detections all sit on one camera has no edge, and the reference's statements cannot process it (sklearn refuses empty
arrays, torch.min an empty tensor).  The case `camera_only` therefore appends such a group's detections to the embedding TABLES only
(they take part in F.normalize over the whole batch, nothing gathers them) and runs the statements on the normal frame; the stored
upstream gradient on `x` is zero in those rows, where the reference has no row.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_graph import make_frame, run_reference  # noqa: E402

OUT = os.path.join(HERE, "graph_grads")


def grads_of(frames, node_raw, reid_raw, max_dist, g_x, g_ea, g_reid, dtype, modes):
    node = node_raw.to(dtype).clone().requires_grad_()
    reid = reid_raw.to(dtype).clone().requires_grad_()
    batch, _, reid_n = run_reference(frames, node, reid, max_dist, **modes)
    n_x = batch.x.shape[0]
    outs, ups = [batch.x, batch.edge_attr], [g_x[:n_x].to(batch.x.dtype), g_ea.to(batch.edge_attr.dtype)]
    if g_reid is not None:
        outs.append(reid_n)
        ups.append(g_reid.to(dtype))
    keep = [k for k, o in enumerate(outs) if o.requires_grad]   # only_dist: edge_attr does not depend on the embeddings
    d_node, d_reid = torch.autograd.grad([outs[k] for k in keep], [node, reid], [ups[k] for k in keep], allow_unused=True)
    d_reid = torch.zeros_like(reid) if d_reid is None else d_reid   # only_dist: no path from the reid table to an output
    return batch, d_node.detach().numpy(), d_reid.detach().numpy()


def save_case(name, frames, d_node, d_reid, max_dist, seed, extra_rows=None, reid_upstream=False, **modes):
    n_frames = sum(len(f) for f in frames)
    n_tot = n_frames + (len(extra_rows) if extra_rows is not None else 0)
    g = torch.Generator().manual_seed(seed)
    node_raw = torch.randn(n_tot, d_node, generator=g)
    reid_raw = torch.randn(n_tot, d_reid, generator=g) + 0.5
    n_attr = 2 if (modes.get("only_appearance") or modes.get("only_dist")) else 4
    n_edges = sum(len(f) ** 2 - int((np.bincount(f["id_cam"].values) ** 2).sum()) for f in frames)
    g_x = torch.randn(n_tot, d_node, generator=g)
    g_x[n_frames:] = 0.0
    g_ea = torch.randn(n_edges, n_attr, generator=g)
    g_reid = torch.randn(n_tot, d_reid, generator=g) * 0.1 if reid_upstream else None
    batch, dn32, dr32 = grads_of(frames, node_raw, reid_raw, max_dist, g_x, g_ea, g_reid, torch.float32, modes)
    _, dn64, dr64 = grads_of(frames, node_raw, reid_raw, max_dist, g_x, g_ea, g_reid, torch.float64, modes)
    assert batch.edge_attr.shape == (n_edges, n_attr)
    all_frames = list(frames) + ([extra_rows] if extra_rows is not None else [])
    rec = {
        "graph_sizes": np.array([len(f) for f in all_frames], dtype=np.int64),
        "xw": np.concatenate([f["xw"].values for f in all_frames]), "yw": np.concatenate([f["yw"].values for f in all_frames]),
        "id": np.concatenate([f["id"].values for f in all_frames]), "id_cam": np.concatenate([f["id_cam"].values for f in all_frames]),
        "max_dist": np.asarray(list(max_dist) + ([1.0] if extra_rows is not None else []), dtype=np.float64),
        "node_embeds_raw": node_raw.numpy(), "reid_embeds_raw": reid_raw.numpy(),
        "only_appearance": np.bool_(modes.get("only_appearance", False)), "only_dist": np.bool_(modes.get("only_dist", False)),
        "edge_index": batch.edge_index.numpy(), "g_x": g_x.numpy(), "g_edge_attr": g_ea.numpy(),
        "d_node32": dn32, "d_node64": dn64, "d_reid32": dr32, "d_reid64": dr64,
    }
    if g_reid is not None:
        rec["g_reid"] = g_reid.numpy()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez(path, **rec)
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    print(f"{name:18s} N={n_tot:3d} E={n_edges:5d} R={d_reid:3d} e_ref node {rel(dn32, dn64):.2e} reid {rel(dr32, dr64):.2e} "
          f"{os.path.getsize(path) // 1024} KiB")


def main():
    rng = np.random.default_rng(21)
    f1 = make_frame(rng, [0] * 4 + [1] * 3 + [2] * 5, 6, 10)
    save_case("one_frame", [f1], 8, 256, [37.5], 301)
    frames = [make_frame(rng, [0] * 3 + [2] * 2, 4, 1), make_frame(rng, [0] * 5 + [1] * 4 + [2] * 6 + [3] * 3, 8, 2),
              make_frame(rng, [1] * 2 + [3] * 2, 3, 3)]
    save_case("batch3", frames, 8, 32, [20.0, 33.0, 7.0], 302)
    fs = make_frame(rng, [0, 1, 0, 2, 1, 0, 2, 2, 1], 5, 4, shuffle=True)   # cameras interleaved -> `row` not sorted
    save_case("interleaved", [fs, make_frame(rng, [0] * 2 + [1] * 2, 2, 5)], 8, 16, [15.0, 15.0], 303)
    big = make_frame(rng, [0] * 30 + [1] * 25 + [2] * 15, 20, 6)            # 70 detections: two candidate chunks; R = 37: no multiple of 4
    save_case("frame70", [big], 8, 37, [50.0], 304)
    lone = make_frame(rng, [1] * 4, 3, 8)                                     # four detections on ONE camera: no edge, zero reid rows
    save_case("camera_only", [make_frame(rng, [0] * 3 + [1] * 4 + [2] * 2, 5, 7)], 8, 24, [25.0], 305, extra_rows=lone)
    save_case("only_appearance", [f1], 8, 16, [37.5], 306, only_appearance=True)
    save_case("only_dist", [f1], 8, 16, [37.5], 307, only_dist=True)
    t32 = make_frame(rng, sum(([c] * 8 for c in range(4)), []), 12, 9)       # the Terrace-shaped 4 x 8 frame
    save_case("terrace32", [t32], 8, 256, [80.0], 308, reid_upstream=True)


if __name__ == "__main__":
    main()
