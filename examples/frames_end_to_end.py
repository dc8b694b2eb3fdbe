#!/usr/bin/env python3
"""End-to-end walk through the reference's per-batch inference flow (inference.py:173-345) on synthetic frames, with
every GPU-side step taken by this repository: graph construction + edge attributes (row N1), the MPN forward (the hot
path), threshold / pruning / identity clusters (row N2), and the per-frame scores of inference.py:349-371 aggregated as main.py:335-348
does (gnn_cca_amd.evaluation), next to the baseline the GNN has to beat: rank-1 ReID links with and without k-reciprocal re-ranking
(MODE eval_RANK, gnn_cca_amd.rerank), same batch, same scorer.  Needs an MI355X.

    python examples/frames_end_to_end.py [frames] [cams] [detections_per_cam] [--top-k K] [--rank-by ground|reid] [--symmetric union|mutual]
                                         [--radius R] [--radius-unit ground|max_dist]

--top-k K keeps every detection's K nearest cross-camera candidates (build_graph_batch(top_k=K); the graph is then directed and the
pruning keeps mutual pairs only); the same batch also goes through the one-call form, FramePipeline(model, top_k=K).
--symmetric union|mutual (with --top-k) closes that list under reversal: an edge is kept if either / both of its endpoints selected the
other.  The build then waits once for its edge count, and the pipeline takes its step-by-step path.  With --top-k the scores are also
printed against the dense truth (evaluate_frames(against='dense'): every dropped edge counts as predicted 0).
--radius R keeps a cross-camera pair only if the two detections are within R on the ground plane (build_graph_batch(radius=R); in the
units of the positions, or of max_dist with --radius-unit max_dist).  The list is closed under reversal and its size is known on the host,
so the pipeline keeps its one-call form; the scores are printed against the dense truth as well.  Not together with --top-k.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (model / GRAPH_NET_PARAMS builders)
from gnn_cca_amd.calibration import SweepAccumulator  # noqa: E402
from gnn_cca_amd.evaluation import EvalAccumulator, evaluate_frames  # noqa: E402
from gnn_cca_amd.graph_build import build_graph_batch  # noqa: E402
from gnn_cca_amd.pipeline import FramePipeline  # noqa: E402
from gnn_cca_amd.postprocess import prune_and_cluster, threshold  # noqa: E402
from gnn_cca_amd.rerank import MAX_FRAME_NODES as RERANK_MAX_FRAME_NODES, rank_baseline  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("frames", nargs="?", type=int, default=8)
    ap.add_argument("cams", nargs="?", type=int, default=4)
    ap.add_argument("per", nargs="?", type=int, default=8, metavar="detections_per_cam")
    ap.add_argument("--top-k", type=int, default=None, metavar="K", help="keep each detection's K nearest cross-camera candidates (default: all)")
    ap.add_argument("--rank-by", choices=("ground", "reid"), default="ground", help="what 'nearest' means for --top-k")
    ap.add_argument("--symmetric", choices=("union", "mutual"), default=None,
                    help="close the --top-k list under reversal: keep an edge if either (union) / both (mutual) endpoints selected the other")
    ap.add_argument("--radius", type=float, default=None, metavar="R", help="keep a cross-camera pair only within R on the ground plane (default: all)")
    ap.add_argument("--radius-unit", choices=("ground", "max_dist"), default="ground", help="R in the units of the positions, or of each frame's max_dist")
    a = ap.parse_args()
    if a.symmetric and not a.top_k:
        ap.error("--symmetric needs --top-k")
    if a.radius is not None and a.top_k:
        ap.error("--radius and --top-k exclude each other")
    frames, cams, per = a.frames, a.cams, a.per
    cap = dict(top_k=a.top_k, rank_by=a.rank_by, symmetric=a.symmetric, radius=a.radius, radius_unit=a.radius_unit)
    pruned_graph = bool(a.top_k) or a.radius is not None
    rng = np.random.default_rng(0)
    n_g = cams * per
    n = frames * n_g
    # what libs/datasets.py would hand over per frame: detections with camera id, person id, ground-plane position
    id_cam = np.tile(np.repeat(np.arange(cams), per), frames)
    ids = np.concatenate([rng.integers(0, per, size=n_g) for _ in range(frames)]).astype(np.int64)
    pos = rng.uniform(-8, 8, size=(frames, per, 2))
    frame_of = np.repeat(np.arange(frames), n_g)
    xw = pos[frame_of, ids, 0] + rng.normal(0, 0.3, n)
    yw = pos[frame_of, ids, 1] + rng.normal(0, 0.3, n)
    max_dist = [80.0] * frames                       # CONFIG['CONV_TO_M'][dataset]
    node_embeds = torch.randn(n, 2048, device="cuda")  # ReID CNN outputs (inference.py:183), random here
    reid_embeds = torch.randn(n, 256, device="cuda")
    model = bench.build_model(bench.graph_net_params(), n_g).cuda().eval()

    def run():
        batch = build_graph_batch(xw, yw, ids, id_cam, [n_g] * frames, max_dist, node_embeds, reid_embeds, **cap)
        with torch.no_grad():
            out = model(batch)
        probs, preds = threshold(out["classified_edges"][-1])
        post = prune_and_cluster(batch.edge_index, preds, n, batch.node_ptr_dev, batch.edge_ptr_dev)
        return batch, probs, post

    # random weights put every logit on one side of 0; centre them so that the pruning / clustering steps have work
    with torch.no_grad():
        batch, _, _ = run()
        sd = model.state_dict()
        last_bias = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[last_bias] -= model(batch)["classified_edges"][-1].median()
        model.load_state_dict(sd)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        batch, probs, post = run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    e = batch.edge_index.shape[1]
    print(f"{frames} frames x {cams} cameras x {per} detections: N={n} E={e}" + (f" (top_k={a.top_k} by {a.rank_by}" + (f", {a.symmetric}" if a.symmetric else "") + ")" if a.top_k else "")
          + (f" (radius={a.radius} {a.radius_unit})" if a.radius is not None else ""))
    print(f"graph build + MPN (L=4) + threshold/prune/cluster: {dt * 1e3:.3f} ms per batch "
          f"({e / dt / 1e6:.1f} M edges/s end to end, host planning included)")
    print(f"active edges after pruning: {int(post['pruned'].sum())}, identity clusters: {int(post['n_clusters'].item())}, "
          f"max out-flow per node: {int(post['flow_out'].max())}")
    # the same batch in ONE native call (gnn_cca_amd.pipeline): bit for bit the steps above
    pipe = FramePipeline(model, **cap)
    r = pipe(xw, yw, ids, id_cam, [n_g] * frames, max_dist, node_embeds, reid_embeds)
    same = torch.equal(r.pruned, post["pruned"]) and torch.equal(r.labels, post["labels"])
    print(f"FramePipeline, {'one call' if r._d2h is not None else 'step by step'}: identity clusters {int(r.n_clusters.item())}, equal to the step-by-step result: {same}")
    # PRUNING: False (config_inference.yaml:7): nothing is pruned, the clusters are the strongly connected components of the active edges
    u = FramePipeline(model, pruning=False, splitting=False, **cap)(xw, yw, ids, id_cam, [n_g] * frames, max_dist, node_embeds, reid_embeds)
    print(f"FramePipeline(pruning=False, splitting=False): active edges {int(u.pruned.sum())}, identity clusters {int(u.n_clusters.item())} "
          f"(strongly connected components), {int(u.final()['n_clusters'].item())} after ROUNDING")
    # per-frame metrics against the ground truth the graph build wrote (batch.edge_labels: same person id), then main.py's aggregates
    acc = EvalAccumulator().add(evaluate_frames(batch, post["pruned"], post["labels"]))
    print("aggregates over the frames:", ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in acc.result().items()))
    if pruned_graph:   # a capped or gated graph: the same predictions scored as the dense graph would have been, dropped edges predicted 0
        acc = EvalAccumulator().add(evaluate_frames(batch, post["pruned"], post["labels"], against="dense"))
        print("against the dense truth:   ", ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in acc.result().items()))
    # which threshold?  every operating point of the batch in one pass (gnn_cca_amd.calibration), the best one applied
    ths = np.arange(0.05, 1.0, 0.05)
    sweep = SweepAccumulator(ths).add(r.sweep(ths))                      # float64 [T, G, 16] on the device; add() does not wait
    best = sweep.best("F_micro")                                         # every threshold of maximal F over the whole batch
    th = float(sweep.thresholds[best[0]])
    tuned = FramePipeline(model, threshold=th, **cap)(xw, yw, ids, id_cam, [n_g] * frames, max_dist, node_embeds, reid_embeds)
    at = EvalAccumulator().add(tuned.evaluate(final=False)).result()
    print(f"threshold sweep: F_micro is maximal ({sweep.result()['F_micro'][best[0]]:.4g}) at {sweep.thresholds[best].round(2).tolist()}; "
          f"FramePipeline(threshold={th:.2f}): TP {at['TP']} FP {at['FP']} FN {at['FN']}, F per frame {at['F']:.4g}")
    # the baseline the GNN has to beat (MODE eval_RANK with RERANK): rank-1 ReID links after k-reciprocal re-ranking, same batch, same scorer
    if n_g <= RERANK_MAX_FRAME_NODES:
        for name, kw in (("rank-1 + re-ranking", dict(rank=1)), ("rank-1, plain distances", dict(rank=1, rerank=False))):
            base = EvalAccumulator().add(rank_baseline(batch, **kw)).result()
            print(f"{name}: " + ", ".join(f"{k} {base[k]:.4g}" for k in ("RI", "MI", "hom", "com", "v")))
        gnn = acc.result() if not pruned_graph else EvalAccumulator().add(evaluate_frames(batch, post["pruned"], post["labels"])).result()
        print("the GNN on the same frames: " + ", ".join(f"{k} {gnn[k]:.4g}" for k in ("RI", "MI", "hom", "com", "v")))
    print("random weights / random embeddings: the cluster structure and the chosen threshold are meaningless, the plumbing is what is shown")


if __name__ == "__main__":
    main()
