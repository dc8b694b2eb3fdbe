#!/usr/bin/env python3
"""Time FrameResult.exclusive() against FrameResult.final() on the same batches, and say how the three partitions differ; prints ONE
JSON line.  GPU box.

Batches: bench.terrace_frames -- 64 consecutive frames of the Terrace sequence's own topology (4 cameras, ~19 detections and ~343 edges
per frame) with synthetic positions and embeddings -- through FramePipeline with the synthetic model whose last classifier bias is
shifted so that the decisions vary (as the evaluation tests do).  The weights are RANDOM: the quality columns say how the device chain's,
final()'s and exclusive()'s partitions differ on such probabilities, not which of them is right.

Method: the pipeline results of every batch are made first (untimed) and the device is idle; then exclusive() of all batches between two
GPU events (device time, no host wait inside) and under a host clock that ends in one synchronise; then final() of all batches under
the host clock (it waits for the host heuristics by itself).  Both are computed once per result, so every round gets fresh results
(--reps of every batch per window); the sides alternate inside a round; the line carries every round's figure, the median and the
spread (max - min).  final() runs the code path of the parent commit, which this feature does not touch: it is the comparison basis.

    python tools/time_exclusive.py [--batches 16] [--reps 8] [--rounds 7] [--threshold 0.5]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def summary(vals):
    return {"rounds_ms": [round(v, 4) for v in vals], "median_ms": round(float(np.median(vals)), 4),
            "spread_ms": round(float(max(vals) - min(vals)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--reps", type=int, default=8, help="results of every batch per timed window (each is timed once: both calls are cached)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threshold", type=float, default=0.5)
    args = ap.parse_args()
    import torch
    from gnn_cca_amd.evaluation import EvalAccumulator, evaluate_frames
    from gnn_cca_amd.pipeline import FramePipeline
    from gnn_cca_amd.tracking import cluster_summaries

    if not torch.cuda.is_available():
        raise SystemExit("tools/time_exclusive.py measures on the GPU; no device found")
    dev = torch.device("cuda", 0)
    frames = bench.terrace_frames(64, args.batches)
    model = bench.build_model(copy.deepcopy(bench.graph_net_params(L=4)), 20, seed=0).to(dev).eval()
    dev_in = [(torch.from_numpy(f["node"]).to(dev), torch.from_numpy(f["reid"]).to(dev)) for f in frames]

    def run(pipe, i):
        f, (node, reid) = frames[i], dev_in[i]
        return pipe(f["xw"], f["yw"], f["ids"], f["id_cam"], f["sizes"], f["max_dist"], node, reid)

    with torch.no_grad():   # the decision boundary inside the logits
        r = run(FramePipeline(model), 0)
        sd = model.state_dict()
        last_bias = [k for k in sd if k.startswith("classifier.") and k.endswith(".bias")][-1]
        sd[last_bias] -= r.outputs["classified_edges"][-1].median()
        model.load_state_dict(sd)
    pipe = FramePipeline(model, threshold=args.threshold)

    def results(reps=1):
        rs = [run(pipe, i) for _ in range(reps) for i in range(args.batches)]
        torch.cuda.synchronize()
        return rs

    # ---- what the three partitions are ------------------------------------------------------------------------------------------------
    acc = {k: EvalAccumulator() for k in ("chain", "final", "exclusive")}
    clusters = {k: 0 for k in acc}
    repeated = {k: 0 for k in acc}
    bad_frames = {k: 0 for k in acc}
    cut_frames = n_frames = n_finalized = 0
    for r in results():
        fin, ex = r.final(), r.exclusive()
        n_finalized += len(fin["frames_finalized"])
        for k, (pred, lab) in (("chain", (r.pruned, r.labels)), ("final", (fin["predictions"], fin["labels"])),
                               ("exclusive", (ex["predictions"], ex["labels"]))):
            acc[k].add(evaluate_frames(r.batch, pred, lab))
            s = cluster_summaries(r.batch, lab)
            twice = (s.size > s.n_cams).cpu().numpy()
            clusters[k] += int(s.count.sum().item())
            repeated[k] += int(twice.sum())
            ptr = np.asarray(r.batch.node_ptr)
            bad_frames[k] += int(sum(twice[ptr[g]:ptr[g + 1]].any() for g in range(len(ptr) - 1)))
        cut_frames += int((ex["cut"] > 0).sum().item())
        n_frames += len(r.batch.node_ptr) - 1
        if int(ex["flags"].sum().item()):
            raise SystemExit("exclusive() refused a frame of this batch: nothing to time")
    quality = {}
    for k in acc:
        res = acc[k].result()
        quality[k] = {"ARI": round(res["RI"], 4), "F": round(res["F"], 4), "v_measure": round(res["v"], 4), "clusters": clusters[k],
                      "clusters_with_a_repeated_camera": round(repeated[k] / max(clusters[k], 1), 4),
                      "frames_with_a_repeated_camera": round(bad_frames[k] / max(n_frames, 1), 4)}
    quality["exclusive"]["frames_with_cut"] = round(cut_frames / max(n_frames, 1), 4)
    quality["final"]["frames_finalized"] = round(n_finalized / max(n_frames, 1), 4)

    # ---- time ---------------------------------------------------------------------------------------------------------------------------
    def time_exclusive(rs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for r in rs:
            r.exclusive()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / len(rs), (time.perf_counter() - t0) * 1e3 / len(rs)

    def time_final(rs):
        t0 = time.perf_counter()
        for r in rs:
            r.final()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(rs)

    for _ in range(2):   # warm-up: every shape and kernel of the timed windows, the host pool's threads
        time_exclusive(results(args.reps))
        time_final(results(args.reps))
    got = {"exclusive_gpu_events": [], "exclusive_host_clock": [], "final_host_clock": []}
    for _ in range(args.rounds):
        ev, host = time_exclusive(results(args.reps))
        got["exclusive_gpu_events"].append(ev), got["exclusive_host_clock"].append(host)
        got["final_host_clock"].append(time_final(results(args.reps)))
    pipe.close()
    res = {"metric": "ms per 64-frame batch, after the device chain", "batches": args.batches, "frames": n_frames, "threshold": args.threshold,
           "nodes_per_batch": round(float(np.mean([len(f["ids"]) for f in frames])), 1), "rounds": args.rounds,
           "results_per_window": args.reps * args.batches, "model": "synthetic (random weights, shifted bias)"}
    res.update({k: summary(v) for k, v in got.items()})
    res["final_over_exclusive_host_clock"] = round(float(np.median(got["final_host_clock"]) / np.median(got["exclusive_host_clock"])), 2)
    res["quality"] = quality
    print(json.dumps(res))


if __name__ == "__main__":
    main()
