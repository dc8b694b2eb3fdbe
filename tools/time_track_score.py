#!/usr/bin/env python3
"""Times gnn_cca_amd.tracking.TrackScorer on the batch of tools/time_tracking.py: 64 frames of 4 cameras x 8 detections (N = 2048), ids =
the person of every detection, tracks from FrameLinker on the ground-truth clusters of that batch.  Needs an MI355X.

    python tools/time_track_score.py [--frames 64] [--cams 4] [--per 8] [--reid 2048] [--reps 200] [--host-reps 3] [--max-gap 0] [--hide 0]
                                     [--cross-only]

Three forms, timed in alternating rounds in one process (host clock around repetitions that end in a device synchronise), the whole
measurement run twice:
  device   TrackScorer.add_raw on tensors that are already on the GPU (one memset and two launches; the state carries from one repetition
           to the next as it would from batch to batch, so the rehash launches of the growing pair table are in the figure)
  host     ids, cams and node tracks copied back (the copies and their synchronisation included), then the numpy restatement of the rule
           (tests/track_score_oracle.py) on a carried state
  copy     those device-to-host copies and their synchronisation alone: the floor under ANY host implementation
and, for scale, `link`: FrameLinker's own call on the summaries of the same batch.  The two results are compared once (switched and
counts exactly, result() by ==).  Prints one JSON line per run, then result() for max_gap 0, 1 and 3 and for both matchings on the
--hide 0.1 batch: SYNTHETIC data with ground-truth clusters, not a trained model.  Last (--cross-only: nothing else), what motion='velocity'
does to the scores where people cross each other: tests/tracking_motion_oracle.cross_sequence (12 frames, 70 and 25 people walking straight
through a 6 x 6 arena at 0.3 .. 0.6 per frame, position noise 0.05, R = 16, seeds 0 .. 2), one JSON line per setting with the scores
of motion none and velocity for max_step in {0.4, 1.0}, lam in {0, 1} and max_gap in {0, 2} (with max_gap 2 people are hidden with
probability 0.12 per frame, for up to 3 frames)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import track_score_oracle as ts  # noqa: E402
import tracking_motion_oracle as tm  # noqa: E402
from time_tracking import make_batch  # noqa: E402
from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker, TrackScorer, cluster_summaries_raw  # noqa: E402


def on_device(b, a, max_gap, matching="mutual"):
    """The batch's ground-truth clusters summarised and linked on the device -> (summaries, linker, ids, cam, node_track, node_ptr_dev)."""
    dev = torch.device("cuda")
    d = {k: torch.from_numpy(b[k]).to(dev) for k in ("labels", "xw", "yw", "cam", "emb")}
    s = cluster_summaries_raw(d["labels"], b["node_ptr"].tolist(), d["xw"], d["yw"], d["cam"], d["emb"])
    link = FrameLinker(1.0, lam=1.0, max_gap=max_gap, matching=matching)
    ids = torch.from_numpy(np.tile(np.tile(np.arange(a.per), a.cams), a.frames).astype(np.int64)).to(dev)
    return s, link, ids, d["cam"], link(s).node_track, s.node_ptr_dev


def measure(a, b):
    s, link, ids, cam, track, nptr = on_device(b, a, a.max_gap)
    ptr_host = b["node_ptr"].tolist()
    score = TrackScorer(max_ids=1024, max_cams=8)

    def device_once():
        return score.add_raw(ids, cam, track, ptr_host, node_ptr_dev=nptr)

    def copy_once():
        return [t.cpu().numpy() for t in (ids, cam, track)]   # (.cpu() of a device tensor synchronises)

    def host_once(state):
        i, c, t = copy_once()
        return ts.add(state, i, c, t, b["node_ptr"], 1024, 8)

    # one comparison of the two results, over two batches so that the carried state is used
    state = ts.new_state()
    sw_dev = [device_once().switched for _ in range(2)]
    sw_host = [host_once(state) for _ in range(2)]
    torch.cuda.synchronize()
    same = all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(sw_dev, sw_host)) and score.counts.cpu().tolist() == ts.counts(state)
    same = same and score.result() == ts.result(state)
    for _ in range(10):   # warm-up: code objects, allocator
        device_once()
        link(s)
    torch.cuda.synchronize()
    dev_ms, host_ms, copy_ms, link_ms = [], [], [], []
    for _ in range(a.rounds):
        score.reset()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            device_once()
        torch.cuda.synchronize()
        dev_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            link(s)
        torch.cuda.synchronize()
        link_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            copy_once()
        copy_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        state = ts.new_state()
        t0 = time.perf_counter()
        for _ in range(a.host_reps):
            host_once(state)
        host_ms.append((time.perf_counter() - t0) / a.host_reps * 1e3)
    torch.cuda.synchronize()
    res = score.result()
    return {"frames": a.frames, "cams": a.cams, "per_cam": a.per, "n_nodes": b["n"], "reps": a.reps, "host_reps": a.host_reps,
            "device_ms": [round(v, 4) for v in dev_ms], "link_ms": [round(v, 4) for v in link_ms], "host_ms": [round(v, 2) for v in host_ms],
            "copy_ms": [round(v, 4) for v in copy_ms], "results_equal": bool(same), "max_gap": a.max_gap, "hide": a.hide,
            "cap_after_a_round": score.cap, "detections_after_a_round": res["detections"], "IDSW_after_a_round": res["IDSW"]}


def crossing_scores():
    """TrackScorer's result for both motions on the crossing walks: one line per (persons, max_step, lam, max_gap, seed)."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for persons in (70, 25):
        for max_step in (0.4, 1.0):
            for lam in (0.0, 1.0):
                for gap in (0, 2):
                    for seed in range(3):
                        summ = tm.cross_sequence(np.random.default_rng(seed), 12, persons, 16, speed=(0.3, 0.6), noise=0.05,
                                                 p_hide=0.12 if gap else 0.0, max_hide=gap + 1, arena=6.0)
                        n, ptr = len(summ["rank"]), summ["node_ptr"]
                        ones = t(np.ones(n, np.int32))
                        s = ClusterSummaries(t(summ["count"]), t(summ["rank"]), ones, ones, t(summ["pos"]), t(summ["emb"]), ptr.tolist(),
                                             t(ptr.astype(np.int32)))
                        ids, cam = t(summ["person"]), t(np.zeros(n, np.int32))
                        line = dict(persons=persons, max_step=max_step, lam=lam, max_gap=gap, seed=seed, synthetic=True)
                        for motion in ("none", "velocity"):
                            track = FrameLinker(max_step, lam=lam, max_gap=gap, motion=motion)(s).node_track
                            score = TrackScorer(max_ids=1024, max_cams=8)
                            score.add_raw(ids, cam, track, ptr.tolist(), node_ptr_dev=s.node_ptr_dev)
                            res = score.result()
                            line[motion] = {k: (round(res[k], 4) if isinstance(res[k], float) else res[k])
                                            for k in ("IDSW", "IDF1", "AssA", "tracks", "tracks_per_id")}
                        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--per", type=int, default=8)
    ap.add_argument("--reid", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-gap", type=int, default=0)
    ap.add_argument("--hide", type=float, default=0.0)
    ap.add_argument("--cross-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_track_score.py measures on the GPU; no device is visible")
    if a.cross_only:
        return crossing_scores()
    b = make_batch(a.frames, a.cams, a.per, a.reid, hide=a.hide)
    for run in range(2):
        print(json.dumps(dict(measure(a, b), run=run)), flush=True)
    hidden = make_batch(a.frames, a.cams, a.per, a.reid, hide=0.1)
    for gap in (0, 1, 3):   # what max_gap and the matching do to the scores: synthetic walks, ground-truth clusters
        for matching in ("mutual", "optimal"):
            _, _, ids, cam, track, nptr = on_device(hidden, a, gap, matching)
            score = TrackScorer(max_ids=1024, max_cams=8)
            score.add_raw(ids, cam, track, hidden["node_ptr"].tolist(), node_ptr_dev=nptr)
            print(json.dumps(dict(score.result(), max_gap=gap, matching=matching, hide=0.1, synthetic=True)), flush=True)
    crossing_scores()


if __name__ == "__main__":
    main()
