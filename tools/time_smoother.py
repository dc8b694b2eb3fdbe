#!/usr/bin/env python3
"""Times gnn_cca_amd.smoothing.TrackSmoother behind a FrameLinker on the batch of tools/time_tracking.py (64 frames of 4 cameras x 8
detections, N = 2048, R = 2048) and prints what the filter does to position and velocity error.  Needs an MI355X.

    python tools/time_smoother.py [--frames 64] [--reid 2048] [--max-gap 0] [--hide 0] [--drift 0] [--reps 200] [--host-reps 3] [--rounds 3]

Call times, not kernel times: the host clock around --reps calls that end in ONE device synchronise, in alternating rounds in one process
(the method of tools/time_tracking.py); summaries and tracks are already on the GPU and the states carry from one repetition to the next,
as from batch to batch.
  link      FrameLinker's call alone
  smooth    TrackSmoother's call alone (three launches) on the Tracks of the linker's latest call
  host      count, size, pos and the linker's matched_prev / matched_gap copied back (the copies and their synchronisation included), then
            the numpy restatement of the rule (tests/track_smooth_oracle.py)
  copy      those device-to-host copies alone: the floor under ANY host implementation
The two results are compared once, from a fresh state (all five outputs exactly).
Scores: synthetic crossing walks (tests/tracking_motion_oracle.py cross_sequence: straight lines at 0.3 .. 0.6 per frame, position noise
0.05 per coordinate, GROUND-TRUTH clusters, not a trained model), linked and filtered on the device.  Over the rows of age >= 3: the RMSE
of the raw and of the filtered position against the noise-free position, and of the one-step velocity (the displacement since the
predecessor over the frames gone by -- what Tracks.velocity is) and of the filtered velocity against the noise-free displacement.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time_tracking  # noqa: E402  (puts the root in front of sys.path)
import torch  # noqa: E402
import track_smooth_oracle as so  # noqa: E402
import tracking_motion_oracle as tm  # noqa: E402
from gnn_cca_amd.smoothing import TrackSmoother  # noqa: E402
from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker, cluster_summaries_raw  # noqa: E402

KEYS = ("pos", "vel", "cov", "nis", "age")


def scores(q, r, vel_var):
    out = []
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for seed in (11, 12, 13):
        kw = dict(g=24, persons=10, r=16, speed=(0.3, 0.6), p_hide=0.1, max_hide=1, arena=8.0)
        noisy = tm.cross_sequence(np.random.default_rng(seed), noise=0.05, **kw)
        clean = tm.cross_sequence(np.random.default_rng(seed), noise=0.0, **kw)   # the same draws: the same walks, rows and order
        assert np.array_equal(noisy["person"], clean["person"])
        ptr = noisy["node_ptr"]
        s = ClusterSummaries(t(noisy["count"]), t(noisy["rank"]), t(noisy["size"]), t(noisy["n_cams"]), t(noisy["pos"]), t(noisy["emb"]), ptr.tolist(),
                             t(ptr.astype(np.int32)))
        link = FrameLinker(0.8, lam=1.0, max_gap=1)
        tracks = link(s)
        tr = TrackSmoother(link, q, r, vel_var)(s, tracks)
        prev, gap, age = tracks.matched_prev.cpu().numpy(), tracks.matched_gap.cpu().numpy(), tr.age.cpu().numpy()
        frame = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        linked = gap >= 0
        pred = np.where(linked, ptr[np.maximum(frame - 1 - gap, 0)] + prev, 0)
        dt = (gap + 1).astype(np.float64)[:, None]
        raw_vel, true_vel = (noisy["pos"] - noisy["pos"][pred]) / dt, (clean["pos"] - clean["pos"][pred]) / dt
        old = age >= 3
        rmse = lambda a, b: round(float(np.sqrt(((a[old] - b[old]) ** 2).sum(axis=1).mean())), 4)
        out.append({"seed": seed, "rows_age_ge_3": int(old.sum()), "same_person_links": int((noisy["person"][pred] == noisy["person"])[linked].sum()),
                    "links": int(linked.sum()), "pos_rmse_raw": rmse(noisy["pos"], clean["pos"]), "pos_rmse_filtered": rmse(tr.pos.cpu().numpy(), clean["pos"]),
                    "vel_rmse_one_step": rmse(raw_vel, true_vel), "vel_rmse_filtered": rmse(tr.vel.cpu().numpy(), true_vel)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--per", type=int, default=8)
    ap.add_argument("--reid", type=int, default=2048)
    ap.add_argument("--max-gap", type=int, default=0)
    ap.add_argument("--hide", type=float, default=0.0)
    ap.add_argument("--drift", type=float, default=0.0)
    ap.add_argument("--q", type=float, default=1e-4)
    ap.add_argument("--r", type=float, default=0.0025)
    ap.add_argument("--vel-var", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_smoother.py measures on the GPU; no device is visible")
    b = time_tracking.make_batch(a.frames, a.cams, a.per, a.reid, hide=a.hide, drift=a.drift)
    d = {k: torch.from_numpy(b[k]).cuda() for k in ("labels", "xw", "yw", "cam", "emb")}
    s = cluster_summaries_raw(d["labels"], b["node_ptr"].tolist(), d["xw"], d["yw"], d["cam"], d["emb"])
    link = FrameLinker(1.0, lam=1.0, max_gap=a.max_gap)
    sm = TrackSmoother(link, a.q, a.r, a.vel_var)
    keys_s, keys_t = ("count", "size", "pos"), ("matched_prev", "matched_gap")

    def copy_once(tracks):
        out = [getattr(s, k).cpu() for k in keys_s] + [getattr(tracks, k).cpu() for k in keys_t]   # (.cpu() of a device tensor synchronises)
        return [x.numpy() for x in out]

    def host_once(tracks, state):
        h = copy_once(tracks)
        return so.smooth(dict(zip(keys_s, h[:3])), b["node_ptr"], dict(zip(keys_t, h[3:])), a.q, a.r, a.vel_var, max_gap=a.max_gap, state=state)

    # one comparison of the two results, from a fresh state
    tracks = link(s)
    tr = sm(s, tracks)
    want, host_state = host_once(tracks, None)
    torch.cuda.synchronize()
    same = all(np.array_equal(getattr(tr, k).cpu().numpy(), want[k]) for k in KEYS)
    age = tr.age.cpu().numpy()
    for _ in range(10):   # warm-up: code objects, allocator
        tracks = link(s)
        sm(s, tracks)
    torch.cuda.synchronize()
    link_ms, smooth_ms, both_ms, host_ms, copy_ms = [], [], [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            tracks = link(s)
        torch.cuda.synchronize()
        link_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            sm(s, tracks)   # (the links of a batch that continues the carried frames: the same chains every repetition)
        torch.cuda.synchronize()
        smooth_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            sm(s, link(s))
        torch.cuda.synchronize()
        both_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            copy_once(tracks)
        copy_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.host_reps):
            host_once(tracks, host_state)   # (a later batch of the sequence: every chain starts in the carried frames)
        host_ms.append((time.perf_counter() - t0) / a.host_reps * 1e3)
    print(json.dumps({"frames": a.frames, "n_nodes": b["n"], "reid_dim": a.reid, "max_gap": a.max_gap, "hide": a.hide, "drift": a.drift, "reps": a.reps,
                      "host_reps": a.host_reps, "clusters_first_call": int((age >= 0).sum()), "longest_chain_first_call": int(age.max()) + 1,
                      "outputs_equal": bool(same), "link_ms": [round(v, 4) for v in link_ms], "smooth_ms": [round(v, 4) for v in smooth_ms],
                      "link_then_smooth_ms": [round(v, 4) for v in both_ms], "host_ms": [round(v, 2) for v in host_ms],
                      "copy_ms": [round(v, 4) for v in copy_ms], "q": a.q, "r": a.r, "vel_var": a.vel_var,
                      "scores_synthetic_ground_truth_clusters": scores(a.q, a.r, a.vel_var)}))


if __name__ == "__main__":
    main()
