#!/usr/bin/env python3
"""Times gnn_cca_amd.tracking on a Terrace-shaped batch: cluster summaries plus frame linking for 64 frames of 4 cameras x 8 detections
(N = 2048, every person seen once per camera: 8 clusters of 4 per frame) with R = 2048 appearance columns.  Needs an MI355X.

    python tools/time_tracking.py [--frames 64] [--cams 4] [--per 8] [--reid 2048] [--reps 200] [--host-reps 3] [--max-gap 0] [--hide 0]
                                  [--matching mutual|optimal] [--crowded] [--motion none|velocity|kalman] [--max-nis X] [--drift 0]
                                  [--times drop:P|jitter:S]

Two ways to the same result, timed in alternating rounds in one process (host clock around work that ends in a device synchronise):
  device   cluster summaries (2 launches) + FrameLinker (3 launches) on tensors that are already on the GPU, as a FramePipeline
           result holds them; the state carries from one repetition to the next, as it would from batch to batch
  host     labels, positions, cameras and embeddings copied back (the copies and their synchronisation included), then the numpy
           restatement of the rules (tests/tracking_oracle.py: plain loops for the sums, float64 matching)
and, as the floor under ANY host implementation, `copy`: those device-to-host copies and their synchronisation alone.
The two results are compared once (summaries bit for bit, ids exactly).  Prints one JSON line.
--max-gap M > 0 times FrameLinker(max_gap=M) (M + 4 launches instead of 3; --hide P then hides each person's cluster with probability P per
frame, so that there is something to find again) against the numpy restatement of ITS rule (tests/tracking_gap_oracle.py).
--matching optimal times FrameLinker(matching='optimal') (the gap path, M + 4 launches also at --max-gap 0) against
tests/tracking_assign_oracle.py.  --crowded times, instead of all of the above, the linker's call alone on a crowded synthetic sequence
(12 frames, 120 persons on 10 x 10, the first frame 102 single-node clusters, position only, --max-gap 1 unless given): both matchings in
alternating rounds, each compared with its oracle once.
--motion velocity times FrameLinker(motion='velocity') (three launches whatever --max-gap is, one workgroup walking the frames in order)
against tests/tracking_motion_oracle.py; the ids AND the velocities are compared once per run.  --drift V selects a batch whose people
move: every person walks a straight line at V units per frame in a direction of its own (the default batch only jitters around a point,
so its velocities are noise).
--motion kalman times kalman.KalmanLinker (q = 0.001, r = 0.0025 = the batch's detection noise squared, vel_var = 0.25; --max-nis X adds the
variance gate) against tests/tracking_kalman_oracle.py -- ids, links, the filtered velocity and the five trajectories arrays are compared
once, bit for bit -- and, in the same alternating rounds, FrameLinker(motion='velocity') on the same batch (`velocity_ms`).  It then links
the crossing walks of DESIGN.md section 9 (40 frames, 25 people, noise 0.10, people hiding for up to 2 frames, max_step 0.35, lam 0,
max_gap 2, seeds 0 .. 3) with the velocity linker, the Kalman linker under the same gate, and the Kalman linker with max_nis = 13.8 under
four times the gate, and prints IDSW / IDF1 of each (`walks`; scored by tests/track_score_oracle.py on the device's ids).
--times times the call WITH time stamps (linker(s, times=...), the _timed entries; the adjacent linker then runs the gap path with
M = 0) against tests/tracking_time_oracle.py: drop:P removes every frame but the first with probability P and stamps the survivors with
their indices, jitter:S (S < 0.5) keeps every frame and perturbs its index by uniform +-S.  Every repetition continues the times of the
one before it (the state carries), so a repetition is a batch of a running sequence.  Without --times the call has no time stamps."""
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
import tracking_assign_oracle as ta  # noqa: E402
import track_score_oracle as tso  # noqa: E402
import tracking_gap_oracle as tg  # noqa: E402
import tracking_kalman_oracle as tk  # noqa: E402
import tracking_motion_oracle as tm  # noqa: E402
import tracking_oracle as to  # noqa: E402
import tracking_time_oracle as tt  # noqa: E402
from gnn_cca_amd.kalman import KalmanLinker  # noqa: E402
from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker, cluster_summaries_raw  # noqa: E402


def make_batch(frames, cams, per, reid, seed=0, hide=0.0, drift=0.0):
    rng = np.random.default_rng(seed)
    n_g = cams * per
    n = frames * n_g
    cam = np.tile(np.repeat(np.arange(cams), per), frames).astype(np.int32)
    person = np.tile(np.tile(np.arange(per), cams), frames)
    frame_of = np.repeat(np.arange(frames), n_g)
    walk = rng.uniform(-8, 8, size=(1, per, 2)) + np.cumsum(rng.normal(0, 0.1, size=(frames, per, 2)), axis=0)
    if drift > 0:   # (drawn only when asked for: the default batch keeps its numbers)
        heading = rng.uniform(0, 2 * np.pi, size=per)
        walk = walk + drift * np.arange(frames)[:, None, None] * np.stack([np.cos(heading), np.sin(heading)], -1)[None]
    xw = walk[frame_of, person, 0] + rng.normal(0, 0.05, n)
    yw = walk[frame_of, person, 1] + rng.normal(0, 0.05, n)
    look = rng.standard_normal((per, reid)).astype(np.float32)
    emb = look[person] + 0.1 * rng.standard_normal((n, reid)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    # a person's detections are one cluster; its label is the smallest node id (the person's detection on camera 0)
    labels = (frame_of * n_g + person).astype(np.int32)
    if hide > 0:   # a hidden person: its detections stay in the batch as clusters of their own, far away from everybody
        gone = rng.random((frames, per)) < hide
        gone[0] = False
        out = gone[frame_of, person]
        labels[out] = np.arange(n, dtype=np.int32)[out]
        xw[out] += 1000.0 + 50.0 * np.arange(n)[out]
    node_ptr = (np.arange(frames + 1) * n_g).astype(np.int64)
    return dict(labels=labels, node_ptr=node_ptr, xw=xw, yw=yw, cam=cam, emb=emb.astype(np.float32), n=n)


def stamp(b, spec, n_g, seed=1):
    """--times: -> (the batch, without its dropped frames; the time of every remaining frame, float64).  Labels point inside a node's own
    frame, so they move with their frame."""
    kind, _, value = spec.partition(":")
    try:
        value = float(value)
    except ValueError:
        value = -1.0
    frames = len(b["node_ptr"]) - 1
    rng = np.random.default_rng(seed)
    if kind == "jitter" and 0 <= value < 0.5:
        return b, np.arange(frames, dtype=np.float64) + rng.uniform(-value, value, size=frames)
    if kind != "drop" or not 0 <= value < 1:
        raise SystemExit("--times takes drop:P with 0 <= P < 1 or jitter:S with 0 <= S < 0.5")
    keep = rng.random(frames) >= value
    keep[0] = True
    rows = np.flatnonzero(np.repeat(keep, n_g))
    new_row = np.full(b["n"], -1, np.int64)
    new_row[rows] = np.arange(len(rows))
    out = {k: b[k][rows] for k in ("xw", "yw", "cam", "emb")}
    out["labels"] = new_row[b["labels"][rows]].astype(np.int32)
    out["node_ptr"] = (np.arange(int(keep.sum()) + 1) * n_g).astype(np.int64)
    out["n"] = len(rows)
    return out, np.flatnonzero(keep).astype(np.float64)


KALMAN = dict(q=0.001, r=0.0025, vel_var=0.25)   # --motion kalman on the Terrace-shaped batch (detection noise 0.05)


def crossing_walks():
    """IDSW / IDF1 on the crossing walks of DESIGN.md section 9, linked on the device: velocity, Kalman under the same gate, Kalman with the
    variance gate under four times the distance gate."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rows = []
    for seed in range(4):
        summ = tm.cross_sequence(np.random.default_rng(seed), 40, 25, 8, noise=0.10, p_hide=0.1, max_hide=2)
        n = len(summ["rank"])
        ones = t(np.ones(n, np.int32))
        s = ClusterSummaries(t(summ["count"]), t(summ["rank"]), ones, ones, t(summ["pos"]), t(summ["emb"]), summ["node_ptr"].tolist(),
                             t(summ["node_ptr"].astype(np.int32)))
        links = {"velocity": FrameLinker(0.35, lam=0.0, max_gap=2, motion="velocity"),
                 "kalman": KalmanLinker(0.35, 0.001, 0.01, 0.25, lam=0.0, max_gap=2),
                 "kalman_nis": KalmanLinker(1.4, 0.001, 0.01, 0.25, lam=0.0, max_gap=2, max_nis=13.8)}
        row = {"seed": seed}
        for name, link in links.items():
            ids = link(s).node_track.cpu().numpy()
            res = tso.score(summ["person"], np.zeros(n, np.int32), ids, summ["node_ptr"], 1024, 8)[2]
            row[name] = {"IDSW": res["IDSW"], "IDF1": round(res["IDF1"], 4)}
        rows.append(row)
    return rows


def crowded(a):
    """The linker's call alone on the crowded sequence, both matchings."""
    m = a.max_gap if a.max_gap > 0 else 1
    summ = tg.hide_sequence(np.random.default_rng(7), 12, 120, 8, arena=10.0, max_hide=1, noise=0.3, max_alive=120)
    n = len(summ["rank"])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ones = t(np.ones(n, np.int32))
    s = ClusterSummaries(t(summ["count"]), t(summ["rank"]), ones, ones, t(summ["pos"]), t(summ["emb"]), summ["node_ptr"].tolist(),
                         t(summ["node_ptr"].astype(np.int32)))
    links = {k: FrameLinker(0.8, lam=0.0, max_gap=m, matching=k) for k in ("mutual", "optimal")}
    out = {"crowded": True, "clusters_per_frame": summ["count"].tolist(), "max_gap": m, "reps": a.reps}
    for k, link in links.items():
        want, _ = ta.link_gap(summ, summ["node_ptr"], 0.8, 0.0, None, m, matching=k)
        got = link(s)
        out[k + "_ids_equal"] = bool(all(np.array_equal(getattr(got, f).cpu().numpy(), want[f])
                                         for f in ("cluster_track", "node_track", "matched_prev", "matched_gap")))
        out[k + "_tracks"] = int(got.next_id.item())
        out[k + "_ms"] = []
        for _ in range(10):
            link.reset()
            link(s)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, link in links.items():
            t0 = time.perf_counter()
            for _ in range(a.reps):
                link.reset()   # (every call links the whole sequence from nothing: the same work each time)
                link(s)
            torch.cuda.synchronize()
            out[k + "_ms"].append(round((time.perf_counter() - t0) / a.reps * 1e3, 4))
    print(json.dumps(out))


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
    ap.add_argument("--matching", choices=("mutual", "optimal"), default="mutual")
    ap.add_argument("--crowded", action="store_true")
    ap.add_argument("--motion", choices=("none", "velocity", "kalman"), default="none")
    ap.add_argument("--max-nis", type=float, default=None)
    ap.add_argument("--drift", type=float, default=0.0)
    ap.add_argument("--times", default=None, metavar="drop:P|jitter:S")
    a = ap.parse_args()
    if a.times and a.crowded:
        raise SystemExit("--times goes with the Terrace-shaped batch")
    if a.motion != "none" and (a.matching == "optimal" or a.crowded):
        raise SystemExit(f"--motion {a.motion} goes with --matching mutual on the Terrace-shaped batch")
    if a.max_nis is not None and a.motion != "kalman":
        raise SystemExit("--max-nis goes with --motion kalman")
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_tracking.py measures on the GPU; no device is visible")
    if a.crowded:
        return crowded(a)
    b = make_batch(a.frames, a.cams, a.per, a.reid, hide=a.hide, drift=a.drift)
    times = None
    if a.times:
        b, times = stamp(b, a.times, a.cams * a.per)
    calls = [0, 0]   # timed: every call continues the times of the one before it, a.frames periods later
    dev = torch.device("cuda")
    d = {k: torch.from_numpy(b[k]).to(dev) for k in ("labels", "xw", "yw", "cam", "emb")}
    ptr_host = b["node_ptr"].tolist()
    max_step, lam = 1.0, 1.0
    kalman = a.motion == "kalman"
    if kalman:
        link = KalmanLinker(max_step, KALMAN["q"], KALMAN["r"], KALMAN["vel_var"], lam=lam, max_gap=a.max_gap, max_nis=a.max_nis)
        beside = FrameLinker(max_step, lam=lam, max_gap=a.max_gap, motion="velocity")   # timed in the same rounds
    else:
        link = FrameLinker(max_step, lam=lam, max_gap=a.max_gap, matching=a.matching, motion=a.motion)

    def device_once():
        s = cluster_summaries_raw(d["labels"], ptr_host, d["xw"], d["yw"], d["cam"], d["emb"])
        if times is None:
            return s, link(s)
        calls[0] += 1
        return s, link(s, times=times + float((calls[0] - 1) * a.frames))

    def beside_once():
        s = cluster_summaries_raw(d["labels"], ptr_host, d["xw"], d["yw"], d["cam"], d["emb"])
        if times is None:
            return beside(s)
        calls[1] += 1   # (a running sequence of its own)
        return beside(s, times=times + float((calls[1] - 1) * a.frames))

    def copy_once():
        out = [d[k].cpu() for k in ("labels", "xw", "yw", "cam", "emb")]   # (.cpu() of a device tensor synchronises)
        return [t.numpy() for t in out]

    def host_once(state):
        labels, xw, yw, cam, emb = copy_once()
        s = to.summaries(labels, b["node_ptr"], xw, yw, cam, emb)
        if kalman:
            return s, tk.link_kalman(s, b["node_ptr"], max_step, lam=lam, max_cos=None, max_gap=a.max_gap, max_nis=a.max_nis, times=times,
                                     state=state, **KALMAN)
        if times is not None:
            return s, tt.link_timed(s, b["node_ptr"], times, max_step, lam, None, a.max_gap, state, matching=a.matching,
                                    motion=a.motion == "velocity")
        if a.motion == "velocity":
            return s, tm.link_motion(s, b["node_ptr"], max_step, lam, None, a.max_gap, state)
        if a.matching == "optimal":
            return s, ta.link_gap(s, b["node_ptr"], max_step, lam, None, a.max_gap, state, matching="optimal")
        if a.max_gap > 0:
            return s, tg.link_gap(s, b["node_ptr"], max_step, lam, None, a.max_gap, state)
        return s, to.link(s, b["node_ptr"], max_step, lam, None, state)

    # one comparison of the two results, from a fresh state
    s_dev, t_dev = device_once()
    s_host, (t_host, _) = host_once(None)
    torch.cuda.synchronize()
    same = all(np.array_equal(getattr(s_dev, k).cpu().numpy(), s_host[k]) for k in ("count", "rank", "size", "n_cams", "pos", "emb"))
    same_ids = all(np.array_equal(getattr(t_dev, k).cpu().numpy(), t_host[k]) for k in ("cluster_track", "node_track", "matched_prev"))
    gaps = t_dev.matched_gap.cpu().numpy()
    if a.max_gap > 0 or a.matching == "optimal" or a.motion != "none" or times is not None:
        same_ids = same_ids and np.array_equal(gaps, t_host["matched_gap"])
    if a.motion != "none":
        same_ids = same_ids and np.array_equal(t_dev.velocity.cpu().numpy(), t_host["velocity"])
    if kalman:   # the five trajectories arrays, bit for bit
        same_ids = same_ids and all(np.array_equal(getattr(t_dev.trajectories, k).cpu().numpy().view(np.uint8), t_host[k].view(np.uint8))
                                    for k in ("pos", "vel", "cov", "nis", "age"))
    for _ in range(10):   # warm-up: code objects, allocator
        device_once()
        if kalman:
            beside_once()
    torch.cuda.synchronize()
    dev_ms, host_ms, copy_ms, beside_ms = [], [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            device_once()
        torch.cuda.synchronize()
        dev_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        if kalman:
            t0 = time.perf_counter()
            for _ in range(a.reps):
                beside_once()
            torch.cuda.synchronize()
            beside_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            copy_once()
        copy_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.host_reps):
            host_once(None)
        host_ms.append((time.perf_counter() - t0) / a.host_reps * 1e3)
    more = {}
    if kalman:
        more = {"velocity_ms": [round(v, 4) for v in beside_ms], "max_nis": a.max_nis, "kalman": KALMAN,
                "median_ratio_kalman_over_velocity": round(float(np.median(dev_ms) / np.median(beside_ms)), 3), "walks": crossing_walks()}
    print(json.dumps({**more, "frames": a.frames, "cams": a.cams, "per_cam": a.per, "n_nodes": b["n"], "reid_dim": a.reid, "reps": a.reps,
                      "host_reps": a.host_reps, "device_ms": [round(v, 4) for v in dev_ms], "host_ms": [round(v, 2) for v in host_ms],
                      "copy_ms": [round(v, 4) for v in copy_ms], "summaries_equal": bool(same), "ids_equal": bool(same_ids),
                      "tracks": int(t_dev.next_id.item()), "max_gap": a.max_gap, "hide": a.hide, "matching": a.matching, "motion": a.motion, "drift": a.drift,
                      "times": a.times, "frames_kept": len(b["node_ptr"]) - 1,
                      "matches_per_gap": [int((gaps == k).sum()) for k in range(a.max_gap + 1)]}))


if __name__ == "__main__":
    main()
