#!/usr/bin/env python3
"""Times gnn_cca_amd.reentry.TrackGallery behind a FrameLinker on the --hide batch of tools/time_tracking.py (64 frames of 4 cameras x 8
detections, N = 2048, R = 2048; a hidden person's detections stay in the batch as far-away strangers, so every frame has births) with
occlusions longer than max_gap, and prints what the gallery does to TrackScorer's scores.  Needs an MI355X.

    python tools/time_reentry.py [--frames 64] [--reid 2048] [--max-gap 1] [--hide 0.3] [--reps 50] [--host-reps 2] [--rounds 3]
                                 [--window 1024] [--parent-tree DIR]

Call times, not kernel times: the host clock around work that ends in a device synchronise, in alternating rounds in one process.
  gallery  TrackGallery's call alone (six launches) on summaries and tracks that are already on the GPU; the linker's call for the same
           batch runs before the clock starts, and both states carry from one repetition to the next, as from batch to batch
  host     count, rank, pos, emb and the linker's cluster_track / matched_prev / matched_gap copied back (the copies and their
           synchronisation included), then the numpy restatement of the rule (tests/reentry_oracle.py)
  copy     those device-to-host copies alone: the floor under ANY host implementation
The two results are compared once, from a fresh state (identities exactly).
Scores: the three look-alike sequences of tests/test_gpu_reentry.py (synthetic walks with GROUND-TRUTH clusters, not a trained model),
linked and scored on the device, TrackScorer's IDSW / IDF1 / tracks with node_track and with the gallery's node_identity.
--parent-tree DIR: a built checkout of the parent commit.  FrameLinker's call alone is then timed in fresh child processes, the parent's
tree and this one alternating, two runs of --rounds rounds each: linking is untouched if this tree's rounds lie within the parent's own
spread (its slowest minus its fastest round over its two runs).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tree(argv):
    return os.path.abspath(argv[argv.index("--tree") + 1]) if "--tree" in argv else ROOT


TREE = _tree(sys.argv)   # a child timing the linker alone imports the package and the batch of the tree it is given
sys.path.insert(0, os.path.join(TREE, "tests"))
sys.path.insert(0, os.path.join(TREE, "tools"))
import time_tracking  # noqa: E402  (puts its own tree's root in front of sys.path)
import torch  # noqa: E402
from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker, TrackScorer, cluster_summaries_raw  # noqa: E402


def device_summaries(a):
    b = time_tracking.make_batch(a.frames, a.cams, a.per, a.reid, hide=a.hide)
    d = {k: torch.from_numpy(b[k]).cuda() for k in ("labels", "xw", "yw", "cam", "emb")}
    return b, cluster_summaries_raw(d["labels"], b["node_ptr"].tolist(), d["xw"], d["yw"], d["cam"], d["emb"])


def linker_only(a):
    """The child: FrameLinker's call alone, state carried from one repetition to the next."""
    _, s = device_summaries(a)
    link = FrameLinker(1.0, lam=1.0, max_gap=a.max_gap)
    for _ in range(10):
        link(s)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            link(s)
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) / a.reps * 1e3, 4))
    print(json.dumps({"link_ms": ms}))


def scores(max_cos):
    import reentry_oracle as ro
    from gnn_cca_amd.reentry import TrackGallery
    out = []
    for seed, persons, g, m, max_hide, p_hide in [(1, 12, 24, 1, 6, 0.15), (3, 30, 24, 0, 5, 0.2), (7, 40, 12, 1, 5, 0.25)]:
        seq = ro.lookalike_sequence(seed, g, persons, max_hide, p_hide)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        s = ClusterSummaries(t(seq["count"]), t(seq["rank"]), t(seq["size"]), t(seq["n_cams"]), t(seq["pos"]), t(seq["emb"]),
                             seq["node_ptr"].tolist(), t(seq["node_ptr"].astype(np.int32)))
        link = FrameLinker(0.8, lam=1.0, max_gap=m)
        tracks = link(s)
        ids = TrackGallery(link, max_cos)(s, tracks)
        person, cam, ptr = t(seq["person"]), t(np.zeros(len(seq["person"]), np.int32)), seq["node_ptr"].tolist()
        res = {}
        for name, node_ids in (("without", tracks.node_track), ("with", ids.node_identity)):
            sc = TrackScorer()
            sc.add_raw(person, cam, node_ids, ptr)
            r = sc.result()
            res[name] = {"IDSW": r["IDSW"], "IDF1": round(r["IDF1"], 4), "tracks": r["tracks"]}
        res.update(persons=persons, frames=g, max_gap=m, reentries=int((ids.reentered_from >= 0).sum().item()))
        out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--cams", type=int, default=4)
    ap.add_argument("--per", type=int, default=8)
    ap.add_argument("--reid", type=int, default=2048)
    ap.add_argument("--max-gap", type=int, default=1)
    ap.add_argument("--hide", type=float, default=0.3)
    ap.add_argument("--max-cos", type=float, default=0.3)
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--linker-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_reentry.py measures on the GPU; no device is visible")
    if a.linker_only:
        return linker_only(a)
    import reentry_oracle as ro
    from gnn_cca_amd.reentry import TrackGallery
    b, s = device_summaries(a)
    n = b["n"]
    link = FrameLinker(1.0, lam=1.0, max_gap=a.max_gap)
    gal = TrackGallery(link, a.max_cos, window=a.window, max_batch=max(n, 2048))
    kw = dict(window=a.window, max_batch=max(n, 2048))
    keys_s, keys_t = ("count", "rank", "pos", "emb"), ("cluster_track", "matched_prev", "matched_gap")

    def copy_once(tracks):
        out = [getattr(s, k).cpu() for k in keys_s] + [getattr(tracks, k).cpu() for k in keys_t]   # (.cpu() of a device tensor synchronises)
        return [x.numpy() for x in out]

    def host_once(tracks, state):
        h = copy_once(tracks)
        summ, tr = dict(zip(keys_s, h[:4])), dict(zip(keys_t, h[4:]))
        return ro.gallery(summ, b["node_ptr"], tr, a.max_gap, a.max_cos, state=state, **kw)

    # one comparison of the two results, from a fresh state
    tracks = link(s)
    ids = gal(s, tracks)
    want, host_state = host_once(tracks, None)
    torch.cuda.synchronize()
    same = all(np.array_equal(getattr(ids, k).cpu().numpy(), want[k]) for k in ("cluster_identity", "node_identity", "reentered_from"))
    births, back = int((tracks.matched_prev < 0).sum().item()), int((ids.reentered_from >= 0).sum().item())
    for _ in range(5):   # warm-up: code objects, allocator
        gal(s, link(s))
    torch.cuda.synchronize()
    gal_ms, host_ms, copy_ms = [], [], []
    for _ in range(a.rounds):
        spent = 0.0
        for _ in range(a.reps):
            tracks = link(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gal(s, tracks)
            torch.cuda.synchronize()
            spent += time.perf_counter() - t0
        gal_ms.append(spent / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            copy_once(tracks)
        copy_ms.append((time.perf_counter() - t0) / a.reps * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.host_reps):
            host_once(tracks, host_state)   # (a later batch of the sequence: the ring is full of ended tracks)
        host_ms.append((time.perf_counter() - t0) / a.host_reps * 1e3)
    out = {"frames": a.frames, "n_nodes": n, "reid_dim": a.reid, "max_gap": a.max_gap, "hide": a.hide, "window": a.window, "reps": a.reps,
           "host_reps": a.host_reps, "births_first_call": births, "reentries_first_call": back, "identities_equal": bool(same),
           "gallery_ms": [round(v, 4) for v in gal_ms], "host_ms": [round(v, 1) for v in host_ms], "copy_ms": [round(v, 4) for v in copy_ms],
           "scores_synthetic_ground_truth_clusters": scores(a.max_cos)}
    if a.parent_tree:
        runs = {"parent": [], "this": []}
        common = [sys.executable, os.path.abspath(__file__), "--linker-only", "--frames", str(a.frames), "--cams", str(a.cams), "--per", str(a.per),
                  "--reid", str(a.reid), "--max-gap", str(a.max_gap), "--hide", str(a.hide), "--reps", str(max(a.reps, 200)), "--rounds", str(a.rounds)]
        for _ in range(2):   # fresh child processes, alternating
            for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                got = subprocess.run(common + ["--tree", tree], check=True, capture_output=True, text=True, timeout=300).stdout
                runs[name].append(json.loads(got.strip().splitlines()[-1])["link_ms"])
        flat = [v for r in runs["parent"] for v in r]
        spread = max(flat) - min(flat)
        mine = [v for r in runs["this"] for v in r]
        out["linker_call_ms"] = runs
        out["parent_spread_ms"] = round(spread, 4)
        out["linker_within_parent_spread"] = bool(min(flat) - spread <= min(mine) and max(mine) <= max(flat) + spread)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
