#!/usr/bin/env python3
"""Track ids over time on synthetic frames: FramePipeline results -> per-cluster summaries (fused position, mean appearance, size,
camera count) -> persistent track ids across frames and batches (gnn_cca_amd.tracking).  Everything stays on the GPU until the final
print.  The reference has no counterpart of this stage: it scores single frames (inference.py:349-371).  Needs an MI355X.

    python examples/track_frames.py [batches] [frames_per_batch] [cams] [persons] [--exclusive] [--smooth] [--kalman]

Persons walk on the ground plane; every camera sees every person, with noise on the position.  The model has random weights, so its
clusters mean nothing: the ids are shown for the model's partition AND for the ground-truth partition of the same detections, where a
person keeps one id as long as the walk stays inside max_step.  In the middle frame of every batch person 0 is hidden from every camera:
the linker with max_gap=1 finds them again one frame later under the same id, the linker without max_gap hands out a new one.  Two
more linkers on the true partition show matching='optimal' and motion='velocity' (a cluster is looked for at its last position plus its
last displacement per frame; these persons wander without a heading, so it has little to predict here: DESIGN.md section 9 has people
crossing each other).  Four TrackScorers accumulate, on the device, the identity scores of the four linkers on the true partition
against the person ids.  Last, a DROPPED frame: the same batches without their frame 1, as a camera network that lost it would deliver
them, go to two linkers with motion -- one is told nothing and takes the frames for consecutive, the other gets a time stamp per frame
(linker(s, times=...)), so the hole is a gap of two periods: its velocities stay displacements per PERIOD and its gate and prediction
cover the time that really passed.  A TrackGallery (gnn_cca_amd.reentry) stands behind the linker WITHOUT max_gap: it cannot bridge the
hidden frame, so person 0 comes back as a new track, and the gallery gives that track the old identity back by appearance; its
identities are scored like track ids.  With --exclusive one more linker runs the WAITING-FREE loop on a partition that is legal by
construction: r.exclusive() (no cluster holds two detections of one camera, whatever the number of cameras; no wait for the host
heuristics of final()) -> cluster_summaries -> FrameLinker, one extra line per batch.  With --smooth a TrackSmoother (gnn_cca_amd.smoothing)
stands behind the linker with max_gap=1: a constant-velocity Kalman filter along every track turns the ids into trajectories -- filtered
position, velocity, their variances, and how far a detection lay from where its track was expected; one extra line per batch (these
persons wander without a heading, so the filtered velocity is small: DESIGN.md section 9 has straight walks).  With --kalman a
KalmanLinker (gnn_cca_amd.kalman) links the true partition with that filter INSIDE the linker: a track is looked for where its filtered
state predicts it and a pair is gated by the variance of the prediction (max_nis); its tracks carry their trajectories, and it is scored
like the others.  The scorers' result() is the last thing printed (synthetic walks and the ground-truth partition: what linking does to tracking quality with a trained model has not been measured).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (model / GRAPH_NET_PARAMS builders)
from gnn_cca_amd.kalman import KalmanLinker  # noqa: E402
from gnn_cca_amd.pipeline import FramePipeline  # noqa: E402
from gnn_cca_amd.reentry import TrackGallery  # noqa: E402
from gnn_cca_amd.smoothing import TrackSmoother  # noqa: E402
from gnn_cca_amd.tracking import ClusterSummaries, FrameLinker, Tracks, TrackScorer, cluster_summaries  # noqa: E402


def without_frame(s, q):
    """The summaries of a batch without its frame q (rows are per frame, so the others move up as they are)."""
    ptr = s.node_ptr
    kept = [g for g in range(len(ptr) - 1) if g != q]
    rows = torch.cat([torch.arange(ptr[g], ptr[g + 1]) for g in kept]).to(s.rank.device)
    new_ptr = np.concatenate([[0], np.cumsum([ptr[g + 1] - ptr[g] for g in kept])])
    return ClusterSummaries(s.count[kept], s.rank[rows], s.size[rows], s.n_cams[rows], s.pos[rows], s.emb[rows], new_ptr.tolist(),
                            torch.from_numpy(new_ptr.astype(np.int32)).to(s.rank.device)), kept


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("batches", nargs="?", type=int, default=3)
    ap.add_argument("frames", nargs="?", type=int, default=8, metavar="frames_per_batch")
    ap.add_argument("cams", nargs="?", type=int, default=4)
    ap.add_argument("persons", nargs="?", type=int, default=6)
    ap.add_argument("--exclusive", action="store_true", help="also link the camera-exclusive clusters of r.exclusive(): the loop that never waits")
    ap.add_argument("--smooth", action="store_true", help="also filter the tracks of the max_gap=1 linker: trajectories with velocities and variances")
    ap.add_argument("--kalman", action="store_true", help="also link the true partition by the filtered state, gated by its variance")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n_g = a.cams * a.persons
    model = bench.build_model(bench.graph_net_params(), n_g).cuda().eval()
    pipe = FramePipeline(model)
    by_model, by_truth = FrameLinker(max_step=1.0, lam=1.0), FrameLinker(max_step=1.0, lam=1.0)
    by_exclusive = FrameLinker(max_step=1.0, lam=1.0)              # --exclusive: the model's probabilities, at most one detection per camera
    by_truth_gap = FrameLinker(max_step=1.0, lam=1.0, max_gap=1)   # a track survives one frame that misses it
    by_truth_opt = FrameLinker(max_step=1.0, lam=1.0, max_gap=1, matching="optimal")   # per frame pair the min-cost assignment, not mutual best
    score, score_gap = TrackScorer(max_ids=a.persons, max_cams=a.cams), TrackScorer(max_ids=a.persons, max_cams=a.cams)
    score_opt = TrackScorer(max_ids=a.persons, max_cams=a.cams)
    by_truth_vel = FrameLinker(max_step=1.0, lam=1.0, max_gap=1, motion="velocity")   # a cluster is looked for where it is heading
    score_vel = TrackScorer(max_ids=a.persons, max_cams=a.cams)
    gallery = TrackGallery(by_truth, max_cos=0.3)   # ended tracks, matched against newly born ones by appearance
    # --smooth: the walk's step is 0.15 per axis and frame (the process noise), a detection's noise 0.05, and a cluster fuses `cams` of them
    smooth = TrackSmoother(by_truth_gap, process_noise=0.15 ** 2, measurement_noise=0.05 ** 2, vel_var=0.15 ** 2, per_detection=True)
    # --kalman: the filter inside the linker.  These persons WANDER: a step of 0.15 per axis and frame without a heading is, to a
    # constant-velocity model, noise around a velocity near zero, so it goes into the measurement variance beside the fused detection
    # noise (with r = 0.05 ** 2 / cams alone the variance gate, 13.8 = chi-square(2) at one in a thousand, cuts tracks at ordinary steps)
    by_truth_kal = KalmanLinker(max_step=1.0, process_noise=0.15 ** 2, measurement_noise=0.15 ** 2 + 0.05 ** 2 / a.cams, vel_var=0.15 ** 2,
                                lam=1.0, max_gap=1, max_nis=13.8)
    score_kal = TrackScorer(max_ids=a.persons, max_cams=a.cams)
    score_back = TrackScorer(max_ids=a.persons, max_cams=a.cams)
    blind, timed = (FrameLinker(max_step=1.0, lam=1.0, max_gap=1, motion="velocity") for _ in range(2))   # for the batches that lost a frame
    where = rng.uniform(-8, 8, size=(a.persons, 2))
    look = rng.standard_normal((a.persons, 256)).astype(np.float32)
    id_cam = np.tile(np.repeat(np.arange(a.cams), a.persons), a.frames)
    ids = np.tile(np.tile(np.arange(a.persons), a.cams), a.frames).astype(np.int64)
    frame_of = np.repeat(np.arange(a.frames), n_g)
    hidden = a.frames // 2                                    # the frame in which nobody sees person 0 (none in a one-frame batch)
    seen = ~((frame_of == hidden) & (ids == 0)) if a.frames > 1 else np.ones(len(ids), bool)
    id_cam, ids, frame_of = id_cam[seen], ids[seen], frame_of[seen]
    sizes = np.bincount(frame_of, minlength=a.frames).tolist()
    n = len(ids)
    # the ground-truth partition in the pipeline's convention: a detection's label is the smallest node id of its person in its frame
    first = {}
    truth = torch.tensor([first.setdefault((q, p), v) for v, (q, p) in enumerate(zip(frame_of.tolist(), ids.tolist()))], dtype=torch.int32).cuda()
    for k in range(a.batches):
        steps = np.cumsum(rng.normal(0, 0.15, size=(a.frames, a.persons, 2)), axis=0)
        walk = where[None] + steps
        where = walk[-1]
        xw = walk[frame_of, ids, 0] + rng.normal(0, 0.05, n)
        yw = walk[frame_of, ids, 1] + rng.normal(0, 0.05, n)
        node = torch.randn(n, 2048, device="cuda")
        reid = torch.from_numpy(look[ids] + 0.1 * rng.standard_normal((n, 256)).astype(np.float32)).cuda()
        r = pipe(xw, yw, ids, id_cam, sizes, [80.0] * a.frames, node, reid)
        s = r.identities(final=False)            # the device chain's partition, no wait for the host heuristics (final=True: r.final()'s)
        t = by_model(s)                          # or by_model(r): a FrameResult's identities() are taken
        st = cluster_summaries(r.batch, truth)   # any partition of the batch's detections can be summarised
        tt = by_truth(st)
        tg = by_truth_gap(st)                    # tg.matched_gap: 1 where a cluster continues one that was last seen two frames ago
        if a.smooth:
            tj = smooth(st, tg)                  # Trajectories: pos / vel [N, 2], cov [N, 3], nis [N], age [N], rows as tg.cluster_track
        back = gallery(st, tt)                   # identities: a track born after an absence too long for the linker takes an ended track's
        score_back.add(r, Tracks(back.cluster_identity, back.node_identity, tt.matched_prev, tt.next_id, None))   # scored where tracks stood
        score.add(r, tt)                         # ids (batch.y), cameras and node tracks joined over time: nothing waits for the GPU
        score_gap.add(r, tg)
        score_opt.add(r, by_truth_opt(st))
        tv = by_truth_vel(st)                    # tv.velocity: float64 [N, 2], the displacement per frame since the predecessor
        score_vel.add(r, tv)
        if a.kalman:
            tk = by_truth_kal(st)                # KalmanTracks: a Tracks whose velocity is the filtered one, plus tk.trajectories
            score_kal.add(r, tk)
        if a.exclusive:   # exclusive() -> cluster_summaries -> FrameLinker: device work only, legal clusters without final()'s wait
            ex = r.exclusive()
            se = cluster_summaries(r.batch, ex["labels"])
            te = by_exclusive(se)
        # ---- only the printing below waits for the GPU ----
        last = slice(r.batch.node_ptr[-2], r.batch.node_ptr[-1])
        k_model, k_truth = int(s.count[-1].item()), int(st.count[-1].item())
        print(f"batch {k}: {a.frames} frames, N={n}; model partition: {int(s.count.sum().item())} clusters, tracks so far {int(t.next_id.item())}; "
              f"true partition: {int(st.count.sum().item())} clusters, tracks so far {int(tt.next_id.item())}")
        print(f"  last frame, true partition: ids {tt.cluster_track[last][:k_truth].tolist()} at "
              f"{[[round(v, 2) for v in p] for p in st.pos[last][:k_truth].tolist()]}, cameras {st.n_cams[last][:k_truth].tolist()}")
        print(f"  last frame, model partition: {k_model} clusters, sizes {s.size[last][:k_model].tolist()}")
        print(f"  last frame, true partition, motion='velocity': ids {tv.cluster_track[last][:k_truth].tolist()}, velocities "
              f"{[[round(v, 2) for v in p] for p in tv.velocity[last][:k_truth].tolist()]}")
        if a.exclusive:
            print(f"  exclusive partition: {int(ex['n_clusters'].item())} clusters, every one with size == cameras: "
                  f"{bool((se.size == se.n_cams).all().item())} (model partition: {bool((s.size == s.n_cams).all().item())}); candidate pairs cut "
                  f"{int(ex['cut'].sum().item())}, tracks so far {int(te.next_id.item())}")
        if a.smooth:
            print(f"  last frame, true partition, smoothed: positions {[[round(v, 2) for v in p] for p in tj.pos[last][:k_truth].tolist()]}, "
                  f"velocities {[[round(v, 2) for v in p] for p in tj.vel[last][:k_truth].tolist()]}, position sigma "
                  f"{[round(v ** 0.5, 3) for v in tj.cov[last][:k_truth, 0].tolist()]}, links since birth {tj.age[last][:k_truth].tolist()}, "
                  f"largest nis of the batch {float(tj.nis.max()):.2f}")
        if a.kalman:
            tj2 = tk.trajectories
            print(f"  last frame, true partition, KalmanLinker: ids {tk.cluster_track[last][:k_truth].tolist()}, filtered velocities "
                  f"{[[round(v, 2) for v in p] for p in tk.velocity[last][:k_truth].tolist()]}, position sigma "
                  f"{[round(v ** 0.5, 3) for v in tj2.cov[last][:k_truth, 0].tolist()]}, links since birth {tj2.age[last][:k_truth].tolist()}, "
                  f"largest nis of the batch {float(tj2.nis.max()):.2f} (gate 13.8)")
        if a.frames > 2:   # frame 1 never arrives: without time stamps the step over the hole passes for one period's
            sd, kept = without_frame(st, 1)
            tb = blind(sd)
            tm = timed(sd, times=[k * a.frames + g for g in kept])   # (host numbers, checked before any launch; nothing waits for the GPU)
            hole = slice(sd.node_ptr[1], sd.node_ptr[1] + int(sd.count[1].item()))   # the first frame after the hole
            speed = lambda t: [round(float(v), 2) for v in t.velocity[hole].norm(dim=1).tolist()]
            print(f"  frame 1 dropped: speeds in the frame after the hole {speed(tb)} taken for consecutive, {speed(tm)} per period with "
                  f"times; tracks so far {int(tb.next_id.item())} against {int(tm.next_id.item())}")
        if a.frames > 2:   # person 0 is cluster 0 of every frame that shows them (their camera-0 detection is the frame's first node)
            before, after = r.batch.node_ptr[hidden - 1], r.batch.node_ptr[hidden + 1]
            print(f"  person 0, hidden in frame {hidden}: id {int(tt.cluster_track[before])} -> {int(tt.cluster_track[after])} without max_gap, "
                  f"{int(tg.cluster_track[before])} -> {int(tg.cluster_track[after])} with max_gap=1 "
                  f"(matched_gap {int(tg.matched_gap[after])}); tracks so far {int(tt.next_id.item())} against {int(tg.next_id.item())}")
            print(f"  ... and behind the linker without max_gap the gallery: identity {int(back.cluster_identity[before])} -> "
                  f"{int(back.cluster_identity[after])} (re-entered from track {int(back.reentered_from[after])})")
    print("random weights: the model's clusters are meaningless, the plumbing is what is shown; on the true partition a person keeps its id")
    for name, sc in (("without max_gap", score), ("without max_gap, identities of the re-entry gallery", score_back), ("with max_gap=1", score_gap), ("with max_gap=1, matching='optimal'", score_opt),
                     ("with max_gap=1, motion='velocity'", score_vel)) + ((("with max_gap=1, KalmanLinker(max_nis=13.8)", score_kal),) if a.kalman else ()):   # result(): the one synchronisation of a scorer
        res = sc.result()
        print(f"true partition {name}: " + ", ".join(f"{q} {v:.3f}" if isinstance(v, float) else f"{q} {v}" for q, v in res.items()))


if __name__ == "__main__":
    main()
