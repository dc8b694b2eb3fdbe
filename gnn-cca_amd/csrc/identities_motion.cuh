// identities_motion.cuh -- gap-tolerant linking with a constant-velocity prediction (gnncca_link_frames_motion), included at the end of
// identities.hip after identities_gap.cuh and identities_assign.cuh.  The pair rule, the partner search, side_b, the numbering, the history
// state and its slot writer, link_init_kernel and plan_history are link_common.cuh's, shared with the other linkers.
//
// The rule (include/gnncca_mpn.h has it in full): the levels, gates, masks, cost, mutual best and ties of gnncca_link_frames_gap, but at
// level k cluster b of frame t - 1 - k is looked for at pred(b) = pos(b) + (double)(k + 1) * vel(b), and a cluster a linked at level k to b
// gets vel(a) = (pos(a) - pos(b)) / (double)(k + 1).  vel(b) is known only when frame t - 1 - k has been through ALL its levels, so the
// order is frames outside, levels inside: the dependency is serial in time and ONE workgroup walks the frames of the batch.
// Launches, 3 of them whatever max_gap is:
//   1. link_init_kernel (frame-parallel), with a velocity array: predecessor record of the N batch rows = none, velocity = 0, successor
//      flags of the S history rows copied from state_in (which is never written), of the batch rows cleared -- one array over the
//      COMBINED rows as in the gap path.
//   2. motion_walk_kernel, grid = 1: for every frame in order the levels 0 .. M (fwd / bwd in LDS, mutual_best with side B standing at
//      pos + steps * vel, commit between barriers), then the ids at once -- the running next_id is known because the frames go in order;
//      the clusters without a predecessor are numbered in ascending rank (number_fresh).  No workgroup waits for another: there is only one.
//      The walk is one workgroup deep, so a table's chain of memory round trips is what it waits for: the search loads a row's and a
//      column's mask, position and velocity together and looks at the mask afterwards (side_at), and this kernel instantiates the cosine
//      with FOUR loads per side in flight, added in the order of the one-load loop (the same bits).
//   3. motion_finish_kernel, grid = G + the history frames carried along (frame-parallel): node tracks and the rows of the new state.
// Arrays the walking workgroup writes and later reads (the predecessor record, the successor flags, velocity, cluster_track) are plain
// pointers -- not const, not __restrict__ -- and every frame's and level's writes are ordered before the next one's reads by __syncthreads().
// They reach the walk as one block (WalkOutputs) that it keeps in LDS and reads where a level is set up, committed or numbered: held in
// scalar registers over the whole walk they did not fit beside the two inlined partner searches (DESIGN.md section 9 has the numbers).
// For the same reason the row count S of the old state is read from the LDS copy of the offsets where it is used.
// The carried state is the history state of link_common.cuh WITH velocities: a state of its own kind, the gap state's layout is as it was.
#pragma once

namespace gnncca {

// what the walk writes (and, in later frames, reads) and what only the set-up of a level needs: plain pointers, passed as one block
struct WalkOutputs {
    int* matched_prev;
    int* matched_gap;
    double* velocity;
    long long* cluster_track;
    long long* next_id;
    int* succ;                // the successor flags over the combined rows
    const char* state_in;     // (never written)
    double lam, max_cos;      // the rule's two numbers that only the inside of a gate needs
    const float* emb;         // the batch's appearance rows (never written)
};

// the same block for a call with time stamps: two more members, read where a level is set up
struct TimedWalkOutputs : WalkOutputs {
    const double* frame_time; // time stamps over the combined frames, fp64 [history frames + G] (never written)
    double max_dt;            // a table whose dt is not in (0, max_dt] is skipped
};

// One workgroup, every frame of the batch in order.  `rule.max_step` is the caller's max_step; the gate of level k is max_step * (k + 1),
// one fp64 multiplication; with time stamps (outs.frame_time) dt = T[t] - T[t - 1 - k], one fp64 subtraction, stands wherever k + 1 does,
// and a table with !(dt > 0 && dt <= max_dt) is skipped whole.  Timed or not is the TYPE of the block (OUTS = WalkOutputs or
// TimedWalkOutputs), not a null check: the untimed instantiation is the walk as it was, argument for argument (read at run time, the
// pointer's round trip to LDS and back stood in front of every level's search and cost the untimed call 0.027 ms of 0.94 on 64 frames
// x 3 levels, outside the run-to-run spread).  Every loop is bounded by G, max_gap, P_lds (a count above it is taken as 0) or the 64 lanes of a wave.
template <int BLOCK, class OUTS>
__global__ __launch_bounds__(BLOCK) void motion_walk_kernel(const int* __restrict__ node_ptr, int N_all, int G, const int* __restrict__ count,
                                                            const double* __restrict__ pos, int R, LinkRule rule,
                                                            int max_gap, GapFrames in, int P_lds, OUTS outs) {
    constexpr bool TIMED = std::is_same_v<OUTS, TimedWalkOutputs>;
    extern __shared__ int s_dyn[];
    __shared__ int s_fresh;
    int* fwd = s_dyn;                // [a] -> b; after the levels: a fresh cluster's rank among the frame's fresh ones
    int* bwd = s_dyn + P_lds;        // [b] -> a
    int* gap_a = s_dyn + 2 * P_lds;  // the frame's predecessor record as it grows: -1, or the level that found it
    const int tid = threadIdx.x;
    // What only the set-up of a level, the commit and the ids use is kept in LDS and read where it is used, not held in scalar registers
    // over the walk: the history's row offsets (s_off[HN] = S, the rows of the old state) and the output pointers.
    __shared__ int s_off[kGapMaxFrames + 1];
    __shared__ OUTS s_out;
    if (tid <= kGapMaxFrames) s_off[tid] = in.off[tid];
    if (tid == 0) s_out = outs;
    const int HN = in.n;
    __syncthreads();
    long long next_id = outs.state_in ? reinterpret_cast<const GapHeader*>(outs.state_in)->next_id : 0;   // (the same in every thread)

    for (int t = 0; t < G; ++t) {
        int v0, n;
        const bool ok = frame_range(node_ptr, t, N_all, v0, n);
        const int ca = ok ? usable_count(count, t, n, P_lds) : 0;
        for (int a = tid; a < ca; a += BLOCK) gap_a[a] = -1;
        __syncthreads();
        const double* apos = pos + 2 * (size_t)v0;
        const float* emb = s_out.emb;
        const float* aemb = emb + (size_t)v0 * R;
        for (int k = 0; k <= max_gap && ca > 0; ++k) {
            int* succ_ws = s_out.succ;
            int brow;   // the combined row of B's rank 0
            const int S = __builtin_amdgcn_readfirstlane(s_off[HN]);   // (read here, not held over the walk)
            LinkSide sb = side_b(t - 1 - k, node_ptr, N_all, count, pos, s_out.velocity, emb, R, s_out.state_in, HN, s_off, S, true, P_lds, brow);
            if (sb.n == 0) continue;   // (uniform: the counts are the same in every thread)
            sb.mask = succ_ws + brow, sb.free = 0;
            const LinkSide sa{apos, nullptr, aemb, gap_a, -1, ca};
            const double* bpos = sb.pos;
            double steps = (double)(k + 1);
            if constexpr (TIMED) {   // (uniform; side B exists, so HN + t - 1 - k >= 0.  The null check stays: without it this instantiation spilled 2 SGPRs)
                const double* frame_time = s_out.frame_time;
                if (frame_time && !level_dt(frame_time, HN + t, HN + t - 1 - k, s_out.max_dt, steps)) continue;
            }
            const LinkRule level_rule{rule.max_step * steps, s_out.lam, s_out.max_cos, rule.need_emb, rule.has_max_cos};   // gate_k: one fp64 multiplication
            mutual_best<BLOCK, 4, true>(sa, sb, steps, R, level_rule, fwd, bwd);
            __syncthreads();   // (every read of the masks above comes before the writes below)
            int* matched_prev = s_out.matched_prev;
            int* matched_gap = s_out.matched_gap;
            double* velocity = s_out.velocity;
            for (int a = tid; a < ca; a += BLOCK) {
                const int b = fwd[a];
                if (b >= 0 && bwd[b] == a) {   // (fwd[a] >= 0 only where a had no predecessor; bwd[b] == a only where b had no successor)
                    matched_prev[v0 + a] = b;
                    matched_gap[v0 + a] = k;
                    gap_a[a] = k;
                    succ_ws[brow + b] = 1;
                    velocity[2 * (size_t)(v0 + a)] = (apos[2 * (size_t)a] - bpos[2 * (size_t)b]) / steps;
                    velocity[2 * (size_t)(v0 + a) + 1] = (apos[2 * (size_t)a + 1] - bpos[2 * (size_t)b + 1]) / steps;
                }
            }
            __syncthreads();   // (the next level, and the next frame, read what this one wrote)
        }
        number_fresh(gap_a, ca, fwd, &s_fresh);   // the clusters without a predecessor, numbered in rank order
        __syncthreads();
        const int* matched_prev = s_out.matched_prev;
        long long* cluster_track = s_out.cluster_track;
        const char* state_in = s_out.state_in;
        for (int a = tid; a < ca; a += BLOCK) {
            const int k = gap_a[a];
            long long id;
            if (k < 0) {
                id = next_id + fwd[a];
            } else {   // (a level wrote a match only into a usable earlier frame, whose ids are final)
                const int m = matched_prev[v0 + a], tp = t - 1 - k;
                id = tp >= 0 ? cluster_track[node_ptr[tp] + m]
                              : StateView(state_in, s_off[HN], R, true).track[s_off[HN + tp] + m];
            }
            cluster_track[v0 + a] = id;
        }
        for (int c = ca + tid; c < n; c += BLOCK) cluster_track[v0 + c] = -1;
        next_id += s_fresh;
        __syncthreads();   // (s_fresh, fwd and gap_a are the next frame's to write; its levels read this frame's ids and velocities)
    }
    if (tid == 0) *s_out.next_id = next_id;
}

// ---- launch 3: node tracks, the new state ---------------------------------------------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void motion_finish_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                              const int* __restrict__ rank, const double* __restrict__ pos,
                                                              const float* __restrict__ emb, int R, int G, const double* __restrict__ velocity,
                                                              const long long* __restrict__ cluster_track, const int* __restrict__ succ_ws,
                                                              const char* __restrict__ state_in, GapFrames in, char* __restrict__ state_out,
                                                              GapFrames out, int P_lds, long long* __restrict__ node_track) {
    const int tid = threadIdx.x;
    const int S = in.off[in.n];
    const StateView ov(state_out, out.off[out.n], R, true);   // (next_id, at offset 0 of its header, is the walk's to write)
    const int first_kept = G - out.n;   // the batch frame that becomes slot 0 of the new state (negative: history frames stay)

    if ((int)blockIdx.x >= G) {   // a history frame that stays: slot j of the new state is frame f of the old one
        const int j = (int)blockIdx.x - G;
        keep_slot<BLOCK>(ov, out, j, state_in, in, in.n + first_kept + j, R, true, succ_ws, P_lds);
        return;
    }

    const int g = blockIdx.x;
    int v0, n;
    const bool ok = frame_range(node_ptr, g, N_all, v0, n);
    const int ca = ok ? usable_count(count, g, n, P_lds) : 0;
    write_node_tracks<BLOCK>(rank + v0, n, ca, cluster_track + v0, node_track + v0);
    if (g == G - 1 && tid == 0) {
        ov.head->n_frames = out.n;
        ov.head->reid_dim = R;
    }
    if (g < first_kept) return;
    const int j = g - first_kept, orow = out.off[j];
    const int cs = ca <= out.off[j + 1] - orow ? ca : 0;   // (a frame with more clusters than its slot has rows is carried as empty)
    write_slot<BLOCK>(ov, j, orow, cs, R, pos + 2 * (size_t)v0, velocity + 2 * (size_t)v0, cluster_track + v0, succ_ws + S + v0, emb + (size_t)v0 * R);
}

constexpr int kMotionWalkBlock = 1024;   // one workgroup has the CU to itself, a wave takes a row

}  // namespace gnncca

extern "C" {

size_t gnncca_link_motion_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim) {
    if (capacity_rows < 0 || reid_dim < 0 || n_frames_kept < 0 || n_frames_kept > gnncca::kGapMaxFrames) return 0;
    return gnncca::round256(gnncca::hist_succ_off(capacity_rows, reid_dim, true) + (size_t)capacity_rows * sizeof(int32_t));
}

size_t gnncca_link_motion_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows) {
    if (n_nodes < 0 || n_frames < 0 || state_rows < 0) return 0;
    return gnncca::round256(((size_t)state_rows + (size_t)n_nodes) * sizeof(int32_t));   // successor flags [S + N]
}

}  // extern "C"

namespace gnncca {

// gnncca_link_frames_motion and gnncca_link_frames_motion_timed: one body (frame_time nullptr from the untimed entry)
static int link_frames_motion_run(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                                  int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                                  int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t motion, const void* state_in,
                                  const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                                  const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                                  int32_t* matched_prev, int32_t* matched_gap, double* velocity, void* workspace, size_t workspace_bytes,
                                  gnncca_stream_t stream, const double* frame_time, double max_dt) {
    if (motion != 1) return GNNCCA_ERR_INVALID_ARG;
    HistoryPlan p;
    const int rc = plan_history(n_nodes, n_frames, reid_dim, max_frame_nodes, max_step, lam, has_max_cos, max_cos, max_gap, 0, state_in,
                                state_in_frame_rows, state_in_frames, state_out, state_out_frame_rows, state_out_frames, node_ptr_dev, count, emb,
                                rank && pos && cluster_track && node_track && matched_prev && matched_gap && velocity, workspace,
                                workspace_bytes, gnncca_link_motion_workspace_bytes, p);
    if (rc != GNNCCA_OK || p.nothing) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* succ_ws = static_cast<int*>(workspace);
    char* sout = static_cast<char*>(state_out);
    launch_link_init(st, p, true, n_nodes, succ_ws, matched_prev, matched_gap, velocity);
    HIP_TRY(hipGetLastError());
    const WalkOutputs outs{matched_prev, matched_gap, velocity, reinterpret_cast<long long*>(cluster_track),
                           &reinterpret_cast<GapHeader*>(sout)->next_id, succ_ws, p.sin, lam, max_cos, emb};
    if (!frame_time) {
        hipLaunchKernelGGL((motion_walk_kernel<kMotionWalkBlock, WalkOutputs>), dim3(1), dim3(kMotionWalkBlock), (size_t)3 * p.P * sizeof(int), st,
                           node_ptr_dev, (int)n_nodes, (int)n_frames, count, pos, p.R, p.rule, (int)max_gap, p.in, p.P, outs);
    } else {
        TimedWalkOutputs timed;
        static_cast<WalkOutputs&>(timed) = outs;
        timed.frame_time = frame_time, timed.max_dt = max_dt;
        hipLaunchKernelGGL((motion_walk_kernel<kMotionWalkBlock, TimedWalkOutputs>), dim3(1), dim3(kMotionWalkBlock), (size_t)3 * p.P * sizeof(int),
                           st, node_ptr_dev, (int)n_nodes, (int)n_frames, count, pos, p.R, p.rule, (int)max_gap, p.in, p.P, timed);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((motion_finish_kernel<256>), dim3((unsigned)(n_frames + p.carried)), dim3(256), 0, st, node_ptr_dev, (int)n_nodes, count, rank,
                       pos, emb, p.R, (int)n_frames, velocity, reinterpret_cast<const long long*>(cluster_track), succ_ws, p.sin, p.in, sout, p.out, p.P,
                       reinterpret_cast<long long*>(node_track));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // namespace gnncca

extern "C" {

int gnncca_link_frames_motion(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                              int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                              int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t motion, const void* state_in,
                              const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                              const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                              int32_t* matched_prev, int32_t* matched_gap, double* velocity, void* workspace, size_t workspace_bytes,
                              gnncca_stream_t stream) {
    return gnncca::link_frames_motion_run(node_ptr_dev, count, rank, pos, emb, reid_dim, n_nodes, n_frames, max_frame_nodes, max_step, lam,
                                          has_max_cos, max_cos, max_gap, motion, state_in, state_in_frame_rows, state_in_frames, state_out,
                                          state_out_frame_rows, state_out_frames, cluster_track, node_track, matched_prev, matched_gap, velocity,
                                          workspace, workspace_bytes, stream, nullptr, 0.0);
}

/* gnncca_link_frames_motion with a time stamp per frame (include/gnncca_mpn.h has the rule): the same run; dt from frame_time_dev, fp64
 * [state_in_frames + n_frames], stands where k + 1 does in the gate, the prediction and the velocity. */
int gnncca_link_frames_motion_timed(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                                    int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                                    int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t motion, const void* state_in,
                                    const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                                    const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                                    int32_t* matched_prev, int32_t* matched_gap, double* velocity, void* workspace, size_t workspace_bytes,
                                    gnncca_stream_t stream, const double* frame_time_dev, double max_dt) {
    if (!(max_dt > 0.0) || !(max_dt < __builtin_inf())) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames > 0 && !frame_time_dev) return GNNCCA_ERR_INVALID_ARG;
    return gnncca::link_frames_motion_run(node_ptr_dev, count, rank, pos, emb, reid_dim, n_nodes, n_frames, max_frame_nodes, max_step, lam,
                                          has_max_cos, max_cos, max_gap, motion, state_in, state_in_frame_rows, state_in_frames, state_out,
                                          state_out_frame_rows, state_out_frames, cluster_track, node_track, matched_prev, matched_gap, velocity,
                                          workspace, workspace_bytes, stream, frame_time_dev, max_dt);
}

}  // extern "C"
