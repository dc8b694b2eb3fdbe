// identities_kalman.cuh -- gap-tolerant linking by a constant-velocity Kalman filter (gnncca_link_frames_kalman), included at the end of
// identities.hip after identities_motion.cuh: the motion walk whose prediction starts from the FILTERED position and velocity, whose links
// feed the filter, and whose pairs may in addition be gated by the innovation variance.  The pair rule, the partner search, side_b, the
// numbering, the history state and its slot writer, plan_history and the filter's arithmetic (cv_predicted_var, cv_kalman_step: the
// smoother's lines) are link_common.cuh's; WalkOutputs is identities_motion.cuh's.
//
// The rule (include/gnncca_mpn.h has it in full, tests/tracking_kalman_oracle.py as loops).  Frames outside, levels 0 .. max_gap inside,
// dt = (double)(k + 1) or, with time stamps, T[t] - T[t - 1 - k] (a table with dt outside (0, max_dt] is skipped whole).  Every cluster
// carries x = (px, py, vx, vy, a, b, c) and an age.  At level k cluster b of frame t - 1 - k without a successor stands at
// pred(b) = p(b) + dt * v(b); d, the gate max_step * dt, the cosine term, max_cos and the cost are the shared pair rule between the RAW
// pos(a) and pred(b); with max_nis a pair is admissible only if also (dx*dx + dy*dy) / s <= max_nis, s = a_ + r, a_ the predicted
// position variance of b after dt.  Mutual best, ties to the smaller index, a shorter gap wins.  On commit
// x(a), nis(a), age(a) = step(x(b), age(b), z = pos(a), dt, q, r); a cluster without a predecessor starts as (z, 0, 0, r, 0, vel_var),
// age 0, nis 0.  Ids as in the motion walk.
// Launches, 3 of them whatever max_gap is:
//   1. kalman_init_kernel (frame-parallel): link_init_kernel's work, and the five filter outputs of the N batch rows = zero, age = -1 (what
//      a row at or beyond its frame's count keeps).
//   2. kalman_walk_kernel, grid = 1: motion_walk_kernel's structure.  Side B is a LinkSide whose pos and vel point at the filtered arrays
//      (of the batch's outputs or of the carried state), so side_at, best_partner and mutual_best are used as they are; the variance gate is
//      the extra admissibility predicate of pair_rule (VarianceGate).  s depends on (b, level) only: with max_nis the workgroup computes it
//      once per level into an LDS array of P_lds doubles, before the search, between barriers.  The commit loop runs the filter's step
//      per linked row and writes x, nis and age; the numbering loop writes the births.  Between a level's writes and the next reads stand
//      the same __syncthreads() as in the motion walk.  Every loop is bounded by G, max_gap, P_lds or the 64 lanes of a wave.
//   3. kalman_finish_kernel (frame-parallel): node tracks and the rows of the new state, cov and age included.
// The carried state is the history state of link_common.cuh of the Kalman kind: the state with velocities, pos and vel filtered, plus
// cov fp64 [C][3] and age int32 [C].  Timed or not is the TYPE of the outputs block, as in the motion walk: the untimed instantiation has
// no load of a time.
#pragma once

namespace gnncca {

// WalkOutputs (velocity: the FILTERED velocity) and what the filter adds: plain pointers the walk writes and later reads, and its numbers
struct KalmanOutputs : WalkOutputs {
    double* fpos;   // filtered position [N][2]
    double* cov;    // [N][3]
    double* nis;    // [N]
    int* age;       // [N]
    double q, r, vel_var, max_nis;
    int has_nis;
};

struct TimedKalmanOutputs : KalmanOutputs {
    const double* frame_time;
    double max_dt;
};

// ---- launch 1: link_init_kernel's work plus the filter outputs of the batch rows ---------------------------------------------------------
__global__ __launch_bounds__(256) void kalman_init_kernel(const int* __restrict__ in_succ, int S, int N_all, int* __restrict__ succ_ws,
                                                          int* __restrict__ matched_prev, int* __restrict__ matched_gap,
                                                          double* __restrict__ fpos, double* __restrict__ vel, double* __restrict__ cov,
                                                          double* __restrict__ nis, int* __restrict__ age) {
    const long long total = (long long)S + N_all;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (i < S) {
            succ_ws[i] = in_succ[i] != 0;
        } else {
            const long long v = i - S;
            succ_ws[i] = 0;
            matched_prev[v] = -1;
            matched_gap[v] = -1;
            fpos[2 * v] = 0.0, fpos[2 * v + 1] = 0.0;
            vel[2 * v] = 0.0, vel[2 * v + 1] = 0.0;
            cov[3 * v] = 0.0, cov[3 * v + 1] = 0.0, cov[3 * v + 2] = 0.0;
            nis[v] = 0.0;
            age[v] = -1;
        }
    }
}

// ---- launch 2 ----------------------------------------------------------------------------------------------------------------------------
// One workgroup, every frame of the batch in order.  Dynamic LDS: nis_lds doubles (P_lds with a variance gate, else 0: s per cluster of
// side B at the level at hand), then fwd, bwd, gap_a as in the motion walk.
template <int BLOCK, class OUTS>
__global__ __launch_bounds__(BLOCK) void kalman_walk_kernel(const int* __restrict__ node_ptr, int N_all, int G, const int* __restrict__ count,
                                                            const double* __restrict__ pos, int R, LinkRule rule, int max_gap, GapFrames in,
                                                            int P_lds, int nis_lds, OUTS outs) {
    constexpr bool TIMED = std::is_same_v<OUTS, TimedKalmanOutputs>;
    extern __shared__ double s_kal[];
    __shared__ int s_fresh;
    double* s_var = s_kal;
    int* fwd = reinterpret_cast<int*>(s_kal + nis_lds);   // [a] -> b; after the levels: a fresh cluster's rank among the frame's fresh ones
    int* bwd = fwd + P_lds;                               // [b] -> a
    int* gap_a = fwd + 2 * P_lds;                         // the frame's predecessor record as it grows: -1, or the level that found it
    const int tid = threadIdx.x;
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
        const double* apos = pos + 2 * (size_t)v0;   // the RAW positions: the measurements
        const float* emb = s_out.emb;
        const float* aemb = emb + (size_t)v0 * R;
        for (int k = 0; k <= max_gap && ca > 0; ++k) {
            int* succ_ws = s_out.succ;
            int brow;   // the combined row of B's rank 0
            const int S = __builtin_amdgcn_readfirstlane(s_off[HN]);
            const int sf = t - 1 - k;
            // side B stands at its FILTERED position plus dt times its FILTERED velocity
            LinkSide sb = side_b(sf, node_ptr, N_all, count, s_out.fpos, s_out.velocity, emb, R, s_out.state_in, HN, s_off, S, kStateKalman, P_lds,
                                 brow);
            if (sb.n == 0) continue;   // (uniform: the counts are the same in every thread)
            sb.mask = succ_ws + brow, sb.free = 0;
            const LinkSide sa{apos, nullptr, aemb, gap_a, -1, ca};
            double steps = (double)(k + 1);
            if constexpr (TIMED) {   // (uniform; side B exists, so HN + t - 1 - k >= 0)
                if (!level_dt(s_out.frame_time, HN + t, HN + sf, s_out.max_dt, steps)) continue;
            }
            const double* bcov;   // side B's covariances and ages: of the batch's outputs, or of the carried state
            const int* bage;
            if (sf >= 0) {
                bcov = s_out.cov + 3 * (size_t)(brow - S);
                bage = s_out.age + (brow - S);
            } else {
                const StateView old(s_out.state_in, S, R, kStateKalman);
                bcov = old.cov + 3 * (size_t)brow;
                bage = old.age + brow;
            }
            const int has_nis = s_out.has_nis;
            if (has_nis) {   // (uniform) s = a_ + r per cluster of side B, once per level
                const double q = s_out.q, r = s_out.r;
                for (int b = tid; b < sb.n; b += BLOCK)
                    s_var[b] = cv_predicted_var(bcov[3 * (size_t)b], bcov[3 * (size_t)b + 1], bcov[3 * (size_t)b + 2], steps, q) + r;
                __syncthreads();
            }
            const LinkRule level_rule{rule.max_step * steps, s_out.lam, s_out.max_cos, rule.need_emb, rule.has_max_cos};   // gate: one fp64 multiplication
            const double max_nis = s_out.max_nis;
            mutual_best<BLOCK, 4, true>(sa, sb, steps, R, level_rule, fwd, bwd, VarianceGate<false>{s_var, max_nis, has_nis},
                                        VarianceGate<true>{s_var, max_nis, has_nis});
            __syncthreads();   // (every read of the masks and of s above comes before the writes below)
            int* matched_prev = s_out.matched_prev;
            int* matched_gap = s_out.matched_gap;
            double* fpos = s_out.fpos;
            double* velocity = s_out.velocity;
            double* cov = s_out.cov;
            const double q = s_out.q, r = s_out.r;
            for (int a = tid; a < ca; a += BLOCK) {
                const int b = fwd[a];
                if (b >= 0 && bwd[b] == a) {   // (fwd[a] >= 0 only where a had no predecessor; bwd[b] == a only where b had no successor)
                    const size_t row = (size_t)(v0 + a);
                    matched_prev[row] = b;
                    matched_gap[row] = k;
                    gap_a[a] = k;
                    succ_ws[brow + b] = 1;
                    double x[7] = {sb.pos[2 * (size_t)b], sb.pos[2 * (size_t)b + 1], sb.vel[2 * (size_t)b], sb.vel[2 * (size_t)b + 1],
                                   bcov[3 * (size_t)b], bcov[3 * (size_t)b + 1], bcov[3 * (size_t)b + 2]};
                    const int age_b = bage[b];
                    const double nis = cv_kalman_step(x, apos[2 * (size_t)a], apos[2 * (size_t)a + 1], steps, q, r);
                    fpos[2 * row] = x[0], fpos[2 * row + 1] = x[1];
                    velocity[2 * row] = x[2], velocity[2 * row + 1] = x[3];
                    cov[3 * row] = x[4], cov[3 * row + 1] = x[5], cov[3 * row + 2] = x[6];
                    s_out.nis[row] = nis;
                    s_out.age[row] = age_b + 1;
                }
            }
            __syncthreads();   // (the next level, and the next frame, read what this one wrote)
        }
        number_fresh(gap_a, ca, fwd, &s_fresh);   // the clusters without a predecessor, numbered in rank order
        __syncthreads();
        const int* matched_prev = s_out.matched_prev;
        long long* cluster_track = s_out.cluster_track;
        const char* state_in = s_out.state_in;
        const double r = s_out.r, vel_var = s_out.vel_var;
        for (int a = tid; a < ca; a += BLOCK) {
            const int k = gap_a[a];
            long long id;
            if (k < 0) {   // a birth: (z, 0, 0, r, 0, vel_var), age 0, nis 0 (velocity and nis are zero from launch 1)
                const size_t row = (size_t)(v0 + a);
                id = next_id + fwd[a];
                s_out.fpos[2 * row] = apos[2 * (size_t)a], s_out.fpos[2 * row + 1] = apos[2 * (size_t)a + 1];
                s_out.cov[3 * row] = r, s_out.cov[3 * row + 2] = vel_var;
                s_out.age[row] = 0;
            } else {   // (a level wrote a match only into a usable earlier frame, whose ids are final)
                const int m = matched_prev[v0 + a], tp = t - 1 - k;
                id = tp >= 0 ? cluster_track[node_ptr[tp] + m]
                              : StateView(state_in, s_off[HN], R, kStateKalman).track[s_off[HN + tp] + m];
            }
            cluster_track[v0 + a] = id;
        }
        for (int c = ca + tid; c < n; c += BLOCK) cluster_track[v0 + c] = -1;
        next_id += s_fresh;
        __syncthreads();   // (s_fresh, fwd and gap_a are the next frame's to write; its levels read this frame's ids and filtered states)
    }
    if (tid == 0) *s_out.next_id = next_id;
}

// ---- launch 3: node tracks, the new state ---------------------------------------------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void kalman_finish_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                              const int* __restrict__ rank, const float* __restrict__ emb, int R, int G,
                                                              const double* __restrict__ fpos, const double* __restrict__ velocity,
                                                              const double* __restrict__ cov, const int* __restrict__ age,
                                                              const long long* __restrict__ cluster_track, const int* __restrict__ succ_ws,
                                                              const char* __restrict__ state_in, GapFrames in, char* __restrict__ state_out,
                                                              GapFrames out, int P_lds, long long* __restrict__ node_track) {
    const int tid = threadIdx.x;
    const int S = in.off[in.n];
    const StateView ov(state_out, out.off[out.n], R, kStateKalman);   // (next_id, at offset 0 of its header, is the walk's to write)
    const int first_kept = G - out.n;   // the batch frame that becomes slot 0 of the new state (negative: history frames stay)

    if ((int)blockIdx.x >= G) {   // a history frame that stays: slot j of the new state is frame f of the old one
        const int j = (int)blockIdx.x - G;
        keep_slot<BLOCK, true>(ov, out, j, state_in, in, in.n + first_kept + j, R, kStateKalman, succ_ws, P_lds);
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
    write_slot<BLOCK, true>(ov, j, orow, cs, R, fpos + 2 * (size_t)v0, velocity + 2 * (size_t)v0, cluster_track + v0, succ_ws + S + v0,
                      emb + (size_t)v0 * R, cov + 3 * (size_t)v0, age + v0);
}

}  // namespace gnncca

extern "C" {

size_t gnncca_link_kalman_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim) {
    if (capacity_rows < 0 || reid_dim < 0 || n_frames_kept < 0 || n_frames_kept > gnncca::kGapMaxFrames) return 0;
    return gnncca::round256(gnncca::hist_succ_off(capacity_rows, reid_dim, gnncca::kStateKalman) + 2 * (size_t)capacity_rows * sizeof(int32_t));
}

size_t gnncca_link_kalman_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows) {
    if (n_nodes < 0 || n_frames < 0 || state_rows < 0) return 0;
    return gnncca::round256(((size_t)state_rows + (size_t)n_nodes) * sizeof(int32_t));   // successor flags [S + N]
}

int gnncca_link_frames_kalman(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                              int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                              int32_t has_max_cos, double max_cos, int32_t max_gap, double q, double r, double vel_var, int32_t has_max_nis,
                              double max_nis, const void* state_in, const int32_t* state_in_frame_rows, int32_t state_in_frames,
                              void* state_out, const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track,
                              int64_t* node_track, int32_t* matched_prev, int32_t* matched_gap, double* out_pos, double* out_vel,
                              double* out_cov, double* out_nis, int32_t* out_age, void* workspace, size_t workspace_bytes,
                              gnncca_stream_t stream, const double* frame_time_dev, double max_dt) {
    using namespace gnncca;
    const double inf = __builtin_inf();
    if (!(q >= 0.0) || !(q < inf) || !(r > 0.0) || !(r < inf) || !(vel_var > 0.0) || !(vel_var < inf)) return GNNCCA_ERR_INVALID_ARG;
    if (has_max_nis != 0 && has_max_nis != 1) return GNNCCA_ERR_INVALID_ARG;
    if (has_max_nis && (!(max_nis > 0.0) || !(max_nis < inf))) return GNNCCA_ERR_INVALID_ARG;
    if (frame_time_dev && (!(max_dt > 0.0) || !(max_dt < inf))) return GNNCCA_ERR_INVALID_ARG;
    HistoryPlan p;
    const int rc = plan_history(n_nodes, n_frames, reid_dim, max_frame_nodes, max_step, lam, has_max_cos, max_cos, max_gap, 0, state_in,
                                state_in_frame_rows, state_in_frames, state_out, state_out_frame_rows, state_out_frames, node_ptr_dev, count, emb,
                                rank && pos && cluster_track && node_track && matched_prev && matched_gap && out_pos && out_vel && out_cov &&
                                    out_nis && out_age,
                                workspace, workspace_bytes, gnncca_link_kalman_workspace_bytes, p);
    if (rc != GNNCCA_OK || p.nothing) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* succ_ws = static_cast<int*>(workspace);
    char* sout = static_cast<char*>(state_out);
    const int nis_lds = has_max_nis ? p.P : 0;
    const size_t lds = (size_t)3 * p.P * sizeof(int) + (size_t)nis_lds * sizeof(double);
    constexpr size_t kMaxLds = (size_t)kTrackMaxNodes * (3 * sizeof(int) + sizeof(double));
    static_assert(kMaxLds + 1024 <= 160 * 1024, "the walk's LDS arrays fit one CU");
    if (lds > 64 * 1024) {
        if (frame_time_dev) HIP_TRY((lds_opt_in<kalman_walk_kernel<kMotionWalkBlock, TimedKalmanOutputs>>(kMaxLds)));
        else HIP_TRY((lds_opt_in<kalman_walk_kernel<kMotionWalkBlock, KalmanOutputs>>(kMaxLds)));
    }
    const int* in_succ = p.sin ? reinterpret_cast<const int*>(p.sin + hist_succ_off(p.S, p.R, kStateKalman)) : nullptr;
    hipLaunchKernelGGL(kalman_init_kernel, dim3(p.init_blocks), dim3(256), 0, st, in_succ, p.S, (int)n_nodes, succ_ws, matched_prev, matched_gap,
                       out_pos, out_vel, out_cov, out_nis, out_age);
    HIP_TRY(hipGetLastError());
    KalmanOutputs outs;
    static_cast<WalkOutputs&>(outs) = WalkOutputs{matched_prev, matched_gap, out_vel, reinterpret_cast<long long*>(cluster_track),
                                                  &reinterpret_cast<GapHeader*>(sout)->next_id, succ_ws, p.sin, lam, max_cos, emb};
    outs.fpos = out_pos, outs.cov = out_cov, outs.nis = out_nis, outs.age = out_age;
    outs.q = q, outs.r = r, outs.vel_var = vel_var, outs.max_nis = max_nis, outs.has_nis = has_max_nis;
    if (!frame_time_dev) {
        hipLaunchKernelGGL((kalman_walk_kernel<kMotionWalkBlock, KalmanOutputs>), dim3(1), dim3(kMotionWalkBlock), lds, st, node_ptr_dev,
                           (int)n_nodes, (int)n_frames, count, pos, p.R, p.rule, (int)max_gap, p.in, p.P, nis_lds, outs);
    } else {
        TimedKalmanOutputs timed;
        static_cast<KalmanOutputs&>(timed) = outs;
        timed.frame_time = frame_time_dev, timed.max_dt = max_dt;
        hipLaunchKernelGGL((kalman_walk_kernel<kMotionWalkBlock, TimedKalmanOutputs>), dim3(1), dim3(kMotionWalkBlock), lds, st, node_ptr_dev,
                           (int)n_nodes, (int)n_frames, count, pos, p.R, p.rule, (int)max_gap, p.in, p.P, nis_lds, timed);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((kalman_finish_kernel<256>), dim3((unsigned)(n_frames + p.carried)), dim3(256), 0, st, node_ptr_dev, (int)n_nodes, count,
                       rank, emb, p.R, (int)n_frames, out_pos, out_vel, out_cov, out_age, reinterpret_cast<const long long*>(cluster_track),
                       succ_ws, p.sin, p.in, sout, p.out, p.P, reinterpret_cast<long long*>(node_track));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
