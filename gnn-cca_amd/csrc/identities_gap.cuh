// identities_gap.cuh -- gap-tolerant linking (gnncca_link_frames_gap), included at the end of identities.hip after link_common.cuh, which
// has what this file shares with the other linkers: the pair rule and the partner search (instantiated here with masks, one load per side
// in flight), side_b, the numbering, the history state (StateView, write_slot, keep_slot), link_init_kernel and plan_history.
//
// The rule (include/gnncca_mpn.h has it in full): levels k = 0 .. M one after the other; at level k the clusters of frame t that have no
// predecessor yet (A) meet the clusters of frame t - 1 - k that have no successor yet (B) under the gate max_step * (k + 1), mutual best
// as in link_match_kernel.  Every cluster is in exactly one (A-frame, B-frame) pair per level, so the workgroup of frame t owns all it
// writes -- the predecessor record of frame t, the successor flags of frame t - 1 - k -- and a level needs no atomics.
// Launches, M + 4 of them, fixed per max_gap:
//   1. link_init_kernel: predecessor record (matched_prev, matched_gap) of the N batch rows = none; successor flags of the S history rows
//      copied from state_in (which is never written), of the N batch rows cleared.  The flags live in the workspace as one array over
//      the COMBINED rows: history row i is i, batch row v is S + v.
//   2. gap_level_kernel, once per level, grid = G: fwd / bwd in LDS, mutual_best over the masked sides; the last level also numbers the
//      frame's clusters that are still without a predecessor (number_fresh), once.
//   3. link_scan_kernel, as it is.
//   4. gap_ids_kernel, grid = G + the history frames carried along: ids along the predecessor chains, node tracks, and the new state --
//      a batch frame among the newest M + 1 writes its own slot (write_slot), an extra workgroup copies a history frame that stays
//      (keep_slot).
// The carried state is the history state of link_common.cuh without velocities.
#pragma once

namespace gnncca {

// ---- launch 2: one level ----------------------------------------------------------------------------------------------------------------
// `rule.max_step` is the gate of THIS level, max_step * (k + 1), multiplied once on the host in fp64 -- unless the call has time stamps
// (frame_time != nullptr, fp64 [history frames + G]): then it is the caller's max_step, dt = T[t] - T[t - 1 - k] is worked out here, the
// gate is max_step * dt (one fp64 multiplication), and a table with !(dt > 0 && dt <= max_dt) is skipped whole.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void gap_level_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                          const double* __restrict__ pos, const float* __restrict__ emb, int R, LinkRule rule,
                                                          int level, int last_level, const char* __restrict__ state_in, GapFrames in, int P_lds,
                                                          int* succ_ws, int* matched_prev, int* matched_gap, int* __restrict__ new_rank_ws,
                                                          int* __restrict__ n_new_ws, const double* __restrict__ frame_time, double max_dt) {
    extern __shared__ int s_dyn[];
    int* fwd = s_dyn;           // [a] -> b; at the last level then the frame's final gaps
    int* bwd = s_dyn + P_lds;   // [b] -> a
    const int g = blockIdx.x, tid = threadIdx.x;
    int v0, n;
    if (!frame_range(node_ptr, g, N_all, v0, n)) {
        if (last_level && tid == 0) n_new_ws[g] = 0;
        return;
    }
    const int ca = usable_count(count, g, n, P_lds);
    int brow;   // the combined row of B's rank 0
    LinkSide sb = side_b(g - 1 - level, node_ptr, N_all, count, pos, nullptr, emb, R, state_in, in.n, in.off, in.off[in.n], false, P_lds, brow);
    if (frame_time && ca > 0 && sb.n > 0) {   // (uniform; side B exists, so in.n + g - 1 - level >= 0)
        double dt;
        if (level_dt(frame_time, in.n + g, in.n + g - 1 - level, max_dt, dt)) rule.max_step = rule.max_step * dt;
        else sb.n = 0;
    }
    if (ca > 0 && sb.n > 0) {   // (uniform)
        const LinkSide sa{pos + 2 * (size_t)v0, nullptr, emb + (size_t)v0 * R, matched_gap + v0, -1, ca};
        sb.mask = succ_ws + brow, sb.free = 0;
        mutual_best<BLOCK, 1, true>(sa, sb, 1.0, R, rule, fwd, bwd);
        __syncthreads();   // (every read of the masks above comes before the writes below)
        for (int a = tid; a < ca; a += BLOCK) {
            const int b = fwd[a];
            if (b >= 0 && bwd[b] == a) {   // (fwd[a] >= 0 only where a had no predecessor; bwd[b] == a only where b had no successor)
                matched_prev[v0 + a] = b;
                matched_gap[v0 + a] = level;
                succ_ws[brow + b] = 1;
            }
        }
    }
    if (!last_level) return;
    __syncthreads();
    for (int a = tid; a < ca; a += BLOCK) fwd[a] = matched_gap[v0 + a];   // each thread reads what it wrote itself (or an earlier launch wrote)
    __syncthreads();
    number_fresh(fwd, ca, new_rank_ws + v0, n_new_ws + g);   // the clusters without a predecessor, numbered in rank order
}

// ---- launch 4: ids along the chains, node tracks, the new state ---------------------------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void gap_ids_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                        const int* __restrict__ rank, const double* __restrict__ pos,
                                                        const float* __restrict__ emb, int R, int G, const int* __restrict__ matched_prev,
                                                        const int* __restrict__ matched_gap, const int* __restrict__ new_rank_ws,
                                                        const int* __restrict__ base_ws, const int* __restrict__ succ_ws,
                                                        const char* __restrict__ state_in, GapFrames in, char* __restrict__ state_out,
                                                        GapFrames out, int P_lds, long long* __restrict__ cluster_track,
                                                        long long* __restrict__ node_track) {
    extern __shared__ long long s_track[];
    const int tid = threadIdx.x;
    const int S = in.off[in.n];
    const long long next0 = state_in ? reinterpret_cast<const GapHeader*>(state_in)->next_id : 0;
    const long long* in_track = state_in ? StateView(state_in, S, R, false).track : nullptr;
    const StateView ov(state_out, out.off[out.n], R, false);
    const int first_kept = G - out.n;   // the batch frame that becomes slot 0 of the new state (negative: history frames stay)

    if ((int)blockIdx.x >= G) {   // a history frame that stays: slot j of the new state is frame f of the old one
        const int j = (int)blockIdx.x - G;
        keep_slot<BLOCK>(ov, out, j, state_in, in, in.n + first_kept + j, R, false, succ_ws, P_lds);
        return;
    }

    const int g = blockIdx.x;
    int v0, n;
    const bool ok = frame_range(node_ptr, g, N_all, v0, n);
    const int ca = ok ? usable_count(count, g, n, P_lds) : 0;
    for (int c = tid; c < ca; c += BLOCK) {
        // back along the predecessor record to the head of the chain (a level wrote a match only into a usable earlier frame)
        int t = g, cc = c;
        long long id;
        for (;;) {
            const int row = node_ptr[t] + cc;
            const int m = matched_prev[row];
            if (m < 0) {
                id = next0 + base_ws[t] + new_rank_ws[row];
                break;
            }
            t -= 1 + matched_gap[row];
            if (t < 0) {
                id = in_track[in.off[in.n + t] + m];
                break;
            }
            cc = m;
        }
        s_track[c] = id;
        cluster_track[v0 + c] = id;
    }
    for (int c = ca + tid; c < n; c += BLOCK) cluster_track[v0 + c] = -1;
    __syncthreads();
    write_node_tracks<BLOCK>(rank + v0, n, ca, s_track, node_track + v0);
    if (g == G - 1 && tid == 0) {
        ov.head->next_id = next0 + base_ws[G];
        ov.head->n_frames = out.n;
        ov.head->reid_dim = R;
    }
    if (g < first_kept) return;
    const int j = g - first_kept, orow = out.off[j];
    const int cs = ca <= out.off[j + 1] - orow ? ca : 0;   // (a frame with more clusters than its slot has rows is carried as empty)
    write_slot<BLOCK>(ov, j, orow, cs, R, pos + 2 * (size_t)v0, nullptr, s_track, succ_ws + S + v0, emb + (size_t)v0 * R);
}

}  // namespace gnncca

extern "C" {

size_t gnncca_link_gap_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim) {
    if (capacity_rows < 0 || reid_dim < 0 || n_frames_kept < 0 || n_frames_kept > gnncca::kGapMaxFrames) return 0;
    return gnncca::round256(gnncca::hist_succ_off(capacity_rows, reid_dim, false) + (size_t)capacity_rows * sizeof(int32_t));
}

size_t gnncca_link_gap_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows) {
    if (n_nodes < 0 || n_frames < 0 || state_rows < 0) return 0;
    // successor flags [S + N], rank among the frame's clusters without a predecessor [N], their number per frame [G], its prefix sum [G + 1]
    return gnncca::round256(((size_t)state_rows + 2 * (size_t)n_nodes + 2 * (size_t)n_frames + 1) * sizeof(int32_t));
}

}  // extern "C"

namespace gnncca {

// the level launch of matching = 1 (identities_assign.cuh, included after this file)
static int assign_level_launch(hipStream_t st, int n_frames, int P, const int* node_ptr_dev, int n_nodes, const int* count, const double* pos,
                               const float* emb, int R, const LinkRule& level_rule, int level, int last_level, const char* sin,
                               const GapFrames& in, int* succ_ws, int* matched_prev, int* matched_gap, int* new_rank_ws, int* n_new_ws,
                               double miss_cost, const double* frame_time, double max_dt);

// gnncca_link_frames_gap (matching 0), gnncca_link_frames_gap_ex and gnncca_link_frames_gap_timed: one body, the form of the level kernel
// chosen by `matching`; frame_time nullptr (and max_dt unused) from the untimed entries, which multiply the gate here, on the host
static int link_frames_gap_run(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                               int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                               int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t matching, double miss_cost, const void* state_in,
                               const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                               const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                               int32_t* matched_prev, int32_t* matched_gap, void* workspace, size_t workspace_bytes, gnncca_stream_t stream,
                               const double* frame_time, double max_dt) {
    HistoryPlan p;
    const int rc = plan_history(n_nodes, n_frames, reid_dim, max_frame_nodes, max_step, lam, has_max_cos, max_cos, max_gap, matching, state_in,
                                state_in_frame_rows, state_in_frames, state_out, state_out_frame_rows, state_out_frames, node_ptr_dev, count, emb,
                                rank && pos && cluster_track && node_track && matched_prev && matched_gap, workspace, workspace_bytes,
                                gnncca_link_gap_workspace_bytes, p);
    if (rc != GNNCCA_OK || p.nothing) return rc;
    const GapFrames& in = p.in;
    const int R = p.R, S = p.S, P = p.P;
    const LinkRule& rule = p.rule;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* succ_ws = static_cast<int*>(workspace);
    int* new_rank_ws = succ_ws + S + n_nodes;
    int* n_new_ws = new_rank_ws + n_nodes;
    int* base_ws = n_new_ws + n_frames;
    const char* sin = p.sin;
    launch_link_init(st, p, false, n_nodes, succ_ws, matched_prev, matched_gap, nullptr);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k <= max_gap; ++k) {
        LinkRule level_rule = rule;
        if (!frame_time) level_rule.max_step = max_step * (double)(k + 1);   // gate_k: one fp64 multiplication (timed: max_step * dt, in the kernel)
        if (matching) {
            const int rc = assign_level_launch(st, (int)n_frames, P, node_ptr_dev, (int)n_nodes, count, pos, emb, R, level_rule, k, (int)(k == max_gap),
                                               sin, in, succ_ws, matched_prev, matched_gap, new_rank_ws, n_new_ws, miss_cost, frame_time, max_dt);
            if (rc != GNNCCA_OK) return rc;
            continue;
        }
        hipLaunchKernelGGL((gap_level_kernel<256>), dim3((unsigned)n_frames), dim3(256), (size_t)2 * P * sizeof(int), st, node_ptr_dev, (int)n_nodes,
                           count, pos, emb, R, level_rule, k, (int)(k == max_gap), sin, in, P, succ_ws, matched_prev, matched_gap, new_rank_ws,
                           n_new_ws, frame_time, max_dt);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(64), 0, st, n_new_ws, (int)n_frames, base_ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((gap_ids_kernel<256>), dim3((unsigned)(n_frames + p.carried)), dim3(256), (size_t)P * sizeof(long long), st, node_ptr_dev,
                       (int)n_nodes, count, rank, pos, emb, R, (int)n_frames, matched_prev, matched_gap, new_rank_ws, base_ws, succ_ws, sin, in,
                       static_cast<char*>(state_out), p.out, P, reinterpret_cast<long long*>(cluster_track),
                       reinterpret_cast<long long*>(node_track));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // namespace gnncca

extern "C" {

int gnncca_link_frames_gap(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                           int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                           int32_t has_max_cos, double max_cos, int32_t max_gap, const void* state_in, const int32_t* state_in_frame_rows,
                           int32_t state_in_frames, void* state_out, const int32_t* state_out_frame_rows, int32_t state_out_frames,
                           int64_t* cluster_track, int64_t* node_track, int32_t* matched_prev, int32_t* matched_gap, void* workspace,
                           size_t workspace_bytes, gnncca_stream_t stream) {
    return gnncca::link_frames_gap_run(node_ptr_dev, count, rank, pos, emb, reid_dim, n_nodes, n_frames, max_frame_nodes, max_step, lam, has_max_cos,
                                       max_cos, max_gap, 0, 0.0, state_in, state_in_frame_rows, state_in_frames, state_out, state_out_frame_rows,
                                       state_out_frames, cluster_track, node_track, matched_prev, matched_gap, workspace, workspace_bytes, stream,
                                       nullptr, 0.0);
}

}  // extern "C"
