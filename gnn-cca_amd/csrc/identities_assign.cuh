// identities_assign.cuh -- matching = 1 of gnncca_link_frames_gap_ex (FrameLinker(matching='optimal')), included by identities.hip after
// identities_gap.cuh: the second form of the level kernel.  Levels, gates, masks, the init / scan / ids kernels and the carried state are
// identities_gap.cuh's, the cost of a pair is link_common.cuh's pair_rule (the one the mutual-best search calls); only the choice of pairs inside a workgroup's (A, B) table differs: the one-to-one set of
// admissible pairs that minimises the sum of cost - miss_cost (leaving a pair's clusters unlinked is worth 0), found by shortest
// augmenting paths in an order that is part of the contract (include/gnncca_mpn.h has it in full; tests/tracking_assign_oracle.py
// restates it as loops and the kernel matches it bit for bit: every fp64 operation is elementwise, the file has `fp contract(off)`, and
// the one reduction is a lexicographic (value, column) minimum).
// One workgroup per frame, as in gap_level_kernel:
//   1. wave 0 ranks the clusters of frame t without a predecessor (A, n of them), wave 1 those of frame t - 1 - k without a successor
//      (B, m of them): ballot scans into LDS;
//   2. all waves build W [n][m] in LDS, a wave per row, its lanes the columns (through ib[]), pair_rule's whole-wave cosine: W = cost -
//      miss_cost for an admissible pair whose cost is not NaN, +inf otherwise ((inf - u) - v = inf is never < minv: not an edge);
//   3. wave 0 alone inserts the rows 0 .. n - 1 over m + n columns (column m + i: row i stays unlinked, 0 for row i, +inf for the
//      others), columns over lanes, the duals and the tree in LDS, the minimum by shuffles: no workgroup barrier inside the loop.  LDS
//      operations of one wave complete in order, so a lane reads what another lane of its wave wrote in an earlier instruction;
//      wave_sync() keeps the compiler from moving an access across such a hand-over.
//      Every loop is bounded by numbers fixed at launch: n rows, at most min(n, m) + 1 tree steps per row (a step that does not end the
//      row's search marks a matched REAL column, of which there are at most min(n - 1, m): an unlinked column is reached only from its
//      own row and only while it is free), and a path of at most as many columns to flip;
//   4. wave 0 writes the predecessor records and successor flags; then, at the last level, the numbering of gap_level_kernel
//      (number_fresh).
// LDS, from numbers the host knows (P = the power of two >= the largest frame of the batch and of the history, >= 64):  W 8 P^2, v and
// minv 2 x 16 P, u 8 P, p / way / used 3 x 8 P, A / B ranks 2 x 4 P, the numbering's flags 4 P, two counts = 8 P^2 + 76 P + 16 bytes:
// 37,648 at P = 64, 140,816 of the 163,840 at P = 128 = GNNCCA_TRACK_MAX_OPTIMAL_FRAME_NODES.  Rows of W are P * 8 bytes and every
// access of a wave is to consecutive doubles of one row: conflict-free 8-byte accesses, all carve offsets multiples of 16.
#pragma once

namespace gnncca {

__host__ __device__ inline size_t assign_lds_bytes(int P) { return (size_t)8 * P * P + (size_t)76 * P + 16; }

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (no instruction: the compiler keeps LDS accesses on their side of it)
    __builtin_amdgcn_wave_barrier();
}

// `rule.max_step` is the gate of THIS level, as in gap_level_kernel -- and with time stamps (frame_time != nullptr) the caller's max_step,
// the gate max_step * dt worked out here and a table outside (0, max_dt] skipped whole, as there.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void gap_level_assign_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                                 const double* __restrict__ pos, const float* __restrict__ emb, int R,
                                                                 LinkRule rule, double miss_cost, int level, int last_level,
                                                                 const char* __restrict__ state_in, GapFrames in, int P_lds, int* succ_ws,
                                                                 int* matched_prev, int* matched_gap, int* __restrict__ new_rank_ws,
                                                                 int* __restrict__ n_new_ws, const double* __restrict__ frame_time,
                                                                 double max_dt) {
    extern __shared__ __attribute__((aligned(16))) char s_assign[];
    const int P = P_lds;
    double* W = reinterpret_cast<double*>(s_assign);   // [P][P]: row i of A, column j of B
    double* v = W + (size_t)P * P;                     // [2 P] column duals
    double* minv = v + 2 * P;                          // [2 P]
    double* u = minv + 2 * P;                          // [P] row duals
    int* p = reinterpret_cast<int*>(u + P);            // [2 P] the row of a column, -1: free
    int* way = p + 2 * P;                              // [2 P] the column before this one on the path
    int* used = way + 2 * P;                           // [2 P]
    int* ia = used + 2 * P;                            // [P] rank of row i within frame t
    int* ib = ia + P;                                  // [P] rank of column j within frame t - 1 - k
    int* fwd = ib + P;                                 // [P] the frame's final gaps (last level)
    int* cnt = fwd + P;                                // n, m
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int v0, nn;
    if (!frame_range(node_ptr, g, N_all, v0, nn)) {
        if (last_level && tid == 0) n_new_ws[g] = 0;
        return;
    }
    const int ca = usable_count(count, g, nn, P);
    int brow;   // the combined row of B's rank 0
    const LinkSide sb = side_b(g - 1 - level, node_ptr, N_all, count, pos, nullptr, emb, R, state_in, in.n, in.off, in.off[in.n], false, P, brow);
    int cb = sb.n;
    if (frame_time && ca > 0 && cb > 0) {   // (uniform; side B exists, so in.n + g - 1 - level >= 0)
        double dt;
        if (level_dt(frame_time, in.n + g, in.n + g - 1 - level, max_dt, dt)) rule.max_step = rule.max_step * dt;
        else cb = 0;
    }
    const double* ppos = sb.pos;
    const float* pemb = sb.emb;
    if (ca > 0 && cb > 0) {   // (uniform; ca, cb <= P)
        if (wave == 0) {
            const int k = wave_compact(matched_gap + v0, -1, ca, ia);
            if (lane == 0) cnt[0] = k;
        } else if (wave == 1) {
            const int k = wave_compact(succ_ws + brow, 0, cb, ib);
            if (lane == 0) cnt[1] = k;
        }
        __syncthreads();   // (every read of the masks above comes before the writes of step 4)
        const int n = cnt[0], m = cnt[1];
        if (n > 0 && m > 0) {   // (uniform)
            const double* cpos = pos + 2 * (size_t)v0;
            const float* cemb = emb + (size_t)v0 * R;
            const double inf = __builtin_inf();
            for (int i = wave; i < n; i += BLOCK / 64) {   // ---- 2. the table
                const int a = ia[i];
                const double rx = cpos[2 * (size_t)a], ry = cpos[2 * (size_t)a + 1];
                for (int base = 0; base < m; base += 64) {
                    const int j = base + lane;
                    double cx = 0.0, cy = 0.0, w = inf;
                    if (j < m) cx = ppos[2 * (size_t)ib[j]], cy = ppos[2 * (size_t)ib[j] + 1];
                    pair_rule<1>(j < m, rx, ry, cx, cy, cemb + (size_t)a * R, [&](int jj) { return pemb + (size_t)ib[base + jj] * R; }, R, rule,
                                 [&](double cost) {
                                     if (cost == cost) w = cost - miss_cost;   // (a NaN cost: not admissible)
                                 });
                    if (j < m) W[(size_t)i * P + j] = w;
                }
            }
            __syncthreads();
            if (wave == 0) {   // ---- 3. the rows, one after the other
                const int nc = m + n, bound = (n < m ? n : m) + 1;
                for (int j = lane; j < nc; j += 64) v[j] = 0.0, p[j] = -1;
                for (int i = lane; i < n; i += 64) u[i] = 0.0;
                for (int i = 0; i < n; ++i) {
                    for (int j = lane; j < nc; j += 64) minv[j] = inf, used[j] = 0, way[j] = -1;
                    wave_sync();
                    int i0 = i, j0 = -1, j1 = -1;
                    bool found = false;
                    for (int step = 0; step < bound; ++step) {
                        const double ui = u[i0];
                        const double* row = W + (size_t)i0 * P;
                        double best = inf;
                        int bj = INT_MAX;
                        for (int j = lane; j < nc; j += 64) {
                            if (used[j]) continue;
                            const double w = j < m ? row[j] : (j - m == i0 ? 0.0 : inf);
                            const double cur = (w - ui) - v[j];
                            double mv = minv[j];
                            if (cur < mv) {
                                mv = cur;
                                minv[j] = cur;
                                way[j] = j0;
                            }
                            if (mv < best) best = mv, bj = j;   // (a lane's columns ascend: the smaller one stays on a tie)
                        }
                        const ValueIndex least = wave_min_lex(best, bj);   // of (minv, column)
                        if (least.i == INT_MAX) break;   // (uniform; cannot be: row i0's own unlinked column is free)
                        const double delta = least.v;
                        j1 = least.i;
                        wave_sync();
                        for (int j = lane; j < nc; j += 64) {
                            if (used[j]) {
                                u[p[j]] += delta;   // (p is one-to-one on the used columns, and none of them holds row i)
                                v[j] -= delta;
                            } else {
                                minv[j] -= delta;
                            }
                        }
                        if (lane == 0) {
                            u[i] += delta;
                            used[j1] = 1;
                        }
                        wave_sync();
                        const int pj = p[j1];
                        if (pj < 0) {
                            found = true;
                            break;
                        }
                        i0 = pj;
                        j0 = j1;
                    }
                    if (found) {   // (uniform) flip the path back along way: every lane the same walk, the same stores
                        int j = j1;
                        for (int q = 0; q < bound; ++q) {
                            const int jp = way[j];
                            const int r = jp < 0 ? i : p[jp];
                            wave_sync();
                            p[j] = r;
                            wave_sync();
                            if (jp < 0) break;
                            j = jp;
                        }
                    }
                    wave_sync();
                }
                for (int j = lane; j < m; j += 64) {   // ---- 4. the pairs
                    const int r = p[j];
                    if (r >= 0 && r < n) {
                        const int a = ia[r], b = ib[j];
                        matched_prev[v0 + a] = b;
                        matched_gap[v0 + a] = level;
                        succ_ws[brow + b] = 1;
                    }
                }
            }
        }
    }
    if (!last_level) return;
    __syncthreads();   // (wave 0's records are visible to the workgroup)
    for (int a = tid; a < ca; a += BLOCK) fwd[a] = matched_gap[v0 + a];
    __syncthreads();
    number_fresh(fwd, ca, new_rank_ws + v0, n_new_ws + g);   // the clusters without a predecessor, numbered in rank order
}

static int assign_level_launch(hipStream_t st, int n_frames, int P, const int* node_ptr_dev, int n_nodes, const int* count, const double* pos,
                               const float* emb, int R, const LinkRule& level_rule, int level, int last_level, const char* sin,
                               const GapFrames& in, int* succ_ws, int* matched_prev, int* matched_gap, int* new_rank_ws, int* n_new_ws,
                               double miss_cost, const double* frame_time, double max_dt) {
    if (P > kTrackMaxOptimalNodes) return GNNCCA_ERR_INVALID_ARG;   // (the entry refused such a frame already)
    HIP_TRY(lds_opt_in<gap_level_assign_kernel<256>>(assign_lds_bytes(kTrackMaxOptimalNodes)));
    hipLaunchKernelGGL((gap_level_assign_kernel<256>), dim3((unsigned)n_frames), dim3(256), assign_lds_bytes(P), st, node_ptr_dev, n_nodes, count,
                       pos, emb, R, level_rule, miss_cost, level, last_level, sin, in, P, succ_ws, matched_prev, matched_gap, new_rank_ws,
                       n_new_ws, frame_time, max_dt);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // namespace gnncca

extern "C" {

int gnncca_link_frames_gap_ex(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                              int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                              int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t matching, double miss_cost, const void* state_in,
                              const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                              const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                              int32_t* matched_prev, int32_t* matched_gap, void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    if (matching != 0 && matching != 1) return GNNCCA_ERR_INVALID_ARG;
    if (!(miss_cost > 0.0) || !(miss_cost < __builtin_inf())) return GNNCCA_ERR_INVALID_ARG;
    return gnncca::link_frames_gap_run(node_ptr_dev, count, rank, pos, emb, reid_dim, n_nodes, n_frames, max_frame_nodes, max_step, lam, has_max_cos,
                                       max_cos, max_gap, matching, miss_cost, state_in, state_in_frame_rows, state_in_frames, state_out,
                                       state_out_frame_rows, state_out_frames, cluster_track, node_track, matched_prev, matched_gap, workspace,
                                       workspace_bytes, stream, nullptr, 0.0);
}

/* gnncca_link_frames_gap_ex with a time stamp per frame (include/gnncca_mpn.h has the rule): the same run, the gate worked out per
 * (frame, level) on the device from frame_time_dev, fp64 [state_in_frames + n_frames]. */
int gnncca_link_frames_gap_timed(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                                 int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                                 int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t matching, double miss_cost, const void* state_in,
                                 const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                                 const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                                 int32_t* matched_prev, int32_t* matched_gap, void* workspace, size_t workspace_bytes, gnncca_stream_t stream,
                                 const double* frame_time_dev, double max_dt) {
    if (matching != 0 && matching != 1) return GNNCCA_ERR_INVALID_ARG;
    if (!(miss_cost > 0.0) || !(miss_cost < __builtin_inf())) return GNNCCA_ERR_INVALID_ARG;
    if (!(max_dt > 0.0) || !(max_dt < __builtin_inf())) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames > 0 && !frame_time_dev) return GNNCCA_ERR_INVALID_ARG;
    return gnncca::link_frames_gap_run(node_ptr_dev, count, rank, pos, emb, reid_dim, n_nodes, n_frames, max_frame_nodes, max_step, lam, has_max_cos,
                                       max_cos, max_gap, matching, miss_cost, state_in, state_in_frame_rows, state_in_frames, state_out,
                                       state_out_frame_rows, state_out_frames, cluster_track, node_track, matched_prev, matched_gap, workspace,
                                       workspace_bytes, stream, frame_time_dev, max_dt);
}

}  // extern "C"
