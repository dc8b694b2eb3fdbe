// identities_gap.cuh -- gap-tolerant linking (gnncca_link_frames_gap), included at the end of identities.hip: it shares LinkRule, frame_range,
// usable_count, the scan kernel and the file's `fp contract(off)`.  gnncca_link_frames and its kernels are not touched.
//
// The rule (include/gnncca_mpn.h has it in full): levels k = 0 .. M one after the other; at level k the clusters of frame t that have no
// predecessor yet (A) meet the clusters of frame t - 1 - k that have no successor yet (B) under the gate max_step * (k + 1), mutual best
// as in link_match_kernel.  Every cluster is in exactly one (A-frame, B-frame) pair per level, so the workgroup of frame t owns all it
// writes -- the predecessor record of frame t, the successor flags of frame t - 1 - k -- and a level needs no atomics.
// Launches, M + 4 of them, fixed per max_gap:
//   1. gap_init_kernel: predecessor record (matched_prev, matched_gap) of the N batch rows = none; successor flags of the S history rows
//      copied from state_in (which is never written), of the N batch rows cleared.  The flags live in the workspace as one array over
//      the COMBINED rows: history row i is i, batch row v is S + v.
//   2. gap_level_kernel, once per level, grid = G: fwd / bwd in LDS, best_partner_masked; the last level also numbers the frame's
//      clusters that are still without a predecessor (ballot scan), once.
//   3. link_scan_kernel, as it is.
//   4. gap_ids_kernel, grid = G + the history frames carried along: ids along the predecessor chains, node tracks, and the new state --
//      a batch frame among the newest M + 1 writes its own slot, an extra workgroup copies a history frame that stays.
// The carried state: GapHeader (64 bytes: next_id as an int64 at offset 0, the number of frames, reid_dim, the cluster count per frame),
// then for a total capacity of C rows: pos fp64 [C][2], track int64 [C], emb fp32 [C][R], succ int32 [C].  Frame f owns the rows
// off[f] .. off[f + 1], the running sum of the per-frame capacities the CALLER knows on the host (node counts bound cluster counts) and
// passes by value: nothing is read back to size anything.
#pragma once

namespace gnncca {

constexpr int kTrackMaxGap = GNNCCA_TRACK_MAX_GAP;
constexpr int kGapMaxFrames = kTrackMaxGap + 1;
constexpr int kTrackMaxOptimalNodes = GNNCCA_TRACK_MAX_OPTIMAL_FRAME_NODES;   // matching = 1: a frame pair's table lives in LDS

struct GapHeader {
    long long next_id;
    int n_frames;
    int reid_dim;
    int count[kGapMaxFrames];
    int pad[3];
};
static_assert(sizeof(GapHeader) == 64, "the gap state's arrays start at byte 64");

// the host-known row offsets of a state's frames: frame f owns rows off[f] .. off[f + 1] (off[n] = all rows)
struct GapFrames {
    int n;
    int off[kGapMaxFrames + 1];
};

__host__ __device__ inline size_t gap_pos_off() { return sizeof(GapHeader); }
__host__ __device__ inline size_t gap_track_off(long long cap) { return sizeof(GapHeader) + (size_t)cap * 16; }
__host__ __device__ inline size_t gap_emb_off(long long cap) { return sizeof(GapHeader) + (size_t)cap * 24; }
__host__ __device__ inline size_t gap_succ_off(long long cap, int R) { return gap_emb_off(cap) + (size_t)cap * (size_t)R * sizeof(float); }

// cluster count of history frame f if the state holds one that fits its rows (0 otherwise: such a frame links to nothing)
__device__ __forceinline__ int gap_hist_count(const char* __restrict__ state_in, const GapFrames& in, int f, int P_lds) {
    const int c = reinterpret_cast<const GapHeader*>(state_in)->count[f];
    const int cap = in.off[f + 1] - in.off[f];
    return (c >= 0 && c <= cap && c <= P_lds) ? c : 0;
}

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gap_init_kernel(const char* __restrict__ state_in, int S, int R, int N_all, int* __restrict__ succ_ws,
                                                       int* __restrict__ matched_prev, int* __restrict__ matched_gap) {
    const int* in_succ = state_in ? reinterpret_cast<const int*>(state_in + gap_succ_off(S, R)) : nullptr;
    const long long total = (long long)S + N_all;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (i < S) {
            succ_ws[i] = in_succ[i] != 0;
        } else {
            succ_ws[i] = 0;
            matched_prev[i - S] = -1;
            matched_gap[i - S] = -1;
        }
    }
}

// ---- launch 2: one level ----------------------------------------------------------------------------------------------------------------
// best_partner with masks: row r is skipped (out[r] = -1) unless rmask[r] == rfree, column c is no candidate unless cmask[c] == cfree.  The
// tie and lane order are best_partner's: the lexicographic (cost, index) minimum over ORIGINAL ranks, never over compacted positions.
template <int BLOCK>
__device__ void best_partner_masked(const double* __restrict__ rpos, const float* __restrict__ remb, const int* rmask, int rfree, int nr,
                                    const double* __restrict__ cpos, const float* __restrict__ cemb, const int* cmask, int cfree, int nc,
                                    int R, const LinkRule& rule, int* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nr; r += BLOCK / 64) {
        if (rmask[r] != rfree) {   // (uniform in the wave)
            if (lane == 0) out[r] = -1;
            continue;
        }
        const double rx = rpos[2 * (size_t)r], ry = rpos[2 * (size_t)r + 1];
        double best = __builtin_inf();
        int bi = INT_MAX;
        for (int base = 0; base < nc; base += 64) {
            const int c = base + lane;
            bool cand = false;
            double d = 0.0, dcos = 0.0;
            if (c < nc && cmask[c] == cfree) {
                const double dx = rx - cpos[2 * (size_t)c], dy = ry - cpos[2 * (size_t)c + 1];
                d = sqrt(dx * dx + dy * dy);
                cand = d <= rule.max_step;   // (rule.max_step holds the level's gate)
            }
            if (rule.need_emb) {
                unsigned long long todo = __ballot(cand);   // (uniform) the pairs inside the gate: the whole wave computes each cosine
                while (todo) {
                    const int j = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const float* er = remb + (size_t)r * R;
                    const float* ec = cemb + (size_t)(base + j) * R;
                    double dot = 0.0, na = 0.0, nb = 0.0;
                    for (int k = lane; k < R; k += 64) {
                        const double x = (double)er[k], y = (double)ec[k];
                        dot += x * y;
                        na += x * x;
                        nb += y * y;
                    }
                    dot = wave_sum_f64(dot);
                    na = wave_sum_f64(na);
                    nb = wave_sum_f64(nb);
                    const double v = (na == 0.0 || nb == 0.0) ? 1.0 : 1.0 - dot / (sqrt(na) * sqrt(nb));
                    if (lane == j) dcos = v;
                }
                if (rule.has_max_cos) cand = cand && dcos <= rule.max_cos;
            }
            if (cand) {
                const double cost = rule.need_emb ? d / rule.max_step + rule.lam * dcos : d / rule.max_step;
                if (cost < best) best = cost, bi = c;   // (a lane's columns ascend: the smaller one stays on a tie)
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {   // lexicographic minimum of (cost, column): the same in every lane
            const double ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (ob < best || (ob == best && oi < bi)) best = ob, bi = oi;
        }
        if (lane == 0) out[r] = bi == INT_MAX ? -1 : bi;
    }
}

// `rule.max_step` is the gate of THIS level, max_step * (k + 1), multiplied once on the host in fp64.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void gap_level_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                          const double* __restrict__ pos, const float* __restrict__ emb, int R, LinkRule rule,
                                                          int level, int last_level, const char* __restrict__ state_in, GapFrames in, int P_lds,
                                                          int* succ_ws, int* matched_prev, int* matched_gap, int* __restrict__ new_rank_ws,
                                                          int* __restrict__ n_new_ws) {
    extern __shared__ int s_dyn[];
    int* fwd = s_dyn;           // [a] -> b; at the last level then the frame's final gaps
    int* bwd = s_dyn + P_lds;   // [b] -> a
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int S = in.off[in.n];
    int v0, n;
    if (!frame_range(node_ptr, g, N_all, v0, n)) {
        if (last_level && tid == 0) n_new_ws[g] = 0;
        return;
    }
    const int ca = usable_count(count, g, n, P_lds);
    int cb = 0, brow = 0;   // brow: the combined row of B's rank 0
    const double* ppos = nullptr;
    const float* pemb = nullptr;
    const int s = g - 1 - level;
    if (s >= 0) {
        int u0, m;
        if (frame_range(node_ptr, s, N_all, u0, m)) {
            cb = usable_count(count, s, m, P_lds);
            ppos = pos + 2 * (size_t)u0;
            pemb = emb + (size_t)u0 * R;
            brow = S + u0;
        }
    } else if (state_in && in.n + s >= 0) {
        const int f = in.n + s;
        cb = gap_hist_count(state_in, in, f, P_lds);
        brow = in.off[f];
        ppos = reinterpret_cast<const double*>(state_in + gap_pos_off()) + 2 * (size_t)brow;
        pemb = reinterpret_cast<const float*>(state_in + gap_emb_off(S)) + (size_t)brow * R;
    }
    if (ca > 0 && cb > 0) {   // (uniform)
        const double* cpos = pos + 2 * (size_t)v0;
        const float* cemb = emb + (size_t)v0 * R;
        best_partner_masked<BLOCK>(cpos, cemb, matched_gap + v0, -1, ca, ppos, pemb, succ_ws + brow, 0, cb, R, rule, fwd);
        best_partner_masked<BLOCK>(ppos, pemb, succ_ws + brow, 0, cb, cpos, cemb, matched_gap + v0, -1, ca, R, rule, bwd);
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
    if (tid < 64) {   // the clusters without a predecessor, numbered in rank order
        const unsigned long long below = (1ull << lane) - 1;
        int c = 0;
        for (int base = 0; base < ca; base += 64) {
            const int a = base + lane;
            const bool fresh = a < ca && fwd[a] < 0;
            const unsigned long long mk = __ballot(fresh);
            if (fresh) new_rank_ws[v0 + a] = c + __popcll(mk & below);
            c += __popcll(mk);
        }
        if (lane == 0) n_new_ws[g] = c;
    }
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
    const int S = in.off[in.n], So = out.off[out.n];
    const long long next0 = state_in ? reinterpret_cast<const GapHeader*>(state_in)->next_id : 0;
    const long long* in_track = state_in ? reinterpret_cast<const long long*>(state_in + gap_track_off(S)) : nullptr;
    GapHeader* oh = reinterpret_cast<GapHeader*>(state_out);
    double* opos = reinterpret_cast<double*>(state_out + gap_pos_off());
    long long* otrack = reinterpret_cast<long long*>(state_out + gap_track_off(So));
    float* oemb = reinterpret_cast<float*>(state_out + gap_emb_off(So));
    int* osucc = reinterpret_cast<int*>(state_out + gap_succ_off(So, R));
    const int first_kept = G - out.n;   // the batch frame that becomes slot 0 of the new state (negative: history frames stay)

    if ((int)blockIdx.x >= G) {   // a history frame that stays: slot j of the new state is frame f of the old one
        const int j = (int)blockIdx.x - G, f = in.n + first_kept + j;
        const int orow = out.off[j], irow = in.off[f];
        int c = gap_hist_count(state_in, in, f, P_lds);
        if (c > out.off[j + 1] - orow) c = 0;
        const double* ipos = reinterpret_cast<const double*>(state_in + gap_pos_off()) + 2 * (size_t)irow;
        const float* iemb = reinterpret_cast<const float*>(state_in + gap_emb_off(S)) + (size_t)irow * R;
        if (tid == 0) oh->count[j] = c;
        for (int i = tid; i < 2 * c; i += BLOCK) opos[2 * (size_t)orow + i] = ipos[i];
        for (int i = tid; i < c; i += BLOCK) {
            otrack[orow + i] = in_track[irow + i];
            osucc[orow + i] = succ_ws[irow + i];
        }
        for (size_t i = tid; i < (size_t)c * R; i += BLOCK) oemb[(size_t)orow * R + i] = iemb[i];
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
    for (int v = tid; v < n; v += BLOCK) {
        const int r = rank[v0 + v];
        node_track[v0 + v] = (r >= 0 && r < ca) ? s_track[r] : -1;
    }
    if (g == G - 1 && tid == 0) {
        oh->next_id = next0 + base_ws[G];
        oh->n_frames = out.n;
        oh->reid_dim = R;
    }
    if (g < first_kept) return;
    const int j = g - first_kept, orow = out.off[j];
    const int cs = ca <= out.off[j + 1] - orow ? ca : 0;   // (a frame with more clusters than its slot has rows is carried as empty)
    if (tid == 0) oh->count[j] = cs;
    for (int i = tid; i < 2 * cs; i += BLOCK) opos[2 * (size_t)orow + i] = pos[2 * (size_t)v0 + i];
    for (int c = tid; c < cs; c += BLOCK) {
        otrack[orow + c] = s_track[c];
        osucc[orow + c] = succ_ws[S + v0 + c];
    }
    for (size_t i = tid; i < (size_t)cs * R; i += BLOCK) oemb[(size_t)orow * R + i] = emb[(size_t)v0 * R + i];
}

// rows[0 .. n) -> running offsets; false if a frame is negative or above the per-frame limit
static bool gap_frames(const int32_t* rows, int n, GapFrames& f) {
    f.n = n;
    f.off[0] = 0;
    for (int i = 0; i < kGapMaxFrames; ++i) {
        int r = 0;
        if (i < n) {
            r = rows[i];
            if (r < 0 || r > kTrackMaxNodes) return false;
        }
        f.off[i + 1] = f.off[i] + r;
    }
    return true;
}

}  // namespace gnncca

extern "C" {

size_t gnncca_link_gap_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim) {
    if (capacity_rows < 0 || reid_dim < 0 || n_frames_kept < 0 || n_frames_kept > gnncca::kGapMaxFrames) return 0;
    return gnncca::round256(gnncca::gap_succ_off(capacity_rows, reid_dim) + (size_t)capacity_rows * sizeof(int32_t));
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
                               double miss_cost);

// gnncca_link_frames_gap (matching 0) and gnncca_link_frames_gap_ex: one body, the form of the level kernel chosen by `matching`
static int link_frames_gap_run(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                               int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                               int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t matching, double miss_cost, const void* state_in,
                               const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                               const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                               int32_t* matched_prev, int32_t* matched_gap, void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    if (n_nodes < 0 || n_frames < 0 || reid_dim < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_gap < 0 || max_gap > kTrackMaxGap) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kTrackMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (state_in_frames < 0 || state_in_frames > max_gap + 1 || (state_in_frames > 0 && (!state_in || !state_in_frame_rows)))
        return GNNCCA_ERR_INVALID_ARG;
    GapFrames in, out;
    if (!gap_frames(state_in_frame_rows, state_in ? state_in_frames : 0, in)) return GNNCCA_ERR_INVALID_ARG;   // a history frame above the limit
    if (matching) {   // the table of a frame pair lives in LDS: before any launch, for the batch and for the carried history alike
        if (max_frame_nodes > kTrackMaxOptimalNodes) return GNNCCA_ERR_INVALID_ARG;
        for (int f = 0; f < in.n; ++f)
            if (in.off[f + 1] - in.off[f] > kTrackMaxOptimalNodes) return GNNCCA_ERR_INVALID_ARG;
    }
    if (!(max_step > 0.0) || !(max_step < __builtin_inf()) || !(lam >= 0.0) || !(lam < __builtin_inf())) return GNNCCA_ERR_INVALID_ARG;
    if (has_max_cos && !(max_cos >= 0.0 && max_cos <= 2.0)) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;   // no time passes: the caller keeps its state
    const long long seen = (long long)in.n + n_frames;
    const int kept = (int)(seen < max_gap + 1 ? seen : max_gap + 1);
    if (state_out_frames != kept || !state_out_frame_rows || !gap_frames(state_out_frame_rows, kept, out)) return GNNCCA_ERR_INVALID_ARG;
    if (!node_ptr_dev || !count || !state_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!rank || !pos || !cluster_track || !node_track || !matched_prev || !matched_gap)) return GNNCCA_ERR_INVALID_ARG;
    LinkRule rule;
    rule.max_step = max_step, rule.lam = lam, rule.max_cos = max_cos;
    rule.has_max_cos = has_max_cos != 0;
    rule.need_emb = lam != 0.0 || has_max_cos != 0;
    // R is the rule's, not this batch's: a batch without rows (emb may then be NULL) must still carry the history's appearance rows along
    const int R = rule.need_emb ? (int)reid_dim : 0;
    if (R > 0 && n_nodes > 0 && !emb) return GNNCCA_ERR_INVALID_ARG;
    const int S = in.off[in.n];
    if (workspace_bytes < gnncca_link_gap_workspace_bytes(n_nodes, n_frames, S)) return GNNCCA_ERR_WORKSPACE;
    if (n_nodes >= (1ll << 31) - 64 - S) return GNNCCA_ERR_UNSUPPORTED;
    int P = 64;
    while (P < max_frame_nodes) P <<= 1;
    for (int f = 0; f < in.n; ++f)
        while (P < in.off[f + 1] - in.off[f]) P <<= 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* succ_ws = static_cast<int*>(workspace);
    int* new_rank_ws = succ_ws + S + n_nodes;
    int* n_new_ws = new_rank_ws + n_nodes;
    int* base_ws = n_new_ws + n_frames;
    const char* sin = in.n ? static_cast<const char*>(state_in) : nullptr;
    const long long cells = (long long)S + n_nodes;
    const unsigned init_blocks = (unsigned)(cells <= 0 ? 1 : (cells + 255) / 256 > 1024 ? 1024 : (cells + 255) / 256);
    hipLaunchKernelGGL(gap_init_kernel, dim3(init_blocks), dim3(256), 0, st, sin, S, R, (int)n_nodes, succ_ws, matched_prev, matched_gap);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k <= max_gap; ++k) {
        LinkRule level_rule = rule;
        level_rule.max_step = max_step * (double)(k + 1);   // gate_k: one fp64 multiplication
        if (matching) {
            const int rc = assign_level_launch(st, (int)n_frames, P, node_ptr_dev, (int)n_nodes, count, pos, emb, R, level_rule, k, (int)(k == max_gap),
                                               sin, in, succ_ws, matched_prev, matched_gap, new_rank_ws, n_new_ws, miss_cost);
            if (rc != GNNCCA_OK) return rc;
            continue;
        }
        hipLaunchKernelGGL((gap_level_kernel<256>), dim3((unsigned)n_frames), dim3(256), (size_t)2 * P * sizeof(int), st, node_ptr_dev, (int)n_nodes,
                           count, pos, emb, R, level_rule, k, (int)(k == max_gap), sin, in, P, succ_ws, matched_prev, matched_gap, new_rank_ws,
                           n_new_ws);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(64), 0, st, n_new_ws, (int)n_frames, base_ws);
    HIP_TRY(hipGetLastError());
    const int carried = kept > n_frames ? kept - n_frames : 0;   // history frames that stay in the new state
    hipLaunchKernelGGL((gap_ids_kernel<256>), dim3((unsigned)(n_frames + carried)), dim3(256), (size_t)P * sizeof(long long), st, node_ptr_dev,
                       (int)n_nodes, count, rank, pos, emb, R, (int)n_frames, matched_prev, matched_gap, new_rank_ws, base_ws, succ_ws, sin, in,
                       static_cast<char*>(state_out), out, P, reinterpret_cast<long long*>(cluster_track),
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
                                       state_out_frames, cluster_track, node_track, matched_prev, matched_gap, workspace, workspace_bytes, stream);
}

}  // extern "C"
