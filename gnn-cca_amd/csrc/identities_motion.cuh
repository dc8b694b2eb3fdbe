// identities_motion.cuh -- gap-tolerant linking with a constant-velocity prediction (gnncca_link_frames_motion), included at the end of
// identities.hip after identities_gap.cuh and identities_assign.cuh: it shares LinkRule, frame_range, usable_count, GapHeader, GapFrames,
// gap_hist_count and the file's `fp contract(off)`.  Nothing above it is touched.
//
// The rule (include/gnncca_mpn.h has it in full): the levels, gates, masks, cost, mutual best and ties of gnncca_link_frames_gap, but at
// level k cluster b of frame t - 1 - k is looked for at pred(b) = pos(b) + (double)(k + 1) * vel(b), and a cluster a linked at level k to b
// gets vel(a) = (pos(a) - pos(b)) / (double)(k + 1).  vel(b) is known only when frame t - 1 - k has been through ALL its levels, so the
// order is frames outside, levels inside: the dependency is serial in time and ONE workgroup walks the frames of the batch.
// Launches, 3 of them whatever max_gap is:
//   1. motion_init_kernel (frame-parallel): predecessor record of the N batch rows = none, velocity = 0, successor flags of the S history
//      rows copied from state_in (which is never written), of the batch rows cleared -- one array over the COMBINED rows as in the gap path.
//   2. motion_walk_kernel, grid = 1: for every frame in order the levels 0 .. M (fwd / bwd in LDS, best_partner_motion, commit between
//      barriers), then the ids at once -- the running next_id is known because the frames go in order; the clusters without a predecessor
//      are numbered in ascending rank by the ballot scan.  No workgroup waits for another: there is only one.
//   3. motion_finish_kernel, grid = G + the history frames carried along (frame-parallel): node tracks and the rows of the new state.
// Arrays the walking workgroup writes and later reads (the predecessor record, the successor flags, velocity, cluster_track) are plain
// pointers -- not const, not __restrict__ -- and every frame's and level's writes are ordered before the next one's reads by __syncthreads().
// They reach the walk as one block (WalkOutputs) that it keeps in LDS and reads where a level is set up, committed or numbered: held in
// scalar registers over the whole walk they did not fit beside the two inlined partner searches (DESIGN.md section 9 has the numbers).
// The carried state: GapHeader (64 bytes), then for a total capacity of C rows: pos fp64 [C][2], vel fp64 [C][2], track int64 [C],
// emb fp32 [C][R], succ int32 [C] -- every 8-byte array before the 4-byte ones.  A state of its own kind: the gap state's layout is as it was.
#pragma once

namespace gnncca {

__host__ __device__ inline size_t motion_pos_off() { return sizeof(GapHeader); }
__host__ __device__ inline size_t motion_vel_off(long long cap) { return sizeof(GapHeader) + (size_t)cap * 16; }
__host__ __device__ inline size_t motion_track_off(long long cap) { return sizeof(GapHeader) + (size_t)cap * 32; }
__host__ __device__ inline size_t motion_emb_off(long long cap) { return sizeof(GapHeader) + (size_t)cap * 40; }
__host__ __device__ inline size_t motion_succ_off(long long cap, int R) { return motion_emb_off(cap) + (size_t)cap * (size_t)R * sizeof(float); }

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void motion_init_kernel(const char* __restrict__ state_in, int S, int R, int N_all, int* __restrict__ succ_ws,
                                                          int* __restrict__ matched_prev, int* __restrict__ matched_gap,
                                                          double* __restrict__ velocity) {
    const int* in_succ = state_in ? reinterpret_cast<const int*>(state_in + motion_succ_off(S, R)) : nullptr;
    const long long total = (long long)S + N_all;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (i < S) {
            succ_ws[i] = in_succ[i] != 0;
        } else {
            succ_ws[i] = 0;
            matched_prev[i - S] = -1;
            matched_gap[i - S] = -1;
            velocity[2 * (i - S)] = 0.0;
            velocity[2 * (i - S) + 1] = 0.0;
        }
    }
}

// ---- launch 2: the walk ---------------------------------------------------------------------------------------------------------------
// best_partner_masked where a side with a velocity stands at pos + steps * vel (one multiplication, one addition per component; the
// other side passes vel = nullptr and stands at pos).  dx is squared, so which side is subtracted from which does not change a bit of d.
// The masks, the velocities and `out` are not __restrict__: the workgroup wrote them in an earlier frame or level, before a barrier.
// The walk is one workgroup deep, so a table's chain of memory round trips is what it waits for: a row's and a column's mask, position
// and velocity are loaded together and the mask is looked at afterwards, and the cosine keeps four loads per side in flight and adds
// them in the order of the one-load loop (k = lane, lane + 64, ...: the same bits).
template <int BLOCK>
__device__ void best_partner_motion(const double* __restrict__ rpos, const double* rvel, const float* __restrict__ remb, const int* rmask, int rfree,
                                    int nr, const double* __restrict__ cpos, const double* cvel, const float* __restrict__ cemb, const int* cmask,
                                    int cfree, int nc, double steps, double gate, double lam, double max_cos, int R, const LinkRule& rule, int* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nr; r += BLOCK / 64) {
        const int rm = rmask[r];   // (the mask is loaded with the position and looked at afterwards: one round trip, not two)
        double rx = rpos[2 * (size_t)r], ry = rpos[2 * (size_t)r + 1];
        if (rvel) {
            rx = rx + steps * rvel[2 * (size_t)r];
            ry = ry + steps * rvel[2 * (size_t)r + 1];
        }
        if (rm != rfree) {   // (uniform in the wave)
            if (lane == 0) out[r] = -1;
            continue;
        }
        double best = __builtin_inf();
        int bi = INT_MAX;
        for (int base = 0; base < nc; base += 64) {
            const int c = base + lane;
            bool cand = false;
            double d = 0.0, dcos = 0.0;
            if (c < nc) {
                const int cm = cmask[c];
                double cx = cpos[2 * (size_t)c], cy = cpos[2 * (size_t)c + 1];
                if (cvel) {
                    cx = cx + steps * cvel[2 * (size_t)c];
                    cy = cy + steps * cvel[2 * (size_t)c + 1];
                }
                if (cm == cfree) {
                    const double dx = rx - cx, dy = ry - cy;
                    d = sqrt(dx * dx + dy * dy);
                    cand = d <= gate;   // (a NaN d is admissible with nobody)
                }
            }
            if (rule.need_emb) {
                unsigned long long todo = __ballot(cand);   // (uniform) the pairs inside the gate: the whole wave computes each cosine
                while (todo) {
                    const int j = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const float* er = remb + (size_t)r * R;
                    const float* ec = cemb + (size_t)(base + j) * R;
                    double dot = 0.0, na = 0.0, nb = 0.0;
                    int k = lane;
                    for (; k + 3 * 64 < R; k += 4 * 64) {   // four loads per side in flight; one addition per element, in the order of k
                        float xs[4], ys[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            xs[u] = er[k + 64 * u];
                            ys[u] = ec[k + 64 * u];
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const double x = (double)xs[u], y = (double)ys[u];
                            dot += x * y;
                            na += x * x;
                            nb += y * y;
                        }
                    }
                    for (; k < R; k += 64) {
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
                if (rule.has_max_cos) cand = cand && dcos <= max_cos;
            }
            if (cand) {
                const double cost = rule.need_emb ? d / gate + lam * dcos : d / gate;
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

// One workgroup, every frame of the batch in order.  `rule.max_step` is the caller's max_step; the gate of level k is max_step * (k + 1),
// one fp64 multiplication.  Every loop is bounded by G, max_gap, P_lds (a count above it is taken as 0) or the 64 lanes of a wave.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void motion_walk_kernel(const int* __restrict__ node_ptr, int N_all, int G, const int* __restrict__ count,
                                                            const double* __restrict__ pos, int R, LinkRule rule,
                                                            int max_gap, GapFrames in, int P_lds, WalkOutputs outs) {
    extern __shared__ int s_dyn[];
    __shared__ int s_fresh;
    int* fwd = s_dyn;                // [a] -> b; after the levels: a fresh cluster's rank among the frame's fresh ones
    int* bwd = s_dyn + P_lds;        // [b] -> a
    int* gap_a = s_dyn + 2 * P_lds;  // the frame's predecessor record as it grows: -1, or the level that found it
    const int tid = threadIdx.x, lane = tid & 63;
    // What only the commit and the ids use is kept in LDS and read where it is used, not held in scalar registers over the walk: the
    // history's row offsets and the output pointers.
    __shared__ int s_off[kGapMaxFrames + 1];
    __shared__ WalkOutputs s_out;
    if (tid <= kGapMaxFrames) s_off[tid] = in.off[tid];
    if (tid == 0) s_out = outs;
    const int S = in.off[in.n], HN = in.n;
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
            int cb = 0, brow = 0;   // brow: the combined row of B's rank 0
            const double* bpos = nullptr;
            const double* bvel = nullptr;
            const float* bemb = nullptr;
            const int s = t - 1 - k;
            const char* state_in = s_out.state_in;
            int* succ_ws = s_out.succ;
            const double lam = s_out.lam, max_cos = s_out.max_cos;
            if (s >= 0) {
                int u0, m;
                if (frame_range(node_ptr, s, N_all, u0, m)) {
                    cb = usable_count(count, s, m, P_lds);
                    bpos = pos + 2 * (size_t)u0;
                    bvel = s_out.velocity + 2 * (size_t)u0;
                    bemb = emb + (size_t)u0 * R;
                    brow = S + u0;
                }
            } else if (state_in && HN + s >= 0) {
                const int f = HN + s;
                brow = __builtin_amdgcn_readfirstlane(s_off[f]);
                const int c = reinterpret_cast<const GapHeader*>(state_in)->count[f];   // (gap_hist_count, with the offsets from LDS)
                cb = (c >= 0 && c <= __builtin_amdgcn_readfirstlane(s_off[f + 1]) - brow && c <= P_lds) ? c : 0;
                bpos = reinterpret_cast<const double*>(state_in + motion_pos_off()) + 2 * (size_t)brow;
                bvel = reinterpret_cast<const double*>(state_in + motion_vel_off(S)) + 2 * (size_t)brow;
                bemb = reinterpret_cast<const float*>(state_in + motion_emb_off(S)) + (size_t)brow * R;
            }
            if (cb == 0) continue;   // (uniform: the counts are the same in every thread)
            const double steps = (double)(k + 1);
            const double gate = rule.max_step * steps;   // gate_k: one fp64 multiplication
            best_partner_motion<BLOCK>(apos, nullptr, aemb, gap_a, -1, ca, bpos, bvel, bemb, succ_ws + brow, 0, cb, steps, gate, lam, max_cos, R, rule, fwd);
            best_partner_motion<BLOCK>(bpos, bvel, bemb, succ_ws + brow, 0, cb, apos, nullptr, aemb, gap_a, -1, ca, steps, gate, lam, max_cos, R, rule, bwd);
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
        if (tid < 64) {   // the clusters without a predecessor, numbered in rank order
            const unsigned long long below = (1ull << lane) - 1;
            int c = 0;
            for (int base = 0; base < ca; base += 64) {
                const int a = base + lane;
                const bool fresh = a < ca && gap_a[a] < 0;
                const unsigned long long mk = __ballot(fresh);
                if (fresh) fwd[a] = c + __popcll(mk & below);
                c += __popcll(mk);
            }
            if (lane == 0) s_fresh = c;
        }
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
                              : reinterpret_cast<const long long*>(state_in + motion_track_off(S))[s_off[HN + tp] + m];
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
    const int S = in.off[in.n], So = out.off[out.n];
    GapHeader* oh = reinterpret_cast<GapHeader*>(state_out);   // (next_id, at offset 0, is the walk's to write)
    double* opos = reinterpret_cast<double*>(state_out + motion_pos_off());
    double* ovel = reinterpret_cast<double*>(state_out + motion_vel_off(So));
    long long* otrack = reinterpret_cast<long long*>(state_out + motion_track_off(So));
    float* oemb = reinterpret_cast<float*>(state_out + motion_emb_off(So));
    int* osucc = reinterpret_cast<int*>(state_out + motion_succ_off(So, R));
    const int first_kept = G - out.n;   // the batch frame that becomes slot 0 of the new state (negative: history frames stay)

    if ((int)blockIdx.x >= G) {   // a history frame that stays: slot j of the new state is frame f of the old one
        const int j = (int)blockIdx.x - G, f = in.n + first_kept + j;
        const int orow = out.off[j], irow = in.off[f];
        int c = gap_hist_count(state_in, in, f, P_lds);
        if (c > out.off[j + 1] - orow) c = 0;
        const double* ipos = reinterpret_cast<const double*>(state_in + motion_pos_off()) + 2 * (size_t)irow;
        const double* ivel = reinterpret_cast<const double*>(state_in + motion_vel_off(S)) + 2 * (size_t)irow;
        const long long* itrack = reinterpret_cast<const long long*>(state_in + motion_track_off(S)) + irow;
        const float* iemb = reinterpret_cast<const float*>(state_in + motion_emb_off(S)) + (size_t)irow * R;
        if (tid == 0) oh->count[j] = c;
        for (int i = tid; i < 2 * c; i += BLOCK) {
            opos[2 * (size_t)orow + i] = ipos[i];
            ovel[2 * (size_t)orow + i] = ivel[i];
        }
        for (int i = tid; i < c; i += BLOCK) {
            otrack[orow + i] = itrack[i];
            osucc[orow + i] = succ_ws[irow + i];
        }
        for (size_t i = tid; i < (size_t)c * R; i += BLOCK) oemb[(size_t)orow * R + i] = iemb[i];
        return;
    }

    const int g = blockIdx.x;
    int v0, n;
    const bool ok = frame_range(node_ptr, g, N_all, v0, n);
    const int ca = ok ? usable_count(count, g, n, P_lds) : 0;
    for (int v = tid; v < n; v += BLOCK) {
        const int r = rank[v0 + v];
        node_track[v0 + v] = (r >= 0 && r < ca) ? cluster_track[v0 + r] : -1;
    }
    if (g == G - 1 && tid == 0) {
        oh->n_frames = out.n;
        oh->reid_dim = R;
    }
    if (g < first_kept) return;
    const int j = g - first_kept, orow = out.off[j];
    const int cs = ca <= out.off[j + 1] - orow ? ca : 0;   // (a frame with more clusters than its slot has rows is carried as empty)
    if (tid == 0) oh->count[j] = cs;
    for (int i = tid; i < 2 * cs; i += BLOCK) {
        opos[2 * (size_t)orow + i] = pos[2 * (size_t)v0 + i];
        ovel[2 * (size_t)orow + i] = velocity[2 * (size_t)v0 + i];
    }
    for (int c = tid; c < cs; c += BLOCK) {
        otrack[orow + c] = cluster_track[v0 + c];
        osucc[orow + c] = succ_ws[S + v0 + c];
    }
    for (size_t i = tid; i < (size_t)cs * R; i += BLOCK) oemb[(size_t)orow * R + i] = emb[(size_t)v0 * R + i];
}

constexpr int kMotionWalkBlock = 1024;   // one workgroup has the CU to itself, a wave takes a row

}  // namespace gnncca

extern "C" {

size_t gnncca_link_motion_state_bytes(int64_t capacity_rows, int32_t n_frames_kept, int32_t reid_dim) {
    if (capacity_rows < 0 || reid_dim < 0 || n_frames_kept < 0 || n_frames_kept > gnncca::kGapMaxFrames) return 0;
    return gnncca::round256(gnncca::motion_succ_off(capacity_rows, reid_dim) + (size_t)capacity_rows * sizeof(int32_t));
}

size_t gnncca_link_motion_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows) {
    if (n_nodes < 0 || n_frames < 0 || state_rows < 0) return 0;
    return gnncca::round256(((size_t)state_rows + (size_t)n_nodes) * sizeof(int32_t));   // successor flags [S + N]
}

int gnncca_link_frames_motion(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                              int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                              int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t motion, const void* state_in,
                              const int32_t* state_in_frame_rows, int32_t state_in_frames, void* state_out,
                              const int32_t* state_out_frame_rows, int32_t state_out_frames, int64_t* cluster_track, int64_t* node_track,
                              int32_t* matched_prev, int32_t* matched_gap, double* velocity, void* workspace, size_t workspace_bytes,
                              gnncca_stream_t stream) {
    using namespace gnncca;
    if (motion != 1) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes < 0 || n_frames < 0 || reid_dim < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_gap < 0 || max_gap > kTrackMaxGap) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kTrackMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (state_in_frames < 0 || state_in_frames > max_gap + 1 || (state_in_frames > 0 && (!state_in || !state_in_frame_rows)))
        return GNNCCA_ERR_INVALID_ARG;
    GapFrames in, out;
    if (!gap_frames(state_in_frame_rows, state_in ? state_in_frames : 0, in)) return GNNCCA_ERR_INVALID_ARG;   // a history frame above the limit
    if (!(max_step > 0.0) || !(max_step < __builtin_inf()) || !(lam >= 0.0) || !(lam < __builtin_inf())) return GNNCCA_ERR_INVALID_ARG;
    if (has_max_cos && !(max_cos >= 0.0 && max_cos <= 2.0)) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;   // no time passes: the caller keeps its state
    const long long seen = (long long)in.n + n_frames;
    const int kept = (int)(seen < max_gap + 1 ? seen : max_gap + 1);
    if (state_out_frames != kept || !state_out_frame_rows || !gap_frames(state_out_frame_rows, kept, out)) return GNNCCA_ERR_INVALID_ARG;
    if (!node_ptr_dev || !count || !state_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!rank || !pos || !cluster_track || !node_track || !matched_prev || !matched_gap || !velocity)) return GNNCCA_ERR_INVALID_ARG;
    LinkRule rule;
    rule.max_step = max_step, rule.lam = lam, rule.max_cos = max_cos;
    rule.has_max_cos = has_max_cos != 0;
    rule.need_emb = lam != 0.0 || has_max_cos != 0;
    // R is the rule's, not this batch's: a batch without rows (emb may then be NULL) must still carry the history's appearance rows along
    const int R = rule.need_emb ? (int)reid_dim : 0;
    if (R > 0 && n_nodes > 0 && !emb) return GNNCCA_ERR_INVALID_ARG;
    const int S = in.off[in.n];
    if (workspace_bytes < gnncca_link_motion_workspace_bytes(n_nodes, n_frames, S)) return GNNCCA_ERR_WORKSPACE;
    if (n_nodes >= (1ll << 31) - 64 - S) return GNNCCA_ERR_UNSUPPORTED;
    int P = 64;
    while (P < max_frame_nodes) P <<= 1;
    for (int f = 0; f < in.n; ++f)
        while (P < in.off[f + 1] - in.off[f]) P <<= 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* succ_ws = static_cast<int*>(workspace);
    const char* sin = in.n ? static_cast<const char*>(state_in) : nullptr;
    char* sout = static_cast<char*>(state_out);
    const long long cells = (long long)S + n_nodes;
    const unsigned init_blocks = (unsigned)(cells <= 0 ? 1 : (cells + 255) / 256 > 1024 ? 1024 : (cells + 255) / 256);
    hipLaunchKernelGGL(motion_init_kernel, dim3(init_blocks), dim3(256), 0, st, sin, S, R, (int)n_nodes, succ_ws, matched_prev, matched_gap, velocity);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((motion_walk_kernel<kMotionWalkBlock>), dim3(1), dim3(kMotionWalkBlock), (size_t)3 * P * sizeof(int), st, node_ptr_dev,
                       (int)n_nodes, (int)n_frames, count, pos, R, rule, (int)max_gap, in, P,
                       WalkOutputs{matched_prev, matched_gap, velocity, reinterpret_cast<long long*>(cluster_track),
                                   &reinterpret_cast<GapHeader*>(sout)->next_id, succ_ws, sin, lam, max_cos, emb});
    HIP_TRY(hipGetLastError());
    const int carried = kept > n_frames ? kept - n_frames : 0;   // history frames that stay in the new state
    hipLaunchKernelGGL((motion_finish_kernel<256>), dim3((unsigned)(n_frames + carried)), dim3(256), 0, st, node_ptr_dev, (int)n_nodes, count, rank,
                       pos, emb, R, (int)n_frames, velocity, reinterpret_cast<const long long*>(cluster_track), succ_ws, sin, in, sout, out, P,
                       reinterpret_cast<long long*>(node_track));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
