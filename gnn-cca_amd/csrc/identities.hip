// identities.hip -- what a consumer of the frames pipeline does with its partition, on gfx950: per-cluster summaries (fused ground-plane
// position, mean appearance, size, camera count) and track ids that persist across the frames of a batch and across batches.  The
// reference has NO counterpart: it scores single frames (inference.py:349-371) and never fuses a cluster or links two frames.
//
// Summaries (gnncca_cluster_summaries), two launches:
//   1. one workgroup per frame, frame-local state in LDS (3 x P int32, P = the batch's largest frame rounded up to a power of two: 48 KiB at
//      4096 nodes): the labels are checked (inside the frame, pointing at a root), the roots are ranked in ascending id (ballot scan), the
//      24-bit keys (rank << 12 | node) are sorted (bitonic), which leaves every cluster's members contiguous in ascending node id; then one
//      thread per cluster sums xw / yw over its run SEQUENTIALLY in fp64 and divides once, and one thread per member decides whether its
//      camera is the first of its value in the run (LDS integer atomics count them).  The member order and each cluster's first position go
//      to the caller's workspace.
//   2. (frame, 256-column tile, row slice): emb[c][col] = the sequential fp32 sum over the members in that order, one division by (float)
//      size.  A thread owns a column, so the row reads are coalesced and a large frame is not served by one workgroup.
// Linking (gnncca_link_frames), three launches:
//   1. one workgroup per pair (frame t, frame t - 1; frame 0 against the carried state): fwd[a] and bwd[b] in LDS, the costs streamed -- a
//      wave takes a row, its lanes the columns; a pair inside max_step gets its cosine from the whole wave (lane-strided fp64 partial sums,
//      then a butterfly: a fixed order), and the wave's best (cost, index) is a lexicographic minimum, so ties go to the smaller index.
//      Then matched_prev and, for the unmatched clusters, their rank among the frame's unmatched ones (ballot scan);
//   2. one small workgroup: exclusive prefix sum of the per-frame unmatched counts (integers);
//   3. one workgroup per frame: a matched cluster follows matched_prev back to the head of its chain (an unmatched cluster: next_id + the
//      prefix of its frame + its rank among the unmatched; or a cluster of the carried state: its id), then node_track; the last frame's
//      workgroup writes the new state.
// The rule that decides a link -- distance, gate, whole-wave cosine, max_cos, cost, the tie -- is written ONCE, in link_common.cuh (included
// below, after `fp contract(off)`), with the partner search, the ballot-scan numbering, the carried history state and the host-side checks
// of the history entries; link_match_kernel above instantiates the search without masks, with one load per side in flight.
// Gap-tolerant linking (gnncca_link_frames_gap: a track survives up to max_gap frames that miss it) is identities_gap.cuh, included at the
// end of this file: its level and ids kernels, the scan kernel shared.  Its level kernel has a second form that picks the pairs of a
// frame pair by a min-cost assignment instead of mutual best (gnncca_link_frames_gap_ex, matching = 1): identities_assign.cuh, after it.
// Scoring the track ids against ground-truth person ids over a sequence (gnncca_track_score_*) is track_score.cuh, included after it:
// integer kernels of its own, nothing shared but this translation unit.  identities_motion.cuh (gnncca_link_frames_motion) comes last.
// A time stamp per frame (gnncca_link_frames_gap_timed in identities_assign.cuh, gnncca_link_frames_motion_timed in identities_motion.cuh)
// is an argument of the same level and walk kernels, not a kernel of its own: link_common.cuh's level_dt.
// The re-entry gallery (gnncca_reentry_update: a track born after a long absence gets an ended track's identity) is identities_reentry.cuh,
// kernels of its own that share frame_range, usable_count, wave_number and wave_min_lex.  The track smoother (gnncca_track_smooth: a
// constant-velocity Kalman filter along the links the linkers made) is identities_smooth.cuh, the last include: three kernels, chain-parallel.
// The Kalman linker (gnncca_link_frames_kalman: the motion walk that predicts with that filter, feeds it and can gate by its variance) is
// identities_kalman.cuh, after identities_motion.cuh; the filter's arithmetic is link_common.cuh's, one definition for both.
// Deterministic: every fp sum has a fixed order, integer counts go through LDS atomics, no fp64 atomics.  No host wait, no allocation:
// capturable.  The file is compiled without fp contraction: the sums, the divisions and the cost are the documented operations one by one.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "hip_try.h"

#pragma clang fp contract(off)

namespace gnncca {

constexpr int kTrackMaxNodes = GNNCCA_TRACK_MAX_FRAME_NODES;   // 12-bit frame-local ids in the sort keys

// The carried state of the linker: header, then pos fp64 [cap][2], track int64 [cap], emb fp32 [cap][R] (cap: the caller's capacity).
struct LinkHeader {
    long long next_id;
    int count;
    int reid_dim;
};
__host__ __device__ inline size_t state_pos_off() { return sizeof(LinkHeader); }
__host__ __device__ inline size_t state_track_off(long long cap) { return sizeof(LinkHeader) + (size_t)cap * 16; }
__host__ __device__ inline size_t state_emb_off(long long cap) { return sizeof(LinkHeader) + (size_t)cap * 24; }

// frame g's node range [v0, v0 + n) if it lies inside [0, N_all]
__device__ __forceinline__ bool frame_range(const int* __restrict__ node_ptr, int g, int N_all, int& v0, int& n) {
    v0 = node_ptr[g];
    const int v1 = node_ptr[g + 1];
    const bool ok = v0 >= 0 && v1 >= v0 && v1 <= N_all;
    n = ok ? v1 - v0 : 0;
    return ok;
}

__device__ __forceinline__ int lds_get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);   // every lane ends with the same bits (a + b == b + a)
    return v;
}

}  // namespace gnncca

#include "link_common.cuh"   // the pair rule, the partner search, numbering, the history state: what all linkers below share

namespace gnncca {

// ---- summaries, launch 1 ------------------------------------------------------------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void summaries_kernel(const int* __restrict__ labels, int N_all, const int* __restrict__ node_ptr,
                                                          const double* __restrict__ xw, const double* __restrict__ yw,
                                                          const int* __restrict__ cam, int P_lds, int max_n, int* __restrict__ count_out,
                                                          int* __restrict__ rank_out, int* __restrict__ size_out, int* __restrict__ ncam_out,
                                                          double* __restrict__ pos_out, int* __restrict__ order_ws, int* __restrict__ start_ws) {
    extern __shared__ int s_dyn[];
    __shared__ int s_bad, s_count;
    int* lab = s_dyn;                                                // frame-local label; after the sort: cam in member order
    int* rk = s_dyn + P_lds;                                         // rank of a local root; after the sort: per cluster, start | n_cams << 12
    unsigned* keys = reinterpret_cast<unsigned*>(s_dyn + 2 * P_lds);   // rank << 12 | node, sorted

    const int g = blockIdx.x, tid = threadIdx.x;
    int v0, n;
    if (!frame_range(node_ptr, g, N_all, v0, n)) {   // no rows to call this frame's
        if (tid == 0) count_out[g] = -1;
        return;
    }
    if (tid == 0) s_bad = 0, s_count = 0;
    __syncthreads();
    const bool fits = n <= max_n;   // (max_n <= P_lds)
    if (fits) {
        int bad = 0;
        for (int v = tid; v < n; v += BLOCK) {
            const long long lp = (long long)labels[v0 + v] - v0;
            const bool in = lp >= 0 && lp < n;
            bad |= !in;
            lab[v] = in ? (int)lp : v;
        }
        __syncthreads();
        for (int v = tid; v < n; v += BLOCK) {
            const int r = lab[v];
            bad |= lab[r] != r;   // the label is not a root
        }
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
    }
    if (!fits || s_bad) {   // (uniform) the frame is refused: count -1, zero rows
        for (int v = tid; v < n; v += BLOCK) {
            rank_out[v0 + v] = -1;
            size_out[v0 + v] = 0;
            ncam_out[v0 + v] = 0;
            pos_out[2 * (size_t)(v0 + v)] = 0.0;
            pos_out[2 * (size_t)(v0 + v) + 1] = 0.0;
        }
        if (tid == 0) count_out[g] = -1;
        return;
    }

    // ranks of the roots in ascending id
    if (tid < 64) {
        const int c = wave_number(n, [&](int v) { return lab[v] == v; }, [&](int v, int k) { rk[v] = k; });
        if (tid == 0) s_count = c;
    }
    __syncthreads();
    const int count = s_count;
    int sort_n = 1;
    while (sort_n < n) sort_n <<= 1;   // (<= P_lds)
    for (int v = tid; v < n; v += BLOCK) {
        const int r = rk[lab[v]];
        keys[v] = ((unsigned)r << 12) | (unsigned)v;
        rank_out[v0 + v] = r;
    }
    for (int v = n + tid; v < sort_n; v += BLOCK) keys[v] = 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= sort_n; k <<= 1) {   // bitonic sort: a cluster's members end up contiguous, in ascending node id
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < sort_n; i += BLOCK) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned x = keys[i], y = keys[l];
                    if ((x > y) == ((i & k) == 0)) {
                        keys[i] = y;
                        keys[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int p = tid; p < n; p += BLOCK) {
        const unsigned key = keys[p];
        const int c = (int)(key >> 12), v = (int)(key & 0xFFFu);
        if (p == 0 || (int)(keys[p - 1] >> 12) != c) rk[c] = p;   // the cluster's first position (n_cams: 0)
        lab[p] = cam[v0 + v];
        order_ws[v0 + p] = v0 + v;
    }
    __syncthreads();
    for (int p = tid; p < n; p += BLOCK) {   // is this member's camera the first of its value in the run?
        const int c = (int)(keys[p] >> 12), s = lds_get(&rk[c]) & 0xFFF, mine = lab[p];
        bool first = true;
        for (int q = s; q < p; ++q) {
            if (lab[q] == mine) {
                first = false;
                break;
            }
        }
        if (first) atomicAdd(&rk[c], 1 << 12);
    }
    __syncthreads();
    for (int c = tid; c < n; c += BLOCK) {
        int size = 0, ncam = 0, s = 0;
        double px = 0.0, py = 0.0;
        if (c < count) {
            const int w = rk[c];
            s = w & 0xFFF;
            ncam = w >> 12;
            size = (c + 1 < count ? (rk[c + 1] & 0xFFF) : n) - s;
            double sx = 0.0, sy = 0.0;
            for (int p = s; p < s + size; ++p) {   // ascending node id, one addition per member
                const int v = v0 + (int)(keys[p] & 0xFFFu);
                sx += xw[v];
                sy += yw[v];
            }
            px = sx / (double)size;
            py = sy / (double)size;
        }
        size_out[v0 + c] = size;
        ncam_out[v0 + c] = ncam;
        pos_out[2 * (size_t)(v0 + c)] = px;
        pos_out[2 * (size_t)(v0 + c) + 1] = py;
        start_ws[v0 + c] = v0 + s;
    }
    if (tid == 0) count_out[g] = count;
}

// ---- summaries, launch 2: the mean appearance rows --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void summaries_emb_kernel(const float* __restrict__ embeds, int R, int N_all, const int* __restrict__ node_ptr,
                                                            const int* __restrict__ count, const int* __restrict__ size,
                                                            const int* __restrict__ order_ws, const int* __restrict__ start_ws,
                                                            float* __restrict__ emb_out) {
    const int g = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    int v0, n;
    if (!frame_range(node_ptr, g, N_all, v0, n) || col >= R) return;
    const int cnt = count[g];
    for (int c = blockIdx.z; c < n; c += gridDim.z) {
        float out = 0.f;
        if (c < cnt) {
            const int s = start_ws[v0 + c], sz = size[v0 + c];
            float acc = 0.f;
            for (int p = s; p < s + sz; ++p) acc += embeds[(size_t)order_ws[p] * R + col];
            out = acc / (float)sz;
        }
        emb_out[(size_t)(v0 + c) * R + col] = out;
    }
}

// ---- linking, launch 1: mutual-best matches of a frame pair -----------------------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void link_match_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                           const double* __restrict__ pos, const float* __restrict__ emb, int R, LinkRule rule,
                                                           const char* __restrict__ state_in, long long state_in_cap, int P_lds,
                                                           int* __restrict__ matched_prev, int* __restrict__ new_rank_ws,
                                                           int* __restrict__ n_new_ws) {
    extern __shared__ int s_dyn[];
    int* fwd = s_dyn;           // [a] -> b, later the match itself
    int* bwd = s_dyn + P_lds;   // [b] -> a
    const int g = blockIdx.x, tid = threadIdx.x;
    int v0, n;
    if (!frame_range(node_ptr, g, N_all, v0, n)) {
        if (tid == 0) n_new_ws[g] = 0;
        return;
    }
    const LinkSide cur{pos + 2 * (size_t)v0, nullptr, emb + (size_t)v0 * R, nullptr, 0, usable_count(count, g, n, P_lds)};
    const int ca = cur.n;
    LinkSide prev{nullptr, nullptr, nullptr, nullptr, 0, 0};
    if (g > 0) {
        int row;
        prev = side_b(g - 1, node_ptr, N_all, count, pos, nullptr, emb, R, nullptr, 0, nullptr, 0, false, P_lds, row);
    } else if (state_in) {
        const LinkHeader* h = reinterpret_cast<const LinkHeader*>(state_in);
        const int c = h->count;
        prev.n = (c >= 0 && c <= state_in_cap && c <= P_lds) ? c : 0;
        prev.pos = reinterpret_cast<const double*>(state_in + state_pos_off());
        prev.emb = reinterpret_cast<const float*>(state_in + state_emb_off(state_in_cap));
    }
    mutual_best<BLOCK, 1, false>(cur, prev, 1.0, R, rule, fwd, bwd);
    __syncthreads();
    for (int a = tid; a < n; a += BLOCK) {
        int m = -1;
        if (a < ca) {
            const int b = fwd[a];
            m = (b >= 0 && bwd[b] == a) ? b : -1;
        }
        matched_prev[v0 + a] = m;
    }
    __syncthreads();   // (fwd is overwritten only after every read of it above)
    for (int a = tid; a < ca; a += BLOCK) fwd[a] = matched_prev[v0 + a];   // each thread reads what it wrote itself
    __syncthreads();
    number_fresh(fwd, ca, new_rank_ws + v0, n_new_ws + g);   // the unmatched clusters, numbered in rank order
}

// ---- linking, launch 2: base[g] = the unmatched clusters of the frames before g (base[G]: all of them) -------------------------------
__global__ __launch_bounds__(64) void link_scan_kernel(const int* __restrict__ n_new_ws, int G, int* __restrict__ base_ws) {
    const int lane = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < G; b0 += 64) {
        const int q = b0 + lane;
        const int x = q < G ? n_new_ws[q] : 0;
        int inc = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(inc, o);
            if (lane >= o) inc += y;
        }
        if (q < G) base_ws[q] = carry + inc - x;
        carry += __shfl(inc, 63);
    }
    if (lane == 0) base_ws[G] = carry;
}

// ---- linking, launch 3: ids along the chains, node tracks, the new state -----------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void link_ids_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                         const int* __restrict__ rank, const double* __restrict__ pos,
                                                         const float* __restrict__ emb, int R, int G, const int* __restrict__ matched_prev,
                                                         const int* __restrict__ new_rank_ws, const int* __restrict__ base_ws,
                                                         const char* __restrict__ state_in, long long state_in_cap, char* __restrict__ state_out,
                                                         long long state_out_cap, int P_lds, long long* __restrict__ cluster_track,
                                                         long long* __restrict__ node_track) {
    extern __shared__ long long s_track[];
    const int g = blockIdx.x, tid = threadIdx.x;
    const long long next0 = state_in ? reinterpret_cast<const LinkHeader*>(state_in)->next_id : 0;
    const long long* in_track = state_in ? reinterpret_cast<const long long*>(state_in + state_track_off(state_in_cap)) : nullptr;
    int v0, n;
    const bool ok = frame_range(node_ptr, g, N_all, v0, n);
    const int ca = ok ? usable_count(count, g, n, P_lds) : 0;
    for (int c = tid; c < ca; c += BLOCK) {
        // back along matched_prev to the head of the chain (link_match_kernel wrote a match only into a usable previous frame or state)
        int t = g, cc = c;
        long long id;
        for (;;) {
            const int row = node_ptr[t] + cc;
            const int m = matched_prev[row];
            if (m < 0) {
                id = next0 + base_ws[t] + new_rank_ws[row];
                break;
            }
            if (t == 0) {
                id = in_track[m];
                break;
            }
            --t;
            cc = m;
        }
        s_track[c] = id;
        cluster_track[v0 + c] = id;
    }
    for (int c = ca + tid; c < n; c += BLOCK) cluster_track[v0 + c] = -1;
    __syncthreads();
    write_node_tracks<BLOCK>(rank + v0, n, ca, s_track, node_track + v0);
    if (g != G - 1) return;
    const int cs = ca <= state_out_cap ? ca : 0;
    if (tid == 0) {
        LinkHeader* h = reinterpret_cast<LinkHeader*>(state_out);
        h->next_id = next0 + base_ws[G];
        h->count = cs;
        h->reid_dim = R;
    }
    double* opos = reinterpret_cast<double*>(state_out + state_pos_off());
    long long* otrack = reinterpret_cast<long long*>(state_out + state_track_off(state_out_cap));
    float* oemb = reinterpret_cast<float*>(state_out + state_emb_off(state_out_cap));
    for (int i = tid; i < 2 * cs; i += BLOCK) opos[i] = pos[2 * (size_t)v0 + i];
    for (int c = tid; c < cs; c += BLOCK) otrack[c] = s_track[c];
    for (size_t i = tid; i < (size_t)cs * R; i += BLOCK) oemb[i] = emb[(size_t)v0 * R + i];
}

static size_t round256(size_t bytes) { return bytes < 256 ? 256 : (bytes + 255) / 256 * 256; }

}  // namespace gnncca

using namespace gnncca;

extern "C" {

size_t gnncca_cluster_summaries_bytes(int64_t n_nodes, int64_t n_frames) {
    if (n_nodes < 0 || n_frames < 0) return 0;
    return round256((size_t)2 * (size_t)n_nodes * sizeof(int32_t));   // member order [N], first position of each cluster [N]
}

int gnncca_cluster_summaries(const int32_t* labels, const int32_t* node_ptr_dev, const double* xw, const double* yw, const int32_t* cam,
                             const float* embeds, int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes,
                             int32_t* count_out, int32_t* rank_out, int32_t* size_out, int32_t* n_cams_out, double* pos_out, float* emb_out,
                             void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    if (n_nodes < 0 || n_frames < 0 || reid_dim < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kTrackMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;
    if (!node_ptr_dev || !count_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!labels || !xw || !yw || !cam || !rank_out || !size_out || !n_cams_out || !pos_out)) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && reid_dim > 0 && (!embeds || !emb_out)) return GNNCCA_ERR_INVALID_ARG;
    if (workspace_bytes < gnncca_cluster_summaries_bytes(n_nodes, n_frames)) return GNNCCA_ERR_WORKSPACE;
    if (n_nodes >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    int P = 1;
    while (P < max_frame_nodes) P <<= 1;
    const size_t lds = (size_t)3 * P * sizeof(int);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* order_ws = static_cast<int*>(workspace);
    int* start_ws = order_ws + n_nodes;
#define GNNCCA_SUMMARIES(B)                                                                                                                 \
    hipLaunchKernelGGL((summaries_kernel<B>), dim3((unsigned)n_frames), dim3(B), lds, st, labels, (int)n_nodes, node_ptr_dev, xw, yw, cam, P, \
                       (int)max_frame_nodes, count_out, rank_out, size_out, n_cams_out, pos_out, order_ws, start_ws)
    if (P <= 64) GNNCCA_SUMMARIES(64);   // small frames (a Terrace frame has ~20 detections): one wave per frame
    else GNNCCA_SUMMARIES(256);
#undef GNNCCA_SUMMARIES
    HIP_TRY(hipGetLastError());
    if (reid_dim > 0 && max_frame_nodes > 0) {
        const unsigned tiles = (unsigned)((reid_dim + 255) / 256), slices = (unsigned)((max_frame_nodes + 15) / 16);
        hipLaunchKernelGGL(summaries_emb_kernel, dim3((unsigned)n_frames, tiles, slices), dim3(256), 0, st, embeds, (int)reid_dim, (int)n_nodes,
                           node_ptr_dev, count_out, size_out, order_ws, start_ws, emb_out);
        HIP_TRY(hipGetLastError());
    }
    return GNNCCA_OK;
}

size_t gnncca_link_state_bytes(int64_t capacity, int32_t reid_dim) {
    if (capacity < 0 || reid_dim < 0) return 0;
    return round256(state_emb_off(capacity) + (size_t)capacity * (size_t)reid_dim * sizeof(float));
}

size_t gnncca_link_workspace_bytes(int64_t n_nodes, int64_t n_frames) {
    if (n_nodes < 0 || n_frames < 0) return 0;
    // rank among the frame's unmatched clusters [N], unmatched clusters per frame [G], their exclusive prefix sum [G + 1]
    return round256(((size_t)n_nodes + 2 * (size_t)n_frames + 1) * sizeof(int32_t));
}

int gnncca_link_frames(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                       int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, double max_step, double lam,
                       int32_t has_max_cos, double max_cos, const void* state_in, int64_t state_in_capacity, void* state_out,
                       int64_t state_out_capacity, int64_t* cluster_track, int64_t* node_track, int32_t* matched_prev, void* workspace,
                       size_t workspace_bytes, gnncca_stream_t stream) {
    if (n_nodes < 0 || n_frames < 0 || reid_dim < 0 || state_in_capacity < 0 || state_out_capacity < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kTrackMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (state_in && state_in_capacity > kTrackMaxNodes) return GNNCCA_ERR_INVALID_ARG;
    LinkRule rule;
    if (!link_rule(max_step, lam, has_max_cos, max_cos, rule)) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;   // nothing to link: the caller keeps its state
    if (!node_ptr_dev || !count || !state_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!rank || !pos || !cluster_track || !node_track || !matched_prev)) return GNNCCA_ERR_INVALID_ARG;
    if (rule.need_emb && reid_dim > 0 && n_nodes > 0 && !emb) return GNNCCA_ERR_INVALID_ARG;
    if (workspace_bytes < gnncca_link_workspace_bytes(n_nodes, n_frames)) return GNNCCA_ERR_WORKSPACE;
    if (n_nodes >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    const int R = emb ? (int)reid_dim : 0;   // (without embeddings the state carries none)
    int P = 64;
    while (P < max_frame_nodes || (state_in && P < state_in_capacity)) P <<= 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* new_rank_ws = static_cast<int*>(workspace);
    int* n_new_ws = new_rank_ws + n_nodes;
    int* base_ws = n_new_ws + n_frames;
    const char* sin = static_cast<const char*>(state_in);
    hipLaunchKernelGGL((link_match_kernel<256>), dim3((unsigned)n_frames), dim3(256), (size_t)2 * P * sizeof(int), st, node_ptr_dev, (int)n_nodes,
                       count, pos, emb, R, rule, sin, (long long)state_in_capacity, P, matched_prev, new_rank_ws, n_new_ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(64), 0, st, n_new_ws, (int)n_frames, base_ws);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((link_ids_kernel<256>), dim3((unsigned)n_frames), dim3(256), (size_t)P * sizeof(long long), st, node_ptr_dev, (int)n_nodes,
                       count, rank, pos, emb, R, (int)n_frames, matched_prev, new_rank_ws, base_ws, sin, (long long)state_in_capacity,
                       static_cast<char*>(state_out), (long long)state_out_capacity, P, reinterpret_cast<long long*>(cluster_track),
                       reinterpret_cast<long long*>(node_track));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"

#include "identities_gap.cuh"   // gnncca_link_frames_gap: the gap-tolerant linker

#include "identities_assign.cuh"   // gnncca_link_frames_gap_ex: the level kernel's min-cost-assignment form (matching = 1)

#include "track_score.cuh"   // gnncca_track_score_*: identity-tracking scores over a sequence (its own kernels)

#include "identities_motion.cuh"   // gnncca_link_frames_motion: the gap-tolerant linker with a velocity prediction (one walking workgroup)

#include "identities_kalman.cuh"   // gnncca_link_frames_kalman: the same walk, predicting with and feeding a constant-velocity Kalman filter

#include "identities_reentry.cuh"   // gnncca_reentry_update: the gallery that gives a returning person the old identity back

#include "identities_smooth.cuh"   // gnncca_track_smooth: a constant-velocity Kalman filter along every track (chain-parallel)
