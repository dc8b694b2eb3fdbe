// graph_build.hip -- SURVEY.md 8f row N1 on gfx950: cross-camera graph construction + edge attributes for a batch of
// frames (replaces the per-frame Python / sklearn / GPU<->CPU round trips of inference.py:189-279).
//
// One wave per (SOURCE detection, slice of its frame's 64-candidate chunks), sources in the order the reference emits
// them (camera-major inside a frame).  A chunk is 64 consecutive detections of the frame, ONE PER LANE: the lane
// decides whether its candidate is on another camera (an edge, inference.py:210-211), and computes for it
//   ground-plane L2 and L1 distance in float64, divided by the frame's max_dist, cast to fp32   (inference.py:229-242)
//   the same-identity label                                                                     (inference.py:262-266)
// while the reid terms -- F.pairwise_distance(p=2, eps=1e-6), F.cosine_similarity(eps=1e-8)     (inference.py:222-226)
// -- are computed by the whole wave, four targets at a time: each target's reid row is one coalesced wave load, the
// 4 x 4 partial sums are reduced across the wave by a transposing butterfly (v_permlane32_swap, v_permlane16_swap,
// then 5 shuffles: 17 cross-lane ops for 16 sums instead of 96) and parked in the candidate's lane; sqrt / divide run
// once per chunk, lane-parallel.  The edge slot of a candidate is edge_ptr[source] + (other-camera candidates before
// it), a ballot prefix, so every store of edge_index / edge_attr / labels is a contiguous wave store in the
// reference's edge order.  Traffic: the reid table (N x R x 4 B) is re-read once per source from L2 -- it is 256 KB
// for a 256-detection frame -- and 8+8+16+4 B are written per edge; the kernel is L2/latency bound, not HBM bound.
//
// The selections that keep a part of these edges -- graph_topk.cuh, graph_topk_sym.cuh, graph_radius.cuh, included below -- decide WHICH
// candidates a source keeps in kernels of their own; what is computed and stored for a kept candidate is written once, here: EdgeSource /
// load_edge_source (the per-source context), emit_edges (label, attributes, slot, stores) and zero_counters.  On the host one function,
// build_edges_zeroing, checks the arguments and launches the kernel of an EdgeSelect (internal.h) for all three public entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "hip_try.h"
#include "wave_reduce.cuh"
#include "with_flag.h"

namespace gnncca {

typedef float f32x4g __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The arithmetic of an edge's attributes, used by emit_edges below and by the capped selections' keys (graph_topk.cuh).
// Ground-plane L2 and L1 distance of two detections in float64, no FMA contraction (sklearn paired_distances, inference.py:229-237):
__device__ __forceinline__ void ground_dists(double xi, double yi, double xj, double yj, double& l2, double& l1) {
    const double dx = __dsub_rn(xi, xj), dy = __dsub_rn(yi, yj);
    l2 = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
    l1 = __dadd_rn(fabs(dx), fabs(dy));
}
// F.pairwise_distance(p=2, eps=1e-6) and F.cosine_similarity(eps=1e-8) from reid_sums_wave's sums (inference.py:222-226):
__device__ __forceinline__ float reid_emb(float sd) { return sqrtf(sd); }
__device__ __forceinline__ float reid_cos(float sab, float saa, float sbb) {
    return sab / (fmaxf(sqrtf(saa), 1e-8f) * fmaxf(sqrtf(sbb), 1e-8f));
}

// The raw reid sums of source row `ri` against the candidates held by the lanes of `mask` (row_of(t): the reid row of lane t's
// candidate), computed by the whole wave, four candidates per round, and parked in each candidate's own lane:
//   sd = sum (a - b + 1e-6)^2,  sab = sum a b,  saa = sum a^2,  sbb = sum b^2      (a = ri[d], b = the candidate's row)
// A lane's partial sums run over d = lane, lane + 64, ... (or four adjacent columns per lane when R % 4 == 0) and the 64 partials
// are added by transpose_reduce16's fixed tree, whose pairing does not depend on the slot a candidate rides in: the bits of a
// candidate's sums depend on the two rows alone, not on which other candidates share its round (what lets gnncca_build_edges_topk
// re-group the survivors of a selection and still emit gnncca_build_edges' bits).
template <class RowOf>
__device__ __forceinline__ void reid_sums_wave(const float* __restrict__ reid, const float* __restrict__ ri, int R, bool vec4,
                                               unsigned long long mask, int lane, RowOf row_of, float& sd, float& sab, float& saa,
                                               float& sbb) {
    unsigned long long m = mask;
    while (m != 0ull) {  // wave-uniform: four targets per round (the last round repeats its last target)
        int t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (m != 0ull) {
                t[k] = __ffsll((long long)m) - 1;
                m &= m - 1;
            } else {
                t[k] = t[k - 1 < 0 ? 0 : k - 1];
            }
        }
        const float* __restrict__ rj[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) rj[k] = reid + (size_t)row_of(t[k]) * R;
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = 0.f;
        auto acc = [&](int k, float a, float b) {
            const float df = (a - b) + 1e-6f;  // F.pairwise_distance adds eps to the difference
            v[4 * k + 0] = fmaf(df, df, v[4 * k + 0]);
            v[4 * k + 1] = fmaf(a, b, v[4 * k + 1]);
            v[4 * k + 2] = fmaf(a, a, v[4 * k + 2]);
            v[4 * k + 3] = fmaf(b, b, v[4 * k + 3]);
        };
        if (vec4) {
            for (int d = lane * 4; d < R; d += 256) {
                const float4 a = *reinterpret_cast<const float4*>(ri + d);
                float4 b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = *reinterpret_cast<const float4*>(rj[k] + d);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    acc(k, a.x, b[k].x);
                    acc(k, a.y, b[k].y);
                    acc(k, a.z, b[k].z);
                    acc(k, a.w, b[k].w);
                }
            }
        } else {
            for (int d = lane; d < R; d += 64) {
                const float a = ri[d];
                float b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = rj[k][d];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc(k, a, b[k]);
            }
        }
        const int toti = __float_as_int(transpose_reduce16(v));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float s0 = __int_as_float(__builtin_amdgcn_readlane(toti, lane_of_sum(4 * k + 0)));
            const float s1 = __int_as_float(__builtin_amdgcn_readlane(toti, lane_of_sum(4 * k + 1)));
            const float s2 = __int_as_float(__builtin_amdgcn_readlane(toti, lane_of_sum(4 * k + 2)));
            const float s3 = __int_as_float(__builtin_amdgcn_readlane(toti, lane_of_sum(4 * k + 3)));
            if (lane == t[k]) sd = s0, sab = s1, saa = s2, sbb = s3;
        }
    }
}

// ---- what the four selections (dense here, graph_topk.cuh, graph_topk_sym.cuh, graph_radius.cuh) share on the device ----
// A kept edge carries the dense build's bits in every selection because all four kernels run emit_edges below: the statements exist once.

// What a wave knows of its source, the detection at position p of src_order: its frame [gs, ge) of graph g, camera, person, ground
// position, the frame's max_dist and its reid row.
struct EdgeSource {
    int i, g, gs, ge, ci, pi;
    double xi, yi, md;
    const float* __restrict__ ri;
    bool vec4;
};
__device__ __forceinline__ EdgeSource load_edge_source(const gnncca_frames& fr, const float* __restrict__ reid, int R, int p) {
    EdgeSource s;
    s.i = fr.src_order[p];
    s.g = fr.graph_of[s.i];
    s.gs = fr.graph_ptr[s.g], s.ge = fr.graph_ptr[s.g + 1];
    s.ci = fr.cam[s.i], s.pi = fr.person_id[s.i];
    s.xi = fr.xw[s.i], s.yi = fr.yw[s.i], s.md = fr.max_dist[s.g];
    s.ri = reid + (size_t)s.i * R;
    s.vec4 = (R & 3) == 0;
    return s;
}

// gnncca_frames_forward*: the post-processing counters of the same batch are zeroed by the build's launch, launches ahead of their first
// use, instead of by a memset node of their own -- ahead of the kernel's early returns (a wave without a source, or a source without a
// kept candidate, still does its share), by the workgroups with `mine`, `width` threads each.
__device__ __forceinline__ void zero_counters(int* __restrict__ zero_ptr, int zero_n, bool mine, int width) {
    if (zero_ptr && mine)
        for (int t = blockIdx.x * width + threadIdx.x; t < zero_n; t += gridDim.x * width) zero_ptr[t] = 0;
}

// The edges of one 64-candidate round of source `s`: this lane holds candidate j, kept iff `keep`; `mask` is the wave's ballot of keep
// (not zero) and row_of(t) the reid row of lane t's candidate (reid_sums_wave).  Label, ground attributes, reid terms, then the stores at
// slot k = base + (kept lanes below this one), so a round's stores are contiguous and in candidate order; a kept lane stores iff slot_ok(k).
template <int MODE, class RowOf, class SlotOk>
__device__ __forceinline__ void emit_edges(const gnncca_frames& fr, const float* __restrict__ reid, int R, const EdgeSource& s, int j, bool keep,
                                           unsigned long long mask, int lane, RowOf row_of, long long base, SlotOk slot_ok, long long E,
                                           long long* __restrict__ ei_out, float* __restrict__ attr_out, float* __restrict__ lab_out) {
    constexpr int NA = MODE == GNNCCA_EDGE_ATTR_FULL ? 4 : 2;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, lab = 0.f;
    if (keep) {
        lab = fr.person_id[j] == s.pi ? 1.f : 0.f;
        if (MODE != GNNCCA_EDGE_ATTR_ONLY_APPEARANCE) {
            // sklearn paired_distances on float64 rows, / max_dist, .type(float32); no FMA contraction
            double l2, l1;
            ground_dists(s.xi, s.yi, fr.xw[j], fr.yw[j], l2, l1);
            a0 = (float)__ddiv_rn(l2, s.md);
            a1 = (float)__ddiv_rn(l1, s.md);
        }
    }
    if (MODE != GNNCCA_EDGE_ATTR_ONLY_DIST) {
        float sd = 0.f, sab = 0.f, saa = 1.f, sbb = 1.f;  // this lane's candidate: raw sums over the reid row
        reid_sums_wave(reid, s.ri, R, s.vec4, mask, lane, row_of, sd, sab, saa, sbb);
        const float emb = reid_emb(sd), cosv = reid_cos(sab, saa, sbb);
        if (MODE == GNNCCA_EDGE_ATTR_FULL) {
            a2 = emb;
            a3 = cosv;
        } else {
            a0 = emb;
            a1 = cosv;
        }
    }
    if (keep) {
        const long long k = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (slot_ok(k)) {
            ei_out[k] = s.i;
            ei_out[E + k] = j;
            if (NA == 4) {
                *reinterpret_cast<float4*>(attr_out + k * 4) = make_float4(a0, a1, a2, a3);
            } else {
                *reinterpret_cast<float2*>(attr_out + k * 2) = make_float2(a0, a1);
            }
            lab_out[k] = lab;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void build_edges_kernel(const gnncca_frames fr, const float* __restrict__ reid, int R, int N,
                                                          long long E, long long* __restrict__ ei_out,
                                                          float* __restrict__ attr_out, float* __restrict__ lab_out,
                                                          int* __restrict__ zero_ptr, int zero_n) {
    zero_counters(zero_ptr, zero_n, blockIdx.y == 0, 256);
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= N) return;
    const EdgeSource s = load_edge_source(fr, reid, R, p);
    long long pos = fr.edge_ptr[p];
    for (int c = 0, j0 = s.gs; j0 < s.ge; ++c, j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < s.ge && fr.cam[j] != s.ci;  // same camera: no edge (inference.py:210-211)
        const unsigned long long mask = __ballot(valid);
        if (c % (int)gridDim.y == (int)blockIdx.y && mask != 0ull)
            emit_edges<MODE>(fr, reid, R, s, j, valid, mask, lane, [&](int t) { return j0 + t; }, pos, [](long long) { return true; }, E,
                             ei_out, attr_out, lab_out);
        pos += __popcll(mask);
    }
}

// Column norms of an [n_rows][n_cols] matrix (F.normalize(x, dim=0), inference.py:189-190), deterministic:
//   partial[chunk][c] = sum over the chunk's kColChunk rows of x[r][c]^2, rows in ascending order
//   norm[c]           = max(sqrt(sum over chunks, in four ordered quarters), 1e-12)
// The first version (256-row chunks, one dependent load per iteration, 512 workgroups) streamed the 2048-wide embedding
// matrix at 0.75 TB/s; here a thread owns four adjacent columns (16-B loads), eight rows are requested before they are
// squared and added (in order), and 64-row chunks put 4x as many workgroups on the chip.
constexpr int kColChunk = 64;
__global__ __launch_bounds__(256) void colnorm_partial_kernel(const float* __restrict__ x, long long n_rows, long long n_cols,
                                                              float* __restrict__ partial) {
    const long long r0 = (long long)blockIdx.y * kColChunk, r1 = min(r0 + kColChunk, n_rows);
    if ((n_cols & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
        if (c >= n_cols) return;
        f32x4g s = {0.f, 0.f, 0.f, 0.f};
        for (long long r = r0; r < r1; r += 8) {
            f32x4g v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4g*>(x + min(r + u, r1 - 1) * n_cols + c);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (r + u < r1)
#pragma unroll
                    for (int q = 0; q < 4; ++q) s[q] = fmaf(v[u][q], v[u][q], s[q]);
        }
        *reinterpret_cast<f32x4g*>(partial + (long long)blockIdx.y * n_cols + c) = s;
    } else {
        for (int q = 0; q < 4; ++q) {  // unaligned / odd widths: one column at a time
            const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) * 4 + q;
            if (c >= n_cols) return;
            float s = 0.f;
            for (long long r = r0; r < r1; ++r) {
                const float v = x[r * n_cols + c];
                s = fmaf(v, v, s);
            }
            partial[(long long)blockIdx.y * n_cols + c] = s;
        }
    }
}

// 64 columns per workgroup: thread (quarter q = tid / 64, column = tid % 64) sums its quarter of the chunks in order,
// eight loads in flight; the four quarter sums are then added in order.
__global__ __launch_bounds__(256) void colnorm_finish_kernel(float* __restrict__ partial, long long n_chunks, long long n_cols) {
    __shared__ float s_q[4][64];
    const int q = threadIdx.x >> 6, cl = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * 64 + cl;
    const long long per = (n_chunks + 3) / 4, k0 = min((long long)q * per, n_chunks), k1 = min(k0 + per, n_chunks);
    float s = 0.f;
    if (c < n_cols) {
        for (long long k = k0; k < k1; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[min(k + u, k1 - 1) * n_cols + c];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k + u < k1) s += v[u];
        }
    }
    s_q[q][cl] = s;
    __syncthreads();
    if (q == 0 && c < n_cols) {
        const float t = ((s_q[0][cl] + s_q[1][cl]) + s_q[2][cl]) + s_q[3][cl];
        partial[n_chunks * n_cols + c] = fmaxf(sqrtf(t), 1e-12f);  // F.normalize clamps the norm at eps = 1e-12
    }
}

__global__ __launch_bounds__(256) void colnorm_apply_kernel(const float* __restrict__ x, const float* __restrict__ norm,
                                                            long long total, long long n_cols, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < total) out[t] = x[t] / norm[t % n_cols];
}

// The three kernels above in ONE launch, for the matrices of a batch of frames (a few thousand rows: the launches, not the bytes, are
// what the per-batch pipeline pays for) and for up to two matrices at once (reid and node embeddings).  A workgroup owns 16 adjacent
// columns of one matrix (144 workgroups for 2048 + 256 columns): (1) chunk sums -- thread (chunk lane = tid / 4, four columns = tid % 4)
// runs colnorm_partial_kernel's fma chain over its 64-row chunks, sixteen rows requested before the first is used -> LDS;
// (2) colnorm_finish_kernel's four ordered quarter sums and the clamp; (3) the division, rows strided over the chunk lanes, eight in
// flight.  Same operations in the same order as the three-kernel form: the results are bit for bit the same.
// (First form: 32 columns per workgroup, eight rows in flight, one row per iteration in (3): 23.6 us for a 1229-row batch, a quarter of
// the Terrace pipeline's GPU time.)
constexpr int kFusedMaxChunks = 64;   // rows <= 4096
constexpr int kFusedCols = 16;
struct ColnormJob {
    const float* x;
    float* out;
    long long n_cols;
    int first_block;   // workgroups [first_block, first_block + ceil(n_cols / 16)) belong to this matrix
};
__global__ __launch_bounds__(256) void colnorm_fused_kernel(const ColnormJob j0, const ColnormJob j1, long long n_rows) {
    __shared__ float s_part[kFusedMaxChunks][kFusedCols];
    __shared__ float s_q[4][kFusedCols];
    __shared__ float s_norm[kFusedCols];
    const bool second = j1.x != nullptr && (int)blockIdx.x >= j1.first_block;
    const ColnormJob& j = second ? j1 : j0;
    const long long n_cols = j.n_cols;
    const float* __restrict__ x = j.x;
    const int tid = threadIdx.x, cl = tid >> 2, cg = tid & 3;
    const long long c0 = (long long)((int)blockIdx.x - j.first_block) * kFusedCols;
    const long long c = c0 + 4 * cg;
    const int n_chunks = (int)((n_rows + kColChunk - 1) / kColChunk);
    const bool vec = (n_cols & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(j.out) & 15) == 0;
    for (int ch = cl; ch < n_chunks; ch += 64) {
        const long long r0 = (long long)ch * kColChunk, r1 = min(r0 + kColChunk, n_rows);
        f32x4g s = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            if (c < n_cols)
                for (long long r = r0; r < r1; r += 16) {
                    f32x4g v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const f32x4g*>(x + min(r + u, r1 - 1) * n_cols + c);
#pragma unroll
                    for (int u = 0; u < 16; ++u)
                        if (r + u < r1)
#pragma unroll
                            for (int q = 0; q < 4; ++q) s[q] = fmaf(v[u][q], v[u][q], s[q]);
                }
        } else {
            for (int q = 0; q < 4; ++q)
                if (c + q < n_cols)
                    for (long long r = r0; r < r1; ++r) {
                        const float v = x[r * n_cols + c + q];
                        s[q] = fmaf(v, v, s[q]);
                    }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) s_part[ch][4 * cg + q] = s[q];
    }
    __syncthreads();
    if (tid < 4 * kFusedCols) {
        const int q = tid / kFusedCols, col = tid % kFusedCols;
        const int per = (n_chunks + 3) / 4, k0 = min(q * per, n_chunks), k1 = min(k0 + per, n_chunks);
        float t = 0.f;
        for (int k = k0; k < k1; ++k) t += s_part[k][col];
        s_q[q][col] = t;
    }
    __syncthreads();
    if (tid < kFusedCols) s_norm[tid] = fmaxf(sqrtf(((s_q[0][tid] + s_q[1][tid]) + s_q[2][tid]) + s_q[3][tid]), 1e-12f);
    __syncthreads();
    float* __restrict__ out = j.out;
    if (vec) {
        if (c < n_cols) {
            const f32x4g nv = {s_norm[4 * cg], s_norm[4 * cg + 1], s_norm[4 * cg + 2], s_norm[4 * cg + 3]};
            for (long long r = cl; r < n_rows; r += 64 * 8) {
                f32x4g v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4g*>(x + min(r + 64 * u, n_rows - 1) * n_cols + c);
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (r + 64 * u < n_rows)
                        *reinterpret_cast<f32x4g*>(out + (r + 64 * u) * n_cols + c) = f32x4g{v[u][0] / nv[0], v[u][1] / nv[1], v[u][2] / nv[2], v[u][3] / nv[3]};
            }
        }
    } else {
        for (int q = 0; q < 4; ++q)
            if (c + q < n_cols)
                for (long long r = cl; r < n_rows; r += 64) out[r * n_cols + c + q] = x[r * n_cols + c + q] / s_norm[4 * cg + q];
    }
}

// The same, for batches whose 16-column strip fits LDS (n_rows <= kLdsRowsMax: every batch of 64 Terrace frames): the strip is read from
// memory ONCE, by LDS-DMA (`buffer_load_dwordx4 ... lds`: 16 rows x 64 B per wave instruction, every request of the workgroup in flight
// at once, no VGPR staging), and both passes -- the chunk sums and the division -- run from LDS.  The kernel above walks its strip twice
// with 16 / 8 requests in flight per thread, and its first pass keeps 4 x ceil(rows / 64) of its 256 threads busy (72 for a 1100-row
// batch): 16.5 us for 10 MB in a pipeline whose kernels sum to 80.  Same operations in the same order: the same bits.
// LDS image: chunk ch (64 rows) at ch * kLdsChunkBytes, row-major [64][16] floats, 64 B of padding behind every chunk -- the chunk lanes
// of pass one then start 64 B apart modulo the 256-B bank row (no conflicts between the sixteen lanes of a ds_read_b128 pass).
constexpr int kLdsChunkBytes = kColChunk * kFusedCols * 4 + 64;
constexpr int kLdsRowsMax = 2304;   // 36 chunks: 149 760 B next to the 4.4 KB of static LDS
typedef __attribute__((address_space(3))) void* gb_lds_ptr;
__global__ __launch_bounds__(256) void colnorm_fused_lds_kernel(const ColnormJob j0, const ColnormJob j1, long long n_rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_strip[];
    __shared__ float s_part[kFusedMaxChunks][kFusedCols];
    __shared__ float s_q[4][kFusedCols];
    __shared__ float s_norm[kFusedCols];
    const bool second = j1.x != nullptr && (int)blockIdx.x >= j1.first_block;
    const ColnormJob& j = second ? j1 : j0;
    const int n_cols = (int)j.n_cols;
    const int tid = threadIdx.x, lane = tid & 63, cl = tid >> 2, cg = tid & 3;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = ((int)blockIdx.x - j.first_block) * kFusedCols;
    const int c = c0 + 4 * cg;
    const int rows = (int)n_rows;
    const int n_chunks = (rows + kColChunk - 1) / kColChunk;
    // (the host checked: 16-byte aligned matrices, n_cols % 4 == 0, n_rows * n_cols * 4 < 2^31; rows beyond the matrix read as zeros)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(j.x), 0, (int)((unsigned)rows * (unsigned)n_cols * 4u), 0x00020000);
    const unsigned col_ok = c < n_cols ? 0u : 0x80000000u;   // column groups beyond the matrix: out of range (zeros), never used
    const int n_groups = (rows + 15) / 16;
    for (int g = wave; g < n_groups; g += 4) {
        const unsigned voff = ((unsigned)(16 * g + (lane >> 2)) * (unsigned)n_cols + (unsigned)c) * 4u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (gb_lds_ptr)(s_strip + (g >> 2) * kLdsChunkBytes + (g & 3) * 1024), 16, voff | col_ok, 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int ch = cl; ch < n_chunks; ch += 64) {
        const int r0 = ch * kColChunk, r1 = min(r0 + kColChunk, rows);
        const unsigned char* base = s_strip + ch * kLdsChunkBytes + cg * 16;
        f32x4g s = {0.f, 0.f, 0.f, 0.f};
        for (int r = r0; r < r1; r += 16) {
            f32x4g v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const f32x4g*>(base + (min(r + u, r1 - 1) - r0) * (kFusedCols * 4));
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (r + u < r1)
#pragma unroll
                    for (int q = 0; q < 4; ++q) s[q] = fmaf(v[u][q], v[u][q], s[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) s_part[ch][4 * cg + q] = s[q];
    }
    __syncthreads();
    if (tid < 4 * kFusedCols) {
        const int q = tid / kFusedCols, col = tid % kFusedCols;
        const int per = (n_chunks + 3) / 4, k0 = min(q * per, n_chunks), k1 = min(k0 + per, n_chunks);
        float t = 0.f;
        for (int k = k0; k < k1; ++k) t += s_part[k][col];
        s_q[q][col] = t;
    }
    __syncthreads();
    if (tid < kFusedCols) s_norm[tid] = fmaxf(sqrtf(((s_q[0][tid] + s_q[1][tid]) + s_q[2][tid]) + s_q[3][tid]), 1e-12f);
    __syncthreads();
    if (c < n_cols) {
        const f32x4g nv = {s_norm[4 * cg], s_norm[4 * cg + 1], s_norm[4 * cg + 2], s_norm[4 * cg + 3]};
        float* __restrict__ out = j.out;
        for (int r = cl; r < rows; r += 64) {   // (tid & 3 == cg for every piece of this thread: 256 % 4 == 0)
            const f32x4g v = *reinterpret_cast<const f32x4g*>(s_strip + (r >> 6) * kLdsChunkBytes + (r & 63) * (kFusedCols * 4) + cg * 16);
            *reinterpret_cast<f32x4g*>(out + (size_t)r * n_cols + c) = f32x4g{v[0] / nv[0], v[1] / nv[1], v[2] / nv[2], v[3] / nv[3]};
        }
    }
}

}  // namespace gnncca

#include "graph_grads.cuh"
#include "graph_topk.cuh"
#include "graph_topk_sym.cuh"
#include "graph_radius.cuh"

using namespace gnncca;

// ---- what the host code of the edge entry points shares ----
// The template arguments of a launch chosen at run time: f(std::integral_constant<int, MODE>) for the edge-attribute mode (the callers have
// checked its range), f(std::true_type / std::false_type) for a flag (with_flag.h).
template <class F>
static void with_mode(int32_t mode, F&& f) {
    switch (mode) {
        case GNNCCA_EDGE_ATTR_FULL: f(std::integral_constant<int, GNNCCA_EDGE_ATTR_FULL>{}); break;
        case GNNCCA_EDGE_ATTR_ONLY_APPEARANCE: f(std::integral_constant<int, GNNCCA_EDGE_ATTR_ONLY_APPEARANCE>{}); break;
        default: f(std::integral_constant<int, GNNCCA_EDGE_ATTR_ONLY_DIST>{}); break;
    }
}
template <class Ground>
constexpr int rank_of(Ground) { return Ground::value ? GNNCCA_RANK_BY_GROUND : GNNCCA_RANK_BY_REID; }   // (the callers have checked rank_by)

// Launch geometry of the capped kernels (graph_topk.cuh, graph_topk_sym.cuh): a wave per source, whose LDS holds the keys of `cap` candidates.
struct TopkGeometry { int cap; size_t lds_bytes; dim3 grid, block; };
static TopkGeometry topk_geometry(int32_t max_deg, int64_t n_nodes) {
    const int cap = std::max(64, (max_deg + 63) / 64 * 64);
    const size_t per_wave = (size_t)cap * kTopkSlotBytes;
    const int waves = per_wave * 4 <= 65536 ? 4 : (per_wave * 2 <= 65536 ? 2 : 1);   // 4096 slots x 12 B = 48 KB: one wave
    return TopkGeometry{cap, per_wave * waves, dim3((unsigned)((n_nodes + waves - 1) / waves)), dim3(64 * waves)};
}

// Two refusals (GNNCCA_ERR_INVALID_ARG) that the build (every selection), the symmetric emit and the backward entry points state alike.  What
// lies between them keeps each entry point's own order, which the tests pin: the build refuses its selection's arguments (max_deg, the radius)
// before its early return for an empty batch, the symmetric emit checks the 2^31 limits and its workspace before that return; the symmetric
// count has no n_edges and stays apart.
static bool edge_sizes_invalid(const gnncca_frames* fr, int64_t n_nodes, int64_t n_edges, int32_t reid_dim, int32_t mode) {
    return !fr || n_nodes < 0 || n_edges < 0 || reid_dim < 0 || mode < GNNCCA_EDGE_ATTR_FULL || mode > GNNCCA_EDGE_ATTR_ONLY_DIST;
}
static bool edge_pointers_null(const gnncca_frames* fr, const void* edge_index_out, const void* edge_attr_out, const void* edge_labels_out) {
    return !fr->xw || !fr->yw || !fr->max_dist || !fr->person_id || !fr->cam || !fr->graph_of || !fr->graph_ptr || !fr->src_order ||
           !fr->edge_ptr || !edge_index_out || !edge_attr_out || !edge_labels_out;
}

// radius: a number >= 0 or +inf (a NaN fails the comparison); unit: one of GNNCCA_RADIUS_UNIT_*
static bool radius_invalid(double radius, int32_t unit) {
    return !(radius >= 0.0) || (unit != GNNCCA_RADIUS_UNIT_GROUND && unit != GNNCCA_RADIUS_UNIT_MAX_DIST);
}

// What a selection refuses of its own arguments (internal.h): stated by every entry point that takes one before it looks at the sizes --
// the build before its early return for an empty batch, gnncca_frames_forward_* before the normalisation's launch.
int gnncca::edge_select_refusal(const EdgeSelect& sel) {
    if (sel.kind == EdgeSelect::kCapped) {
        if (sel.top_k < 1 || sel.max_deg < 0 || (sel.rank_by != GNNCCA_RANK_BY_GROUND && sel.rank_by != GNNCCA_RANK_BY_REID)) return GNNCCA_ERR_INVALID_ARG;
        if (sel.max_deg > GNNCCA_TOPK_MAX_DEG) return GNNCCA_ERR_UNSUPPORTED;   // one wave's LDS holds the keys of at most that many candidates
    }
    if (sel.kind == EdgeSelect::kGated && radius_invalid(sel.radius, sel.unit)) return GNNCCA_ERR_INVALID_ARG;
    return GNNCCA_OK;
}

extern "C" {

int gnncca_normalize_columns2(const float* x0, int64_t n_cols0, float* out0, const float* x1, int64_t n_cols1, float* out1, int64_t n_rows,
                              gnncca_stream_t stream) {
    if (n_rows < 0 || n_cols0 < 0 || n_cols1 < 0) return GNNCCA_ERR_INVALID_ARG;
    if ((n_rows + kColChunk - 1) / kColChunk > kFusedMaxChunks) return GNNCCA_ERR_UNSUPPORTED;
    if (n_rows == 0) return GNNCCA_OK;
    if ((n_cols0 > 0 && (!x0 || !out0)) || (n_cols1 > 0 && (!x1 || !out1))) return GNNCCA_ERR_INVALID_ARG;
    if (n_cols0 == 0) x0 = x1, out0 = out1, n_cols0 = n_cols1, n_cols1 = 0;
    if (n_cols0 == 0) return GNNCCA_OK;
    const long long b0 = (n_cols0 + kFusedCols - 1) / kFusedCols, b1 = (n_cols1 + kFusedCols - 1) / kFusedCols;
    if (b0 + b1 >= (1ll << 31)) return GNNCCA_ERR_UNSUPPORTED;
    ColnormJob j0{x0, out0, (long long)n_cols0, 0};
    ColnormJob j1{n_cols1 > 0 ? x1 : nullptr, out1, (long long)n_cols1, (int)b0};
    // the LDS-resident form where the strip fits and both matrices allow 16-byte accesses through 32-bit offsets
    auto vec_ok = [&](const float* x, const float* out, int64_t nc) {
        return nc == 0 || ((nc & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                           (long long)n_rows * nc * 4 < (1ll << 31));
    };
    static const bool no_lds = diag_env("GNNCCA_COLNORM_NOLDS") != nullptr;   // diagnostics: A/B against the two-pass form
    if (!no_lds && n_rows <= kLdsRowsMax && vec_ok(x0, out0, n_cols0) && vec_ok(x1, out1, n_cols1)) {
        const int lds = (int)((n_rows + kColChunk - 1) / kColChunk) * kLdsChunkBytes;
        HIP_TRY(lds_opt_in<colnorm_fused_lds_kernel>((kLdsRowsMax / kColChunk) * kLdsChunkBytes));
        hipLaunchKernelGGL(colnorm_fused_lds_kernel, dim3((unsigned)(b0 + b1)), dim3(256), (size_t)lds, static_cast<hipStream_t>(stream), j0, j1,
                           (long long)n_rows);
    } else {
        hipLaunchKernelGGL(colnorm_fused_kernel, dim3((unsigned)(b0 + b1)), dim3(256), 0, static_cast<hipStream_t>(stream), j0, j1, (long long)n_rows);
    }
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_normalize_columns(const float* x, int64_t n_rows, int64_t n_cols, float* scratch, float* out, gnncca_stream_t stream) {
    if (n_rows < 0 || n_cols < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n_rows == 0 || n_cols == 0) return GNNCCA_OK;
    if (!x || !scratch || !out) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long chunks = (n_rows + kColChunk - 1) / kColChunk;
    if (chunks > 65535) return GNNCCA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(colnorm_partial_kernel, dim3((unsigned)((n_cols + 1023) / 1024), (unsigned)chunks), dim3(256), 0, st, x,
                       (long long)n_rows, (long long)n_cols, scratch);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(colnorm_finish_kernel, dim3((unsigned)((n_cols + 63) / 64)), dim3(256), 0, st, scratch, chunks,
                       (long long)n_cols);
    HIP_TRY(hipGetLastError());
    const long long total = (long long)n_rows * n_cols;
    hipLaunchKernelGGL(colnorm_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x,
                       (const float*)(scratch + chunks * n_cols), total, (long long)n_cols, out);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

// ---- backward of row N1 (graph_grads.cuh) ----
size_t gnncca_build_edges_backward_bytes(int64_t n_nodes) { return n_nodes > 0 ? (size_t)n_nodes * sizeof(NodeAux) : 0; }

// `edge_index` null: the dense enumeration (gnncca_build_edges); else the pruned edge list of gnncca_build_edges_topk
static int edges_backward(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges, int32_t mode,
                          const int64_t* edge_index, bool pruned, const float* edge_attr, const float* grad_edge_attr, void* workspace,
                          size_t workspace_bytes, float* grad_reid_out, gnncca_stream_t stream) {
    if (edge_sizes_invalid(fr, n_nodes, n_edges, reid_dim, mode)) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes == 0 || reid_dim == 0) return GNNCCA_OK;
    if (!grad_reid_out) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_edges == 0 || mode == GNNCCA_EDGE_ATTR_ONLY_DIST) {   // no edge attribute depends on the reid table: zeros, nothing launched
        HIP_TRY(hipMemsetAsync(grad_reid_out, 0, (size_t)n_nodes * (size_t)reid_dim * sizeof(float), st));
        return GNNCCA_OK;
    }
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    if (!fr->cam || !fr->graph_of || !fr->graph_ptr || !fr->src_order || !fr->edge_ptr || !reid || !edge_attr || !grad_edge_attr || !workspace)
        return GNNCCA_ERR_INVALID_ARG;
    if (pruned && !edge_index) return GNNCCA_ERR_INVALID_ARG;
    if (workspace_bytes < gnncca_build_edges_backward_bytes(n_nodes)) return GNNCCA_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return GNNCCA_ERR_INVALID_ARG;
    NodeAux* aux = static_cast<NodeAux*>(workspace);
    hipLaunchKernelGGL(edges_bwd_prep_kernel, dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, st, *fr, reid, (int)reid_dim, (int)n_nodes, aux);
    HIP_TRY(hipGetLastError());
    const bool vec = (reid_dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(reid) | reinterpret_cast<uintptr_t>(grad_reid_out)) & 15) == 0;
    const int per_block = kGgThreads * (vec ? 4 : 1);
    const dim3 grid((unsigned)((n_nodes + kGgRows - 1) / kGgRows), (unsigned)((reid_dim + per_block - 1) / per_block)), block(kGgThreads);
    if (grid.y > 65535) return GNNCCA_ERR_UNSUPPORTED;
    const long long* dst = pruned ? reinterpret_cast<const long long*>(edge_index) + n_edges : nullptr;
    with_mode(mode, [&](auto M) { with_flag(pruned, [&](auto P) { with_flag(vec, [&](auto V) {
        if constexpr (M() != GNNCCA_EDGE_ATTR_ONLY_DIST)   // (returned above: the kernel has no such instance)
            hipLaunchKernelGGL((edges_bwd_kernel<M(), V(), P()>), grid, block, 0, st, *fr, reid, (int)reid_dim, (int)n_nodes, (long long)n_edges,
                               aux, edge_attr, grad_edge_attr, dst, grad_reid_out);
    }); }); });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_build_edges_backward(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges, int32_t mode,
                                const float* edge_attr, const float* grad_edge_attr, void* workspace, size_t workspace_bytes,
                                float* grad_reid_out, gnncca_stream_t stream) {
    return edges_backward(fr, reid, reid_dim, n_nodes, n_edges, mode, nullptr, false, edge_attr, grad_edge_attr, workspace, workspace_bytes,
                          grad_reid_out, stream);
}

size_t gnncca_build_edges_topk_backward_bytes(int64_t n_nodes) { return gnncca_build_edges_backward_bytes(n_nodes); }

int gnncca_build_edges_topk_backward(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges,
                                     int32_t mode, const int64_t* edge_index, const float* edge_attr, const float* grad_edge_attr,
                                     void* workspace, size_t workspace_bytes, float* grad_reid_out, gnncca_stream_t stream) {
    return edges_backward(fr, reid, reid_dim, n_nodes, n_edges, mode, edge_index, true, edge_attr, grad_edge_attr, workspace, workspace_bytes,
                          grad_reid_out, stream);
}

// ---- row N1 with a capped neighbourhood (graph_topk.cuh) ----
int gnncca_build_edges_topk(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges, int32_t mode,
                            int32_t top_k, int32_t rank_by, int32_t max_deg, int64_t* edge_index_out, float* edge_attr_out,
                            float* edge_labels_out, gnncca_stream_t stream) {
    return gnncca::build_edges_zeroing(fr, reid, reid_dim, n_nodes, n_edges, mode, EdgeSelect::capped(top_k, rank_by, max_deg), edge_index_out,
                                       edge_attr_out, edge_labels_out, nullptr, 0, stream);
}

// ---- row N1 with a ground-plane gate (graph_radius.cuh) ----
int gnncca_build_edges_radius(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges, int32_t mode,
                              double radius, int32_t unit, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                              gnncca_stream_t stream) {
    return gnncca::build_edges_zeroing(fr, reid, reid_dim, n_nodes, n_edges, mode, EdgeSelect::gated(radius, unit), edge_index_out, edge_attr_out,
                                       edge_labels_out, nullptr, 0, stream);
}

// ---- the capped neighbourhood closed under reversal (graph_topk_sym.cuh) ----
size_t gnncca_build_edges_topk_sym_bytes(const int64_t* graph_sizes, int64_t n_frames) {
    if (n_frames < 0 || (n_frames > 0 && !graph_sizes)) return 0;
    long long nodes = 0;
    const long long words = topk_sym_words(graph_sizes, n_frames, &nodes);
    if (words < 0) return 0;
    const size_t bytes = (size_t)words * 16 + (size_t)nodes * sizeof(int32_t);
    return bytes < 16 ? 16 : (bytes + 15) / 16 * 16;
}

// what both entry points check of the frame sizes and the workspace; *words_out: words of one bit matrix
static int topk_sym_layout(const int64_t* graph_sizes, int64_t n_frames, int64_t n_nodes, const void* workspace, size_t workspace_bytes,
                           long long* words_out) {
    if (n_frames < 0 || (n_frames > 0 && !graph_sizes)) return GNNCCA_ERR_INVALID_ARG;
    long long nodes = 0;
    const long long words = topk_sym_words(graph_sizes, n_frames, &nodes);
    if (words < 0 || nodes != n_nodes) return GNNCCA_ERR_INVALID_ARG;   // graph_sizes do not describe these n_nodes detections
    if (n_frames >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return GNNCCA_ERR_INVALID_ARG;
    if (workspace_bytes < gnncca_build_edges_topk_sym_bytes(graph_sizes, n_frames)) return GNNCCA_ERR_WORKSPACE;
    *words_out = words;
    return GNNCCA_OK;
}

int gnncca_build_edges_topk_sym_count(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                      const int64_t* graph_sizes, int64_t n_frames, int32_t top_k, int32_t rank_by, int32_t max_deg,
                                      int32_t symmetric, void* workspace, size_t workspace_bytes, int32_t* edge_ptr_g_dev,
                                      gnncca_stream_t stream) {
    if (!fr || n_nodes < 0 || reid_dim < 0 || top_k < 1 || max_deg < 0) return GNNCCA_ERR_INVALID_ARG;
    if (rank_by != GNNCCA_RANK_BY_GROUND && rank_by != GNNCCA_RANK_BY_REID) return GNNCCA_ERR_INVALID_ARG;
    if (symmetric != GNNCCA_SYMMETRIC_UNION && symmetric != GNNCCA_SYMMETRIC_MUTUAL) return GNNCCA_ERR_INVALID_ARG;
    if (max_deg > GNNCCA_TOPK_MAX_DEG) return GNNCCA_ERR_UNSUPPORTED;   // one wave's LDS holds the keys of at most that many candidates
    if (n_nodes >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    if (!fr->xw || !fr->yw || !fr->cam || !fr->graph_of || !fr->graph_ptr || !fr->src_order || !fr->edge_ptr || !edge_ptr_g_dev)
        return GNNCCA_ERR_INVALID_ARG;
    if (rank_by == GNNCCA_RANK_BY_REID && (!reid || reid_dim == 0)) return GNNCCA_ERR_INVALID_ARG;
    long long words = 0;
    if (const int bad = topk_sym_layout(graph_sizes, n_frames, n_nodes, workspace, workspace_bytes, &words)) return bad;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* bits_a = static_cast<unsigned long long*>(workspace);
    unsigned long long* bits_b = bits_a + words;
    int* counts = reinterpret_cast<int*>(bits_b + words);
    int* edge_ptr = const_cast<int*>(fr->edge_ptr);   // the staging image's own words: the plan's capped values are replaced
    if (n_nodes > 0) {
        const TopkGeometry geo = topk_geometry(max_deg, n_nodes);
        with_flag(rank_by == GNNCCA_RANK_BY_GROUND, [&](auto ground) {
            hipLaunchKernelGGL((topk_sym_select_kernel<rank_of(ground)>), geo.grid, geo.block, geo.lds_bytes, st, *fr, reid, (int)reid_dim, (int)n_nodes,
                               (int)top_k, geo.cap, bits_a, words);
        });
        HIP_TRY(hipGetLastError());
        const dim3 grid4((unsigned)((n_nodes + 3) / 4));
        with_flag(symmetric == GNNCCA_SYMMETRIC_UNION, [&](auto U) {
            hipLaunchKernelGGL((topk_sym_close_kernel<U()>), grid4, dim3(256), 0, st, *fr, (int)n_nodes, bits_a, bits_b, words, counts);
        });
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(topk_sym_scan_kernel, dim3(1), dim3(256), 0, st, counts, (int)n_nodes, (int)n_frames, fr->graph_ptr, edge_ptr,
                       edge_ptr_g_dev);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_build_edges_topk_sym_emit(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes,
                                     const int64_t* graph_sizes, int64_t n_frames, int64_t n_edges, int32_t mode, const void* workspace,
                                     size_t workspace_bytes, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                                     gnncca_stream_t stream) {
    if (edge_sizes_invalid(fr, n_nodes, n_edges, reid_dim, mode)) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    long long words = 0;
    if (const int bad = topk_sym_layout(graph_sizes, n_frames, n_nodes, workspace, workspace_bytes, &words)) return bad;
    if (n_nodes == 0 || n_edges == 0) return GNNCCA_OK;
    if (edge_pointers_null(fr, edge_index_out, edge_attr_out, edge_labels_out)) return GNNCCA_ERR_INVALID_ARG;
    if (mode != GNNCCA_EDGE_ATTR_ONLY_DIST && (!reid || reid_dim == 0)) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned long long* bits_b = static_cast<const unsigned long long*>(workspace) + words;
    long long* ei = reinterpret_cast<long long*>(edge_index_out);
    const dim3 grid((unsigned)((n_nodes + 3) / 4)), block(256);
    with_mode(mode, [&](auto M) {
        hipLaunchKernelGGL((topk_sym_emit_kernel<M()>), grid, block, 0, st, *fr, reid, (int)reid_dim, (int)n_nodes, (long long)n_edges, bits_b,
                           words, ei, edge_attr_out, edge_labels_out);
    });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

size_t gnncca_normalize_columns_backward_bytes(int64_t n_rows, int64_t n_cols) {
    if (n_rows <= 0 || n_cols <= 0) return 0;
    return (size_t)(2 * ((n_rows + kColChunk - 1) / kColChunk + 1) * n_cols) * sizeof(float);
}

int gnncca_normalize_columns_backward(const float* x, const float* grad_out, int64_t n_rows, int64_t n_cols, void* scratch, size_t scratch_bytes,
                                      float* grad_x, gnncca_stream_t stream) {
    if (n_rows < 0 || n_cols < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n_rows == 0 || n_cols == 0) return GNNCCA_OK;
    if (!x || !grad_out || !scratch || !grad_x) return GNNCCA_ERR_INVALID_ARG;
    if (scratch_bytes < gnncca_normalize_columns_backward_bytes(n_rows, n_cols)) return GNNCCA_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long chunks = (n_rows + kColChunk - 1) / kColChunk;
    if (chunks > 65535) return GNNCCA_ERR_UNSUPPORTED;
    float* sq = static_cast<float*>(scratch);
    float* dot = sq + (chunks + 1) * n_cols;
    hipLaunchKernelGGL(colnorm_bwd_partial_kernel, dim3((unsigned)((n_cols + 1023) / 1024), (unsigned)chunks), dim3(256), 0, st, x, grad_out,
                       (long long)n_rows, (long long)n_cols, sq, dot);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(colnorm_bwd_finish_kernel, dim3((unsigned)((n_cols + 63) / 64)), dim3(256), 0, st, sq, dot, chunks, (long long)n_cols);
    HIP_TRY(hipGetLastError());
    const long long total = (long long)n_rows * n_cols;
    hipLaunchKernelGGL(colnorm_bwd_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, grad_out,
                       (const float*)(sq + chunks * n_cols), (const float*)(dot + chunks * n_cols), total, (long long)n_cols, grad_x);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_normalize_columns_backward2(const float* x0, const float* grad_out0, int64_t n_cols0, float* grad_x0, const float* x1,
                                       const float* grad_out1, int64_t n_cols1, float* grad_x1, int64_t n_rows, gnncca_stream_t stream) {
    if (n_rows < 0 || n_cols0 < 0 || n_cols1 < 0) return GNNCCA_ERR_INVALID_ARG;
    if ((n_rows + kColChunk - 1) / kColChunk > kFusedMaxChunks) return GNNCCA_ERR_UNSUPPORTED;
    if (n_rows == 0) return GNNCCA_OK;
    if ((n_cols0 > 0 && (!x0 || !grad_out0 || !grad_x0)) || (n_cols1 > 0 && (!x1 || !grad_out1 || !grad_x1))) return GNNCCA_ERR_INVALID_ARG;
    if (n_cols0 == 0) x0 = x1, grad_out0 = grad_out1, grad_x0 = grad_x1, n_cols0 = n_cols1, n_cols1 = 0;
    if (n_cols0 == 0) return GNNCCA_OK;
    const long long b0 = (n_cols0 + kFusedCols - 1) / kFusedCols, b1 = (n_cols1 + kFusedCols - 1) / kFusedCols;
    if (b0 + b1 >= (1ll << 31)) return GNNCCA_ERR_UNSUPPORTED;
    ColnormBwdJob j0{x0, grad_out0, grad_x0, (long long)n_cols0, 0};
    ColnormBwdJob j1{n_cols1 > 0 ? x1 : nullptr, grad_out1, grad_x1, (long long)n_cols1, (int)b0};
    hipLaunchKernelGGL(colnorm_bwd_fused_kernel, dim3((unsigned)(b0 + b1)), dim3(256), 0, static_cast<hipStream_t>(stream), j0, j1, (long long)n_rows);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_build_edges(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges,
                       int32_t mode, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out,
                       gnncca_stream_t stream) {
    return gnncca::build_edges_zeroing(fr, reid, reid_dim, n_nodes, n_edges, mode, EdgeSelect::dense(), edge_index_out, edge_attr_out,
                                       edge_labels_out, nullptr, 0, stream);
}

}  // extern "C"

// gnncca_build_edges, gnncca_build_edges_topk and gnncca_build_edges_radius, and the build of gnncca_frames_forward_* (zero_ptr: the post
// stage's counters).  The selection's own refusals stand where the capped and the gated entry stated them: before the early return for an
// empty batch.
int gnncca::build_edges_zeroing(const gnncca_frames* fr, const float* reid, int32_t reid_dim, int64_t n_nodes, int64_t n_edges, int32_t mode,
                                const EdgeSelect& sel, int64_t* edge_index_out, float* edge_attr_out, float* edge_labels_out, int32_t* zero_ptr,
                                int64_t zero_n, gnncca_stream_t stream) {
    if (edge_sizes_invalid(fr, n_nodes, n_edges, reid_dim, mode)) return GNNCCA_ERR_INVALID_ARG;
    if (const int bad = edge_select_refusal(sel)) return bad;
    if (n_nodes == 0 || n_edges == 0) return GNNCCA_OK;
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    if (edge_pointers_null(fr, edge_index_out, edge_attr_out, edge_labels_out)) return GNNCCA_ERR_INVALID_ARG;
    const bool capped = sel.kind == EdgeSelect::kCapped;
    const bool reads_reid = mode != GNNCCA_EDGE_ATTR_ONLY_DIST || (capped && sel.rank_by == GNNCCA_RANK_BY_REID);
    if (reads_reid && (!reid || reid_dim == 0)) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long* ei = reinterpret_cast<long long*>(edge_index_out);
    if (capped) {
        const TopkGeometry geo = topk_geometry(sel.max_deg, n_nodes);
        with_mode(mode, [&](auto M) { with_flag(sel.rank_by == GNNCCA_RANK_BY_GROUND, [&](auto ground) {
            hipLaunchKernelGGL((build_edges_topk_kernel<M(), rank_of(ground)>), geo.grid, geo.block, geo.lds_bytes, st, *fr, reid, (int)reid_dim,
                               (int)n_nodes, (long long)n_edges, geo.cap, ei, edge_attr_out, edge_labels_out, zero_ptr, (int)zero_n);
        }); });
    } else {
        // few sources: split each source's candidate chunks over up to 16 waves so that the launch still fills the chip
        unsigned slices = 1;
        while (slices < 16 && (long long)n_nodes * slices < 4096) slices *= 2;
        const dim3 grid((unsigned)((n_nodes + 3) / 4), slices), block(256);
        with_mode(mode, [&](auto M) {
            if (sel.kind == EdgeSelect::kGated)
                hipLaunchKernelGGL((build_edges_radius_kernel<M()>), grid, block, 0, st, *fr, reid, (int)reid_dim, (int)n_nodes, (long long)n_edges,
                                   sel.radius, (int)sel.unit, ei, edge_attr_out, edge_labels_out, zero_ptr, (int)zero_n);
            else
                hipLaunchKernelGGL((build_edges_kernel<M()>), grid, block, 0, st, *fr, reid, (int)reid_dim, (int)n_nodes, (long long)n_edges, ei,
                                   edge_attr_out, edge_labels_out, zero_ptr, (int)zero_n);
        });
    }
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

extern "C" {

// ---- host side of row N1: the edge enumeration of a batch of frames (inference.py:207-212), written straight into the staging image ----
// (the layout of `staging`: internal.h, StagingImage)
size_t gnncca_plan_frames_bytes(int64_t n, int64_t g) { return staging_image_bytes(n, g); }

// top_k == 0: every candidate (gnncca_plan_frames); top_k >= 1: min(top_k, deg) edges per source (gnncca_build_edges_topk)
int64_t gnncca_plan_frames_ex(const double* xw, const double* yw, const int64_t* ids, const int64_t* id_cam, int64_t n,
                              const int64_t* graph_sizes, const double* max_dist, int64_t g, int64_t top_k, void* staging,
                              size_t staging_bytes, int32_t* max_deg_out) {
    if (top_k < 0) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    if (n < 0 || g < 0 || !staging || staging_bytes < gnncca_plan_frames_bytes(n, g)) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    if ((n > 0 && (!xw || !yw || !ids || !id_cam)) || (g > 0 && (!graph_sizes || !max_dist))) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    if (n >= (1ll << 31) - 64 || g >= (1ll << 31) - 64) return -(int64_t)GNNCCA_ERR_UNSUPPORTED;
    long long total = 0;
    for (int64_t q = 0; q < g; ++q) {
        if (graph_sizes[q] < 0) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
        total += graph_sizes[q];
    }
    if (total != n) return -(int64_t)GNNCCA_ERR_INVALID_ARG;   // id_cam length does not match graph_sizes
    const StagingImage img = staging_image(staging, n, g);
    if (n) {
        std::memcpy(img.xw, xw, 8 * (size_t)n);
        std::memcpy(img.yw, yw, 8 * (size_t)n);
        std::memcpy(img.ids, ids, 8 * (size_t)n);
    }
    if (g) std::memcpy(img.max_dist, max_dist, 8 * (size_t)g);
    // cameras: np.unique order (ascending camera id) inside every frame = the rank among the batch's distinct camera ids
    std::vector<int64_t> cams;
    for (int64_t i = 0; i < n; ++i) {
        if (id_cam[i] < INT32_MIN || id_cam[i] > INT32_MAX) return -(int64_t)GNNCCA_ERR_UNSUPPORTED;
        bool seen = false;
        for (int64_t c : cams) seen = seen || c == id_cam[i];
        if (!seen) {
            if (cams.size() >= 4096) return -(int64_t)GNNCCA_ERR_UNSUPPORTED;
            cams.push_back(id_cam[i]);
        }
    }
    std::sort(cams.begin(), cams.end());
    const int64_t n_cam = std::max<int64_t>((int64_t)cams.size(), 1);
    // person ids: any relabelling that preserves equality (gnncca_frames::person_id) -- first appearance, open addressing
    {
        size_t cap = 16;
        while (cap < (size_t)(2 * n + 1)) cap <<= 1;
        std::vector<int64_t> keys(cap);
        std::vector<int32_t> vals(cap, -1);
        int32_t next = 0;
        for (int64_t i = 0; i < n; ++i) {
            const uint64_t hsh = (uint64_t)ids[i] * 0x9E3779B97F4A7C15ull;
            size_t slot = (size_t)(hsh >> 20) & (cap - 1);
            while (vals[slot] >= 0 && keys[slot] != ids[i]) slot = (slot + 1) & (cap - 1);
            if (vals[slot] < 0) keys[slot] = ids[i], vals[slot] = next++;
            img.person[i] = vals[slot];
        }
    }
    // stable counting sort by (frame, camera rank): frame-major, camera order inside a frame, node id ascending inside a camera
    std::vector<int32_t> key((size_t)n);
    std::vector<int32_t> count((size_t)(g * n_cam) + 1, 0);
    {
        int64_t i = 0;
        img.graph_ptr[0] = 0;
        for (int64_t q = 0; q < g; ++q) {
            for (int64_t k = 0; k < graph_sizes[q]; ++k, ++i) {
                const int32_t rank = (int32_t)(std::lower_bound(cams.begin(), cams.end(), id_cam[i]) - cams.begin());
                img.graph_of[i] = (int32_t)q;
                img.cam[i] = (int32_t)id_cam[i];
                key[(size_t)i] = (int32_t)(q * n_cam + rank);
                ++count[(size_t)key[(size_t)i]];
            }
            img.graph_ptr[q + 1] = (int32_t)i;
        }
    }
    std::vector<int32_t> start((size_t)(g * n_cam) + 1, 0);
    for (size_t k = 0; k + 1 < start.size(); ++k) start[k + 1] = start[k] + count[k];
    {
        std::vector<int32_t> cursor(start);
        for (int64_t i = 0; i < n; ++i) img.src_order[cursor[(size_t)key[(size_t)i]]++] = (int32_t)i;
    }
    long long e = 0, max_deg = 0;
    for (int64_t pos = 0; pos < n; ++pos) {
        const int32_t node = img.src_order[pos];
        img.edge_ptr[pos] = (int32_t)e;
        const long long deg = graph_sizes[img.graph_of[node]] - count[(size_t)key[(size_t)node]];   // every node of the frame's OTHER cameras
        max_deg = std::max(max_deg, deg);
        e += top_k > 0 ? std::min<long long>(deg, top_k) : deg;
        if (e >= (1ll << 31) - 64) return -(int64_t)GNNCCA_ERR_UNSUPPORTED;      // more than 2^31 edges in one batch
    }
    img.edge_ptr[n] = (int32_t)e;
    for (int64_t q = 0; q <= g; ++q) img.edge_ptr_g[q] = img.edge_ptr[img.graph_ptr[q]];   // edges are emitted frame by frame
    if (max_deg_out) *max_deg_out = (int32_t)max_deg;
    return (int64_t)e;
}

// The gate of graph_radius.cuh on the host: the identical IEEE sequence (two products and one sum, each rounded once; contraction off).
static inline bool within_radius_host(double xi, double yi, double xj, double yj, double t2) {
#pragma clang fp contract(off)
    const double dx = xi - xj, dy = yi - yj;
    const double a = dx * dx, b = dy * dy;
    const double s = a + b;
    return s <= t2;
}
static inline double radius_gate_t2_host(double radius, int32_t unit, double md) {
#pragma clang fp contract(off)
    const double t = unit == GNNCCA_RADIUS_UNIT_MAX_DIST ? radius * md : radius;
    return t * t;
}

// gnncca_plan_frames' image with edge_ptr / edge_ptr_g counting the candidates within the radius.  Every unordered pair of a frame is
// evaluated once (s(i, j) == s(j, i) bit for bit) and counted for both of its sources.
int64_t gnncca_plan_frames_radius(const double* xw, const double* yw, const int64_t* ids, const int64_t* id_cam, int64_t n,
                                  const int64_t* graph_sizes, const double* max_dist, int64_t g, double radius, int32_t unit, void* staging,
                                  size_t staging_bytes) {
    if (radius_invalid(radius, unit)) return -(int64_t)GNNCCA_ERR_INVALID_ARG;
    const int64_t dense = gnncca_plan_frames_ex(xw, yw, ids, id_cam, n, graph_sizes, max_dist, g, 0, staging, staging_bytes, nullptr);
    if (dense < 0) return dense;
    const StagingImage img = staging_image(staging, n, g);
    std::vector<int32_t> kept((size_t)n, 0);
    for (int64_t q = 0; q < g; ++q) {
        const int32_t gs = img.graph_ptr[q], ge = img.graph_ptr[q + 1];
        const double t2 = radius_gate_t2_host(radius, unit, max_dist[q]);
        for (int32_t a = gs; a < ge; ++a) {
            const double xa = xw[a], ya = yw[a];
            const int32_t ca = img.cam[a];
            int32_t mine = 0;
            for (int32_t b = a + 1; b < ge; ++b) {
                const int32_t hit = (img.cam[b] != ca) & (int32_t)within_radius_host(xa, ya, xw[b], yw[b], t2);
                mine += hit;
                kept[(size_t)b] += hit;
            }
            kept[(size_t)a] += mine;
        }
    }
    long long e = 0;
    for (int64_t pos = 0; pos < n; ++pos) {
        img.edge_ptr[pos] = (int32_t)e;
        e += kept[(size_t)img.src_order[pos]];   // (<= the dense count, which the plan above bounded by 2^31 - 64)
    }
    img.edge_ptr[n] = (int32_t)e;
    for (int64_t q = 0; q <= g; ++q) img.edge_ptr_g[q] = img.edge_ptr[img.graph_ptr[q]];
    return (int64_t)e;
}

int64_t gnncca_plan_frames(const double* xw, const double* yw, const int64_t* ids, const int64_t* id_cam, int64_t n,
                           const int64_t* graph_sizes, const double* max_dist, int64_t g, void* staging, size_t staging_bytes) {
    return gnncca_plan_frames_ex(xw, yw, ids, id_cam, n, graph_sizes, max_dist, g, 0, staging, staging_bytes, nullptr);
}

}  // extern "C"
