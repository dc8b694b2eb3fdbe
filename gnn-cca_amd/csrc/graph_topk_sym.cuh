#pragma once
// Capped graph build closed under reversal: with D the directed edge set of build_edges_topk_kernel (graph_topk.cuh; every source keeps its
// k smallest-key cross-camera candidates, ties to the smaller destination id),
//   'union'   keeps the dense edge (i, j) iff (i, j) in D or  (j, i) in D
//   'mutual'  keeps it                   iff (i, j) in D and (j, i) in D
// so every kept edge has its reverse, mutual is a subset of D and D of union, and for k >= max deg both are the dense build.  Whether i is
// in j's list is decided by j's OWN selection -- the key bits j's wave ranked with ('reid' keys are not symmetric: F.pairwise_distance adds
// its eps to a - b) -- and NO KEY IS EVALUATED TWICE FROM TWO SIDES: the selection is made once per source and published as bits, the
// closure is pure bit arithmetic on them, so a last-ulp difference between two evaluations cannot break it.  A kept edge carries the dense
// build's bits (build_edges_kernel's statements).  LIKE THE CAP ITSELF THIS HAS NO COUNTERPART IN THE REFERENCE, which only builds complete
// graphs (every pair in both directions).
//
// Four launches, one wave per source position in the first, second and last, no atomics:
//   1. select   passes 1-2 of the directed kernel (topk_keys / topk_threshold, the same code); its keep decision is written as a BIT ROW
//               indexed by the destination's offset in the frame: ceil(n_g / 64) 64-bit words per node of frame g, every word written.
//   2. close    for each 64-detection chunk of the frame: own word | or & the ballot of bit (j0 + lane, i) of the others' rows, stored
//               into a SECOND matrix (other waves still read the first), popcount added to the source's edge count.
//   3. scan     counts over src_order positions -> edge_ptr [N + 1] and edge_ptr_g [G + 1], written into the staging image where the plan's
//               capped values were: the post-processing, the evaluation and gnncca_build_edges_topk_backward read the symmetric layout
//               from the places they always read.  The caller copies edge_ptr_g (its last entry is E) to the host and waits: E depends
//               on the data.
//   4. emit     after the host has allocated the outputs: the closed row in candidate order; slot = edge_ptr[position] + bits before.
// Workspace: [bit matrix A | bit matrix B | counts int32 [N]], a matrix being sum_g n_g ceil(n_g / 64) words (topk_sym_words); a frame's
// rows start at the sum over the frames before it (frame_row_base), a node's row at its offset in the frame times the frame's words.
// Every loop's trip count comes from n_g, deg or G; a row that would leave the matrix (a frame layout other than the declared one) is
// neither read nor written, and a source with more candidates than declared selects nothing (a zero row).
// Part of the translation unit graph_build.hip.

namespace gnncca {

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// first word of frame g's rows: sum over the frames before it of n ceil(n / 64)
__device__ __forceinline__ long long frame_row_base(const int* __restrict__ graph_ptr, int g, int lane) {
    long long s = 0;
    for (int q = lane; q < g; q += 64) {
        const long long n = graph_ptr[q + 1] - graph_ptr[q];
        s += n * ((n + 63) >> 6);
    }
    return wave_sum_ll(s);
}

struct SymRow {
    int i, g, gs, ge, words;
    long long row;   // first word of source i's row; -1: outside the declared matrix
};

__device__ __forceinline__ SymRow sym_row(const gnncca_frames& fr, int p, int lane, long long total_words) {
    SymRow r;
    r.i = fr.src_order[p];
    r.g = fr.graph_of[r.i];
    r.gs = fr.graph_ptr[r.g];
    r.ge = fr.graph_ptr[r.g + 1];
    const int n_g = r.ge - r.gs;
    r.words = (n_g + 63) >> 6;
    const long long base = frame_row_base(fr.graph_ptr, r.g, lane);
    const bool ok = n_g > 0 && r.i >= r.gs && r.i < r.ge && base >= 0 && base + (long long)n_g * r.words <= total_words;
    r.row = ok ? base + (long long)(r.i - r.gs) * r.words : -1;
    return r;
}

// ---- 1. select -------------------------------------------------------------------------------------------------------------------
template <int RANK>
__global__ __launch_bounds__(256) void topk_sym_select_kernel(const gnncca_frames fr, const float* __restrict__ reid, int R, int N, int top_k,
                                                              int cap, unsigned long long* __restrict__ bits, long long total_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_topk[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * (blockDim.x >> 6) + wave;
    if (p >= N) return;
    unsigned long long* __restrict__ s_key = reinterpret_cast<unsigned long long*>(s_topk + (size_t)wave * cap * kTopkSlotBytes);
    int* __restrict__ s_node = reinterpret_cast<int*>(s_key + cap);
    const SymRow r = sym_row(fr, p, lane, total_words);
    if (r.row < 0) return;
    const int i = r.i, gs = r.gs, ge = r.ge;
    const int ci = fr.cam[i];
    const float* __restrict__ ri = reid + (size_t)i * R;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long* __restrict__ row = bits + r.row;

    const int deg = topk_keys<RANK>(fr, reid, ri, R, (R & 3) == 0, gs, ge, ci, fr.xw[i], fr.yw[i], cap, lane, s_key, s_node);
    const bool over = deg > cap;   // more candidates than the caller declared: the source selects nothing
    const int n_keep = over ? 0 : min(top_k, deg);
    wave_lds_fence();
    const bool all = n_keep >= deg;
    unsigned long long T = 0ull;
    int need = 0;
    if (!all && n_keep > 0) topk_threshold<RANK>(s_key, deg, n_keep, lane, T, need);

    // the keep decision of pass 3, by the frame's 64-detection chunks: a candidate's slot is its rank among the candidates so far
    int seen = 0, ties = 0;
    for (int c = 0, j0 = gs; j0 < ge; ++c, j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < ge && fr.cam[j] != ci;
        const unsigned long long mask = __ballot(valid);
        const int idx = seen + __popcll(mask & below);
        bool keep = valid && n_keep > 0;
        if (!all && n_keep > 0) {
            const unsigned long long key = valid ? s_key[idx] : ~0ull;   // (valid and !over: idx < deg <= cap)
            const bool eq = valid && key == T;
            const unsigned long long eqm = __ballot(eq);
            keep = (valid && key < T) || (eq && ties + __popcll(eqm & below) < need);
            ties += __popcll(eqm);
        }
        const unsigned long long word = __ballot(keep);
        if (lane == 0) row[c] = word;
        seen += __popcll(mask);
    }
}

// ---- 2. close and count ----------------------------------------------------------------------------------------------------------------
template <bool UNION>
__global__ __launch_bounds__(256) void topk_sym_close_kernel(const gnncca_frames fr, int N, const unsigned long long* __restrict__ bits_a,
                                                             unsigned long long* __restrict__ bits_b, long long total_words,
                                                             int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= N) return;
    const SymRow r = sym_row(fr, p, lane, total_words);
    int cnt = 0;
    if (r.row >= 0) {
        const int li = r.i - r.gs;
        const long long frame0 = r.row - (long long)li * r.words;   // the frame's first row
        const int my_word = li >> 6, my_bit = li & 63;
        for (int c = 0, j0 = r.gs; j0 < r.ge; ++c, j0 += 64) {
            const int lj = (j0 - r.gs) + lane;   // this lane's detection, as an offset in the frame
            const unsigned long long own = bits_a[r.row + c];
            const bool back = j0 + lane < r.ge && ((bits_a[frame0 + (long long)lj * r.words + my_word] >> my_bit) & 1ull) != 0ull;
            const unsigned long long rev = __ballot(back);
            const unsigned long long closed = UNION ? (own | rev) : (own & rev);
            if (lane == 0) bits_b[r.row + c] = closed;
            cnt += __popcll(closed);
        }
    }
    if (lane == 0) counts[p] = cnt;
}

// ---- 3. scan ---------------------------------------------------------------------------------------------------------------------------
// One workgroup: edge_ptr[p] = counts[0] + ... + counts[p - 1], tile by tile with a carry; then edge_ptr_g[g] = edge_ptr[graph_ptr[g]]
// (positions are frame-major: a frame's sources are the positions graph_ptr[g] .. graph_ptr[g + 1]).  Sums are clamped at INT_MAX so that
// the host sees an impossible E rather than a wrapped one.
__global__ __launch_bounds__(256) void topk_sym_scan_kernel(const int* __restrict__ counts, int N, int G, const int* __restrict__ graph_ptr,
                                                            int* edge_ptr, int* edge_ptr_g) {
    __shared__ long long s_wave[4];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < N; base += 256) {
        const int p = base + tid;
        const long long v = p < N ? (long long)max(counts[p], 0) : 0ll;
        long long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        long long before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (p < N) edge_ptr[p] = (int)min(before + incl - v, (long long)INT_MAX);
        __syncthreads();
        if (tid == 255) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) edge_ptr[N] = (int)min(s_carry, (long long)INT_MAX);
    __threadfence_block();
    __syncthreads();
    for (int g = tid; g <= G; g += 256) {
        const int q = graph_ptr[g];
        edge_ptr_g[g] = q >= 0 && q <= N ? edge_ptr[q] : edge_ptr[N];
    }
}

// ---- 4. emit ---------------------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void topk_sym_emit_kernel(const gnncca_frames fr, const float* __restrict__ reid, int R, int N, long long E,
                                                            const unsigned long long* __restrict__ bits, long long total_words,
                                                            long long* __restrict__ ei_out, float* __restrict__ attr_out,
                                                            float* __restrict__ lab_out) {
    constexpr int NA = MODE == GNNCCA_EDGE_ATTR_FULL ? 4 : 2;
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= N) return;
    const SymRow r = sym_row(fr, p, lane, total_words);
    if (r.row < 0) return;
    const int i = r.i, gs = r.gs, ge = r.ge;
    const int ci = fr.cam[i], pi = fr.person_id[i];
    const double xi = fr.xw[i], yi = fr.yw[i], md = fr.max_dist[r.g];
    const float* __restrict__ ri = reid + (size_t)i * R;
    const bool vec4 = (R & 3) == 0;
    long long pos = fr.edge_ptr[p];
    for (int c = 0, j0 = gs; j0 < ge; ++c, j0 += 64) {
        const int j = j0 + lane;
        const bool keep = ((bits[r.row + c] >> lane) & 1ull) != 0ull && j < ge && fr.cam[j] != ci;
        const unsigned long long mask = __ballot(keep);
        if (mask == 0ull) continue;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, lab = 0.f;
        if (keep) {   // build_edges_kernel's statements
            lab = fr.person_id[j] == pi ? 1.f : 0.f;
            if (MODE != GNNCCA_EDGE_ATTR_ONLY_APPEARANCE) {
                double l2, l1;
                ground_dists(xi, yi, fr.xw[j], fr.yw[j], l2, l1);
                a0 = (float)__ddiv_rn(l2, md);
                a1 = (float)__ddiv_rn(l1, md);
            }
        }
        if (MODE != GNNCCA_EDGE_ATTR_ONLY_DIST) {
            float sd = 0.f, sab = 0.f, saa = 1.f, sbb = 1.f;
            reid_sums_wave(reid, ri, R, vec4, mask, lane, [&](int t) { return j0 + t; }, sd, sab, saa, sbb);
            const float emb = reid_emb(sd), cosv = reid_cos(sab, saa, sbb);
            if (MODE == GNNCCA_EDGE_ATTR_FULL) {
                a2 = emb;
                a3 = cosv;
            } else {
                a0 = emb;
                a1 = cosv;
            }
        }
        const long long k = pos + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && k >= 0 && k < E) {
            ei_out[k] = i;
            ei_out[E + k] = j;
            if (NA == 4) {
                *reinterpret_cast<float4*>(attr_out + k * 4) = make_float4(a0, a1, a2, a3);
            } else {
                *reinterpret_cast<float2*>(attr_out + k * 2) = make_float2(a0, a1);
            }
            lab_out[k] = lab;
        }
        pos += __popcll(mask);
    }
}

// words of ONE bit matrix for these frame sizes (host); -1: a negative size
inline long long topk_sym_words(const int64_t* graph_sizes, int64_t n_frames, long long* n_nodes_out) {
    long long words = 0, nodes = 0;
    for (int64_t q = 0; q < n_frames; ++q) {
        const long long n = graph_sizes[q];
        if (n < 0) return -1;
        words += n * ((n + 63) / 64);
        nodes += n;
    }
    if (n_nodes_out) *n_nodes_out = nodes;
    return words;
}

}  // namespace gnncca
