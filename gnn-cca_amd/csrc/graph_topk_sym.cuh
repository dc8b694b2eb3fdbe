#pragma once
// Capped graph build closed under reversal: with D the directed edge set of build_edges_topk_kernel (graph_topk.cuh; every source keeps its
// k smallest-key cross-camera candidates, ties to the smaller destination id),
//   'union'   keeps the dense edge (i, j) iff (i, j) in D or  (j, i) in D
//   'mutual'  keeps it                   iff (i, j) in D and (j, i) in D
// so every kept edge has its reverse, mutual is a subset of D and D of union, and for k >= max deg both are the dense build.  Whether i is
// in j's list is decided by j's OWN selection -- the key bits j's wave ranked with ('reid' keys are not symmetric: F.pairwise_distance adds
// its eps to a - b) -- and NO KEY IS EVALUATED TWICE FROM TWO SIDES: the selection is made once per source and published as bits, the
// closure is pure bit arithmetic on them, so a last-ulp difference between two evaluations cannot break it.  A kept edge carries the dense
// build's bits (the emit kernel calls graph_build.hip's emit_edges, as build_edges_kernel does).  LIKE THE CAP ITSELF THIS HAS NO
// COUNTERPART IN THE REFERENCE, which only builds complete graphs (every pair in both directions).
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
    int words;       // of a row of the source's frame
    long long row;   // first word of the source's row; -1: outside the declared matrix
};

__device__ __forceinline__ SymRow sym_row(const gnncca_frames& fr, const EdgeSource& s, int lane, long long total_words) {
    SymRow r;
    const int n_g = s.ge - s.gs;
    r.words = (n_g + 63) >> 6;
    const long long base = frame_row_base(fr.graph_ptr, s.g, lane);
    const bool ok = n_g > 0 && s.i >= s.gs && s.i < s.ge && base >= 0 && base + (long long)n_g * r.words <= total_words;
    r.row = ok ? base + (long long)(s.i - s.gs) * r.words : -1;
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
    const EdgeSource s = load_edge_source(fr, reid, R, p);
    const SymRow r = sym_row(fr, s, lane, total_words);
    if (r.row < 0) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long* __restrict__ row = bits + r.row;

    const int deg = topk_keys<RANK>(fr, reid, R, s, cap, lane, s_key, s_node);
    const bool over = deg > cap;   // more candidates than the caller declared: the source selects nothing
    const int n_keep = over ? 0 : min(top_k, deg);
    wave_lds_fence();
    const bool all = n_keep >= deg;
    unsigned long long T = 0ull;
    int need = 0;
    if (!all && n_keep > 0) topk_threshold<RANK>(s_key, deg, n_keep, lane, T, need);

    // the keep decision of pass 3, by the frame's 64-detection chunks: a candidate's slot is its rank among the candidates so far
    int seen = 0, ties = 0;
    for (int c = 0, j0 = s.gs; j0 < s.ge; ++c, j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < s.ge && fr.cam[j] != s.ci;
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
    const EdgeSource s = load_edge_source(fr, nullptr, 0, p);   // (no reid table here: the frame and the node id are what it needs)
    const SymRow r = sym_row(fr, s, lane, total_words);
    int cnt = 0;
    if (r.row >= 0) {
        const int li = s.i - s.gs;
        const long long frame0 = r.row - (long long)li * r.words;   // the frame's first row
        const int my_word = li >> 6, my_bit = li & 63;
        for (int c = 0, j0 = s.gs; j0 < s.ge; ++c, j0 += 64) {
            const int lj = (j0 - s.gs) + lane;   // this lane's detection, as an offset in the frame
            const unsigned long long own = bits_a[r.row + c];
            const bool back = j0 + lane < s.ge && ((bits_a[frame0 + (long long)lj * r.words + my_word] >> my_bit) & 1ull) != 0ull;
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
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= N) return;
    const EdgeSource s = load_edge_source(fr, reid, R, p);
    const SymRow r = sym_row(fr, s, lane, total_words);
    if (r.row < 0) return;
    long long pos = fr.edge_ptr[p];
    for (int c = 0, j0 = s.gs; j0 < s.ge; ++c, j0 += 64) {
        const int j = j0 + lane;
        const bool keep = ((bits[r.row + c] >> lane) & 1ull) != 0ull && j < s.ge && fr.cam[j] != s.ci;
        const unsigned long long mask = __ballot(keep);
        if (mask == 0ull) continue;
        emit_edges<MODE>(fr, reid, R, s, j, keep, mask, lane, [&](int t) { return j0 + t; }, pos,
                         [&](long long k) { return k >= 0 && k < E; }, E, ei_out, attr_out, lab_out);
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
