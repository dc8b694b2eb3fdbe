#pragma once
// Graph build with a capped neighbourhood: every detection keeps the k cross-camera candidates of its own frame with the smallest key
// (ground-plane L2 distance in float64, or the fp32 reid distance), ties to the smaller destination id.  The enumeration, the four
// (or two) attributes and the label of a kept edge are gnncca_build_edges' (inference.py:207-266): pass 3 calls graph_build.hip's
// emit_edges, as the dense kernel does, so a kept edge carries the dense build's bits -- but the PRUNING HAS NO COUNTERPART IN THE
// REFERENCE, which only builds complete graphs.
//
// Shape: ONE WAVE PER SOURCE POSITION (sources in src_order), three passes, no workgroup barrier (waves of a workgroup never meet):
//   1. keys.  The frame is walked in 64-detection chunks, one candidate per lane, as in build_edges_kernel.  The key of a cross-camera
//      candidate -- the bits of the float64 L2 distance, or of the fp32 `emb` value reid_sums_wave gives -- goes to LDS at the
//      candidate's rank among the source's candidates (a ballot prefix: candidates stay in the dense edge order), next to its node id.
//      Both keys are non-negative IEEE numbers, so unsigned order of the bits is numeric order (NaNs last, deterministically).
//   2. select.  The k-th smallest key T is found bit by bit from the top (64 or 32 rounds): T takes a bit when fewer than k keys
//      are below the value it would then have -- a count by ballot over the LDS keys, an integer, exact.  Survivors: every key
//      below T, and of the keys equal to T the first k - #(keys below T) in candidate order, i.e. the smaller destination ids.
//      A radix select rather than a sort: it needs no data movement and no cross-lane exchange beyond the ballot, costs
//      bits x ceil(deg / 64) LDS reads per lane (0.8 k for the 768 candidates of a four-camera dense1024 frame, where a rank count
//      would need 9 k and a bitonic sort 55 exchanges of 12 values each), and is skipped when deg <= k (the source keeps everything).
//   3. emit.  The survivors of each 64-candidate chunk are one ballot; their slots are edge_ptr[position] + survivors so far + the
//      ballot prefix, so stores are contiguous and in candidate order: the output is a subsequence of the dense edge list.  The reid
//      terms of the survivors are recomputed here by the whole wave (reid_sums_wave; k rows, not deg) -- with 'ground' ranking the
//      reid table is read for the kept edges only, which is where the dense kernel spends its time.
// LDS: 12 B per candidate slot, max_deg rounded up to 64 slots per wave, four waves per workgroup while that fits 64 KB (every
// Terrace-sized frame), else two or one.  GNNCCA_TOPK_MAX_DEG = 4096 candidates per source is what one wave's 48 KB holds; more is
// refused on the host (GNNCCA_ERR_UNSUPPORTED), and a source whose frame turns out to hold more candidates than the caller declared
// is left unwritten rather than overrunning its slots.
// Passes 1 and 2 are the device functions topk_keys / topk_threshold: the symmetric build (graph_topk_sym.cuh) runs the same code.
// Part of the translation unit graph_build.hip.

namespace gnncca {

constexpr int kTopkSlotBytes = 12;   // u64 key + i32 node id

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- passes 1 and 2, shared with the symmetric build (graph_topk_sym.cuh): one wave, the same statements, the same bits ----
// 1. keys of source s against its frame: key and node id of every cross-camera candidate at its rank among the candidates -> s_key /
// s_node (slots below `cap` only).  Returns deg, the number of candidates found.
template <int RANK>
__device__ __forceinline__ int topk_keys(const gnncca_frames& fr, const float* __restrict__ reid, int R, const EdgeSource& s, int cap, int lane,
                                         unsigned long long* __restrict__ s_key, int* __restrict__ s_node) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int deg = 0;
    for (int j0 = s.gs; j0 < s.ge; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < s.ge && fr.cam[j] != s.ci;   // same camera: no edge (inference.py:210-211)
        const unsigned long long mask = __ballot(valid);
        if (mask == 0ull) continue;
        unsigned long long key = 0ull;
        if (RANK == GNNCCA_RANK_BY_GROUND) {
            if (valid) {
                double l2, l1;
                ground_dists(s.xi, s.yi, fr.xw[j], fr.yw[j], l2, l1);
                key = (unsigned long long)__double_as_longlong(l2);
            }
        } else {
            float sd = 0.f, sab = 0.f, saa = 1.f, sbb = 1.f;
            reid_sums_wave(reid, s.ri, R, s.vec4, mask, lane, [&](int t) { return j0 + t; }, sd, sab, saa, sbb);
            key = (unsigned long long)__float_as_uint(reid_emb(sd));
        }
        const int idx = deg + __popcll(mask & below);
        if (valid && idx < cap) s_key[idx] = key, s_node[idx] = j;
        deg += __popcll(mask);
    }
    return deg;
}

// 2. the n_keep-th smallest of the deg keys in s_key (n_keep < deg): T, and `need`, how many of the keys equal to T survive.
template <int RANK>
__device__ __forceinline__ void topk_threshold(const unsigned long long* __restrict__ s_key, int deg, int n_keep, int lane,
                                               unsigned long long& T, int& need) {
    auto count_below_key = [&](unsigned long long c) {
        int cnt = 0;
        for (int base = 0; base < deg; base += 64) {
            const int idx = base + lane;
            cnt += __popcll(__ballot(idx < deg && s_key[idx] < c));
        }
        return cnt;
    };
    T = 0ull;
    for (int b = RANK == GNNCCA_RANK_BY_GROUND ? 63 : 31; b >= 0; --b) {
        const unsigned long long c = T | (1ull << b);
        if (count_below_key(c) < n_keep) T = c;
    }
    need = n_keep - count_below_key(T);
}

template <int MODE, int RANK>
__global__ __launch_bounds__(256) void build_edges_topk_kernel(const gnncca_frames fr, const float* __restrict__ reid, int R, int N,
                                                               long long E, int cap, long long* __restrict__ ei_out,
                                                               float* __restrict__ attr_out, float* __restrict__ lab_out,
                                                               int* __restrict__ zero_ptr, int zero_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_topk[];
    zero_counters(zero_ptr, zero_n, true, blockDim.x);   // (every thread of the launch: the grid has one row)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * (blockDim.x >> 6) + wave;
    if (p >= N) return;
    unsigned long long* __restrict__ s_key = reinterpret_cast<unsigned long long*>(s_topk + (size_t)wave * cap * kTopkSlotBytes);
    int* __restrict__ s_node = reinterpret_cast<int*>(s_key + cap);
    const long long out0 = fr.edge_ptr[p];
    const int n_keep = fr.edge_ptr[p + 1] - fr.edge_ptr[p];   // min(k, deg) by the plan (gnncca_plan_frames_ex)
    if (n_keep <= 0) return;
    const EdgeSource s = load_edge_source(fr, reid, R, p);
    const unsigned long long below = (1ull << lane) - 1ull;

    // ---- 1. keys ----
    const int deg = topk_keys<RANK>(fr, reid, R, s, cap, lane, s_key, s_node);
    if (deg > cap || n_keep > deg) return;   // more candidates than the caller declared, or a plan of another batch: nothing is written
    wave_lds_fence();

    // ---- 2. the n_keep-th smallest key ----
    const bool all = n_keep >= deg;
    unsigned long long T = 0ull;
    int need = 0;   // how many of the keys equal to T survive
    if (!all) topk_threshold<RANK>(s_key, deg, n_keep, lane, T, need);

    // ---- 3. the survivors, in candidate order ----
    int emitted = 0, ties = 0;
    for (int base = 0; base < deg && emitted < n_keep; base += 64) {
        const int idx = base + lane;
        const bool inb = idx < deg;
        const int j = inb ? s_node[idx] : s.gs;
        bool keep = inb;
        if (!all) {
            const unsigned long long key = inb ? s_key[idx] : ~0ull;
            const bool eq = inb && key == T;
            const unsigned long long eqm = __ballot(eq);
            keep = (inb && key < T) || (eq && ties + __popcll(eqm & below) < need);
            ties += __popcll(eqm);
        }
        const unsigned long long mask = __ballot(keep);
        if (mask == 0ull) continue;
        emit_edges<MODE>(fr, reid, R, s, j, keep, mask, lane, [&](int t) { return __shfl(j, t); }, out0 + emitted,
                         [&](long long k) { return k < E; }, E, ei_out, attr_out, lab_out);
        emitted += __popcll(mask);
    }
}

}  // namespace gnncca
