#pragma once
// strong_closure.cuh -- the reachability matrix of ONE frame in LDS and what a workgroup does with it: the diagonal, the transitive closure
// by in-place repeated squaring, and a node's label from the closed matrix.  Written once for strong_cluster_kernel (strong.cuh, unit
// mpn_post.hip: one prediction vector) and eval_sweep_strong_kernel (eval_sweep_strong.cuh, unit evaluate.hip: every operating point), so
// that the two cannot disagree about the partition.  Nothing here contains floating point: the units' fp settings do not matter.
//
// R: n_pad rows of W = n_pad / 32 words (n_pad = the frame's n nodes rounded up to 32); bit b of row a = "b is reachable from a".  The
// caller sets the bits of the active edges between strong_diagonal and strong_close (atomicOr, a barrier on either side).
namespace gnncca {

constexpr int kStrongMaxRounds = 12;   // ceil(log2(1024)) + 1 = 11 (one flag word per round: no reset, one barrier per round)

__device__ __forceinline__ unsigned strong_ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void strong_st(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// R = the identity on the frame's n nodes, zero elsewhere (the padding rows and columns stay zero for good).  No barrier inside.
template <int BLOCK>
__device__ __forceinline__ void strong_diagonal(unsigned* R, int n, int W) {
    const int words = (W << 5) * W;
    for (int t = threadIdx.x; t < words; t += BLOCK) {
        const int i = t / W, w = t - i * W;
        R[t] = (i < n && w == (i >> 5)) ? 1u << (i & 31) : 0u;
    }
}

// Repeated squaring IN PLACE: the owner of (row i, word w) ORs in word w of every row j whose bit is set in row i.  Every word has exactly
// one writer.  A reader may see another row before or after that row's update of the same round; both are sound, because every set bit is
// a true reachability fact at all times -- so the in-place form reaches the fixpoint at least as fast as the two-buffer form, which covers
// paths of 2^r edges after round r.  A simple path has fewer than n_pad edges: ceil(log2(n_pad)) rounds complete the closure whatever the
// data, and one more detects it.  The loop is COUNTED, with an early exit after a round that changed nothing; there is no "until
// fixpoint".  round_flags: kStrongMaxRounds LDS words, zero on entry (a barrier after the zeroing), [r] = round r changed a word.  Every
// thread of the workgroup calls this (BLOCK may be narrower than the frame); on return the matrix is closed and visible to all of them.
template <int BLOCK>
__device__ __forceinline__ void strong_close(unsigned* R, int n, int W, int* round_flags) {
    const int tid = threadIdx.x;
    const int n_pad = W << 5, items = n * W;
    int lg = 0;
    while ((1 << lg) < n_pad) ++lg;
    const int max_rounds = lg + 1;   // <= kStrongMaxRounds - 1: the bound, whatever the data
    for (int round = 0; round < max_rounds; ++round) {
        int changed = 0;
        for (int t = tid; t < items; t += BLOCK) {
            const int i = t / W, w = t - i * W;
            const unsigned* row = R + i * W;
            const unsigned old = strong_ld(&row[w]);
            unsigned acc = old;
            for (int w2 = 0; w2 < W; ++w2) {
                unsigned bits = strong_ld(&row[w2]);
                while (bits) {
                    const int j = (w2 << 5) + __builtin_ctz(bits);   // j < n: only real nodes' bits are ever set
                    bits &= bits - 1;
                    acc |= strong_ld(&R[j * W + w]);
                }
            }
            if (acc != old) {
                strong_st(&R[t], acc);   // the word's only writer
                changed = 1;
            }
        }
        if (changed) round_flags[round] = 1;
        __syncthreads();
        if (!round_flags[round]) break;   // (uniform: nobody writes this round's word after the barrier)
    }
}

// The frame-local label of node v < n from the CLOSED matrix: the smallest u with R[v][u] && R[u][v].  The set bits of row v are scanned
// ascending and the scan ends at the first hit, v itself at the latest.
__device__ __forceinline__ int strong_root(const unsigned* R, int W, int v) {
    const unsigned* row = R + v * W;
    const int wv = v >> 5;
    const unsigned bv = 1u << (v & 31);
    for (int w2 = 0; w2 <= wv; ++w2) {
        unsigned bits = row[w2];
        while (bits) {
            const int u = (w2 << 5) + __builtin_ctz(bits);
            bits &= bits - 1;
            if (u >= v) return v;   // v's own bit ends the scan at the latest
            if (R[u * W + wv] & bv) return u;
        }
    }
    return v;
}

}  // namespace gnncca
