#pragma once
// excl_common.cuh -- what the two users of the camera-exclusive rule share, as device-inline / template code with no __global__ in it:
// excl_cluster_kernel (exclusive.cuh, translation unit mpn_post.hip: one threshold, compacted candidate list) and eval_sweep_excl_kernel
// (eval_sweep_exclusive.cuh, translation unit evaluate.hip: every threshold of a sweep over one read-only key array).  One definition of
// the activity test, the key codec, the reverse-edge search and the merge and compress phases of a mutual-best round: the two kernels
// cannot drift apart.  exclusive.cuh has the rule and the argument why the rounds give the sequential walk's partition.
#include <hip/hip_runtime.h>

#include "gnncca_mpn.h"

namespace gnncca {

constexpr int kExclMaxNodes = GNNCCA_EXCLUSIVE_MAX_FRAME_NODES;   // 12-bit frame-local ids in the keys
constexpr int kExclMaxCams = GNNCCA_EXCLUSIVE_MAX_CAMERAS;        // one 64-bit mask word

typedef unsigned long long excl_u64;

__device__ __forceinline__ int excl_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void excl_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ bool excl_active(float s, double th) { return (double)s >= th; }   // (false for a NaN)

// eval_sweep_kernel's test of a frame's ranges, with the LDS regions' size in the place of P_lds
__device__ __forceinline__ bool excl_frame_ok(int v0, int v1, long long k0, long long k1, int N_all, long long E, int P) {
    const int n = v1 - v0;
    return !(v0 < 0 || n < 0 || n > P || v1 > N_all || k0 < 0 || k1 < k0 || k1 > E);
}

// Frame g's node and edge range; the whole graph where the offsets are null (post_cc_kernel, strong_cluster_kernel).
struct FrameRange {
    int v0, v1;
    long long k0, k1;
};
__device__ __forceinline__ FrameRange frame_range(const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int g, int N_all,
                                                  long long E) {
    return FrameRange{node_ptr ? node_ptr[g] : 0, node_ptr ? node_ptr[g + 1] : N_all, edge_ptr ? edge_ptr[g] : 0, edge_ptr ? edge_ptr[g + 1] : E};
}

// The answer for a frame that is refused (ranges that do not fit, a camera id out of range): every node its own cluster,
// *n_clusters += n -- as far as the node range allows writing at all.
template <int BLOCK>
__device__ __forceinline__ void frame_singletons(int* __restrict__ labels, int* __restrict__ n_clusters, int v0, int v1, int N_all, int tid) {
    const int n = v1 - v0;
    if (v0 >= 0 && v1 <= N_all && n >= 0) {
        for (int v = v0 + tid; v < v1; v += BLOCK) labels[v] = v;
        if (tid == 0 && n > 0) atomicAdd(n_clusters, n);
    }
}

// 64-bit key of the pair {lo, hi} (frame-local, lo < hi < 4096) of weight w > 0: (fp32 bits of w) << 24 | (4095 - lo) << 12 | (4095 - hi).
// Positive floats order as their bits do, so the LARGEST key is the FIRST candidate of the rule's order; the key alone names the pair;
// 0 is no key.  Nothing in it depends on a threshold: w >= th is read off the key (excl_key_weight).
__device__ __forceinline__ excl_u64 excl_key(float w, int lo, int hi) {
    return ((excl_u64)__float_as_uint(w) << 24) | ((excl_u64)(4095 - lo) << 12) | (excl_u64)(4095 - hi);
}
__device__ __forceinline__ int excl_key_lo(excl_u64 key) { return 4095 - (int)((key >> 12) & 4095); }
__device__ __forceinline__ int excl_key_hi(excl_u64 key) { return 4095 - (int)(key & 4095); }
__device__ __forceinline__ float excl_key_weight(excl_u64 key) { return __uint_as_float((unsigned)(key >> 24)); }

// The edge (dst k, src k), or -1: searched in the CSR segment of dst k as post_prune_kernel searches it (a plan with
// GNNCCA_GRAPH_BAD_INDEX gives no edge a reverse; every index is in [0, N_all) otherwise).  k < E.
__device__ __forceinline__ int excl_reverse_edge(const long long* __restrict__ ei, long long E, long long k, const int* __restrict__ seg_ptr,
                                                 const int* __restrict__ col32, const int* __restrict__ perm, unsigned fl) {
    int r = -1;
    if (!(fl & GNNCCA_GRAPH_BAD_INDEX)) {
        const bool unsorted = (fl & GNNCCA_GRAPH_UNSORTED) != 0;
        const int i = (int)ei[k], j = (int)ei[E + k];
        for (int q = seg_ptr[j]; q < seg_ptr[j + 1]; ++q) {
            if (col32[q] == i) {
                r = unsorted ? perm[q] : q;
                break;
            }
        }
    }
    return r;
}

// Merge phase of a round, between two barriers of the caller: best[x] holds the largest admissible key incident to root x's cluster.
// Only the LARGER root of a pair acts: it hooks itself under the smaller and ORs its mask in.  Its reads are clean -- nobody else writes
// parent[x], and its partner, matched with x alone, is not hooked this round.  A smaller or unmatched root may read a `parent` word that
// is being written: it then sees x itself or a third root t, and best[t] cannot be x's key (the key names a pair between x's cluster and
// its partner's), so it does nothing, as it should.  *merged is set to 1 by every thread that merged.
template <int BLOCK>
__device__ __forceinline__ void excl_merge_phase(int* parent, const excl_u64* best, excl_u64* mask, int n, int tid, int* merged) {
    for (int x = tid; x < n; x += BLOCK) {
        if (excl_ld(&parent[x]) != x) continue;
        const excl_u64 key = best[x];
        if (key == 0) continue;
        const int lo = excl_key_lo(key), hi = excl_key_hi(key);
        const int ra = excl_ld(&parent[lo]), rb = excl_ld(&parent[hi]);
        const int other = ra == x ? rb : ra;
        if (other < x && best[other] == key) {
            excl_st(&parent[x], other);
            atomicOr(&mask[other], mask[x]);
            *merged = 1;
        }
    }
}

// Compress phase: `parent` back to depth one (a node hangs at most two below its new root: old root -> new root, and a new root was not
// hooked this round; a word read while it is written holds its old root or its new one, and both lead to the same root), `best` cleared.
template <int BLOCK>
__device__ __forceinline__ void excl_compress_phase(int* parent, excl_u64* best, int n, int tid) {
    for (int v = tid; v < n; v += BLOCK) {
        int r = excl_ld(&parent[v]);
        for (int q = excl_ld(&parent[r]); q != r; q = excl_ld(&parent[r])) r = q;
        excl_st(&parent[v], r);
        best[v] = 0;
    }
}

}  // namespace gnncca
