#pragma once
// exclusive.cuh -- camera-exclusive identity clusters (gnncca_post_exclusive_frames): a partition of every frame's detections in which no
// cluster holds two detections of one camera, legal by construction for any number of cameras (ids in [0, 64)), computed on the device
// without a host wait.  No counterpart in the reference, whose repair of an illegal cluster (libs/utils.py:25-173, 319-386: ROUNDING /
// SPLITTING, csrc/post_host.cpp here) is tied to four cameras and runs on the host.  Part of the translation unit mpn_post.hip.
//
// The rule for frame g, threshold th (include/gnncca_mpn.h has it in full; tests/exclusive_oracle.py restates it in numpy):
//   active      edge k is ACTIVE iff (double)scores[k] >= th; a NaN score is never active (the sweep's comparison).
//   candidates  the unordered pair {i, j} is a CANDIDATE iff the edges (i, j) and (j, i) both exist in the frame and both are active
//               (the pruning rule).
//   weight      w = min(scores[i -> j], scores[j -> i]), an exact fp32.
//   order       candidates by descending w; ties to the smaller lo = min(i, j), then the smaller hi.  A strict total order.
//   clustering  every node is a cluster with camera mask 1 << cam.  Walk the candidates in that order; merge the two clusters of a
//               candidate iff they differ and their masks are disjoint; the merged mask is the OR.
// The kernel does not walk: it runs MUTUAL-BEST ROUNDS.  A candidate is admissible while its clusters differ and their masks are
// disjoint.  In a round every cluster takes the first admissible candidate incident to it; a candidate that both of its clusters took is
// merged.  That is the same partition: the first admissible candidate overall is first for both of its clusters, so every round with an
// admissible candidate merges; a candidate chosen by both sides is preceded by no admissible candidate touching either cluster, and the
// walk's earlier merges elsewhere touch neither cluster's mask, so the walk merges it too; and admissibility only shrinks as clusters
// grow, so a candidate the walk skipped stays skipped.  Mutual choices form a matching: the merges of one round do not conflict.
//
// 64-bit key of a candidate: (fp32 bits of w) << 24 | (4095 - lo) << 12 | (4095 - hi), frame-local ids.  w > 0 (th > 0), so positive
// floats order as their bits do: the LARGEST key is the FIRST candidate, the key alone names the pair, and 0 is no key.  Every use of the
// keys is an integer maximum (LDS atomicMax on 64-bit words): neither the order in which a frame's keys are appended to its list nor the
// order in which lanes arrive changes a bit of the result.  No float atomics anywhere.
#include "excl_common.cuh"   // the activity test, the key codec, the reverse-edge search, the merge and compress phases: shared with the sweep

namespace gnncca {

// One thread per edge: rev[k] = the edge (dst k, src k) or -1, searched in the CSR segment of dst k as post_prune_kernel and
// eval_sweep_prepare_kernel search it (a plan with GNNCCA_GRAPH_BAD_INDEX gives no edge a reverse).  Thread 0 of the launch also zeroes
// *n_clusters, which the frames' workgroups add to in the next launch: the entry point needs no memset, its stream holds kernels only.
// Launched with at least one block also when E == 0 (nothing but the zero is written then; the plan's words are not read).
__global__ __launch_bounds__(256) void excl_prepare_kernel(const long long* __restrict__ ei, long long E, const int* __restrict__ seg_ptr,
                                                           const int* __restrict__ col32, const int* __restrict__ perm,
                                                           const unsigned* __restrict__ flags, int* __restrict__ rev,
                                                           int* __restrict__ n_clusters) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k == 0) *n_clusters = 0;
    if (k >= E) return;
    rev[k] = excl_reverse_edge(ei, E, k, seg_ptr, col32, perm, flags[0]);
}

// Workgroup g: frame g.  Dynamic LDS: best u64 [P] | mask u64 [P] | parent int [P] | 8 ints (20 P + 32 bytes: 80 KiB at 4096 nodes).
// First the frame's candidate list: the thread of an edge k with src < dst whose pair is a candidate appends the pair's key at
// cand[edge_ptr[g] + (a counter in LDS)++] -- at most one key per edge of the frame, so the list stays inside the frame's own edge range
// whatever the workspace held before.  `parent` is kept at depth one between rounds (parent[v] IS v's root), and the larger root always
// goes under the smaller, so a cluster's root is its smallest node: post_cc_kernel's label convention.  *n_clusters must be zero on entry
// (excl_prepare_kernel).
// flags_out[g]: GNNCCA_EXCLUSIVE_BAD_CAMERA (a camera id outside [0, 64): every node its own cluster, predictions 0, cut 0) or
// GNNCCA_EXCLUSIVE_BAD_RANGE (ranges that do not fit: the same, as far as the ranges allow writing at all).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void excl_cluster_kernel(const long long* __restrict__ ei, long long E, const float* __restrict__ scores,
                                                             double th, const int* __restrict__ cam, const int* __restrict__ rev,
                                                             excl_u64* __restrict__ cand, int N_all,
                                                             const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int P,
                                                             long long* __restrict__ preds, int* __restrict__ labels,
                                                             int* __restrict__ n_clusters, int* __restrict__ cut,
                                                             unsigned* __restrict__ flags_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_excl[];
    excl_u64* best = reinterpret_cast<excl_u64*>(s_excl);
    excl_u64* mask = best + P;
    int* parent = reinterpret_cast<int*>(mask + P);
    int* s_misc = parent + P;   // [0] a merge happened this round, [1] a camera id out of range, [2] roots, [3] cut pairs, [4] candidates
    const int g = blockIdx.x, tid = threadIdx.x;
    const int v0 = node_ptr[g], v1 = node_ptr[g + 1];
    const long long k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
    const int n = v1 - v0;
    if (!excl_frame_ok(v0, v1, k0, k1, N_all, E, P)) {
        frame_singletons<BLOCK>(labels, n_clusters, v0, v1, N_all, tid);
        if (k0 >= 0 && k1 >= k0 && k1 <= E)
            for (long long k = k0 + tid; k < k1; k += BLOCK) preds[k] = 0;
        if (tid == 0) cut[g] = 0, flags_out[g] = GNNCCA_EXCLUSIVE_BAD_RANGE;
        return;
    }
    if (tid < 8) s_misc[tid] = 0;
    __syncthreads();
    for (int v = tid; v < n; v += BLOCK) {
        const int c = cam[v0 + v];
        if ((unsigned)c >= (unsigned)kExclMaxCams) s_misc[1] = 1;
        parent[v] = v;
        mask[v] = 1ull << (c & 63);
        best[v] = 0;
    }
    __syncthreads();
    if (s_misc[1]) {
        frame_singletons<BLOCK>(labels, n_clusters, v0, v1, N_all, tid);   // (the ranges fit: its guard holds)
        for (long long k = k0 + tid; k < k1; k += BLOCK) preds[k] = 0;
        if (tid == 0) cut[g] = 0, flags_out[g] = GNNCCA_EXCLUSIVE_BAD_CAMERA;
        return;
    }
    excl_u64* mine = cand + k0;
    for (long long k = k0 + tid; k < k1; k += BLOCK) {
        const long long r = rev[k];
        if (r < k0 || r >= k1) continue;                    // the reverse edge must be the frame's own (SweepPred)
        const long long a = ei[k] - v0, b = ei[E + k] - v0;
        if (a < 0 || a >= b || b >= n) continue;            // one thread per pair; an edge that leaves its frame: ignored (post_cc_kernel)
        const float sk = scores[k], sr = scores[r];
        if (!excl_active(sk, th) || !excl_active(sr, th)) continue;
        mine[atomicAdd(&s_misc[4], 1)] = excl_key(fminf(sk, sr), (int)a, (int)b);   // (one append per edge of the frame at most: the slot is below k1 - k0)
    }
    __syncthreads();
    const int n_cand = s_misc[4];
    for (int round = 0; round < n; ++round) {   // a round with an admissible candidate merges: n - 1 merges at most.  The bound is never
        //                                         the reason to stop; it is there so that no input can make the loop spin.
        if (tid == 0) s_misc[0] = 0;            // (last read before the barrier that ended the previous round)
        for (int c = tid; c < n_cand; c += BLOCK) {
            const excl_u64 key = mine[c];
            if (key == 0) continue;             // dropped in an earlier round
            const int lo = excl_key_lo(key), hi = excl_key_hi(key);   // (both below n: written above)
            const int ra = parent[lo], rb = parent[hi];   // roots: nothing writes `parent` in this phase
            if (ra != rb && (mask[ra] & mask[rb]) == 0) {
                atomicMax(&best[ra], key);
                atomicMax(&best[rb], key);
            } else {
                mine[c] = 0;                    // admissibility only shrinks: inadmissible once, inadmissible for good
            }
        }
        __syncthreads();
        excl_merge_phase<BLOCK>(parent, best, mask, n, tid, &s_misc[0]);   // the mutual choices merge (excl_common.cuh)
        __syncthreads();
        excl_compress_phase<BLOCK>(parent, best, n, tid);                  // `parent` back to depth one, `best` cleared
        const int merged = s_misc[0];
        __syncthreads();
        if (!merged) break;
    }
    int roots = 0, cuts = 0;
    for (int v = tid; v < n; v += BLOCK) {
        const int r = parent[v];
        labels[v0 + v] = v0 + r;
        roots += r == v;
    }
    for (long long k = k0 + tid; k < k1; k += BLOCK) {
        long long p = 0;
        const long long r = rev[k];
        if (r >= k0 && r < k1 && excl_active(scores[k], th) && excl_active(scores[r], th)) {
            const long long a = ei[k] - v0, b = ei[E + k] - v0;
            if (a >= 0 && a < n && b >= 0 && b < n && a != b) {   // a candidate pair of this frame
                const bool same = parent[a] == parent[b];
                p = same ? 1 : 0;
                cuts += (!same && a < b) ? 1 : 0;
            }
        }
        preds[k] = p;
    }
    if (roots) atomicAdd(&s_misc[2], roots);
    if (cuts) atomicAdd(&s_misc[3], cuts);
    __syncthreads();
    if (tid == 0) {
        if (s_misc[2]) atomicAdd(n_clusters, s_misc[2]);
        cut[g] = s_misc[3];
        flags_out[g] = 0;
    }
}

}  // namespace gnncca
