#pragma once
// eval_sweep_exclusive.cuh -- every operating point of a batch scored on its CAMERA-EXCLUSIVE partition in one pass
// (gnncca_eval_sweep_exclusive).  eval_sweep.cuh scores the connected components of the pruned edges; the partition that
// gnncca_post_exclusive_frames ships (exclusive.cuh) is another one, and a threshold chosen on the first says nothing about the second.
// Part of the translation unit evaluate.hip (fp contract(off)): the scoring is eval_frame_body itself, the rounds' merge and compress
// phases are excl_common.cuh's, the ones excl_cluster_kernel runs.
//
// The rule for threshold t and frame g is nothing new: rows[t][g] = gnncca_eval_frames of the `predictions` and `labels` that
// gnncca_post_exclusive_frames(threshold = thresholds[t]) returns, bit for bit, and labels[t] = those labels.
//
// What makes one pass cheap: a pair's key (excl_key: fp32 bits of w = min of its two scores, then the two local ids) does not depend on
// the threshold, and the candidates at threshold th are exactly the pairs with (double)w >= th -- w IS one of the two scores, so this is
// the comparison "both edges active".  One key array per batch, slot k for the edge k with src < dst of a pair, serves every threshold
// read-only: the workspace stays O(E + N).  The T workgroups of a frame share the slots, so none of them writes there; a workgroup
// re-tests a slot's admissibility every round (two `parent` and two `mask` reads in LDS) where excl_cluster_kernel drops the slot.
// The order among the candidates of a threshold is the order of their keys, as in excl_cluster_kernel: the same rounds, the same bits.
//
// Launches (their number does not depend on T): the graph plan, the plan finish, eval_sweep_excl_prepare_kernel, eval_sweep_excl_kernel
// with grid (G, T).  Kernels only: nothing is counted or compacted, so nothing needs a memset.
namespace gnncca {

// Blocks [0, edge_blocks): one edge per thread.  rev[k] = the edge (dst k, src k) or -1, and keys[k] = the key of the pair of edge k iff
// src k < dst k, the reverse edge lies in the same frame as k, both ends lie in the frame, and both scores are not NaN and > 0; 0
// otherwise.  EVERY slot is written.  The frame of edge k is the last g with edge_ptr[g] <= k, checked (edge_ptr[g] <= k < edge_ptr[g + 1]
// and ranges that pass excl_frame_ok with the sweep kernel's P): with ranges that do not ascend a slot can only become 0 or the key of a
// pair of the frame found, and the sweep kernel checks the ids of every key against its own frame.
// Blocks [edge_blocks, edge_blocks + G): frame g's lgamma table, as eval_sweep_prepare_kernel fills it (fill_lgamma_table).
__global__ __launch_bounds__(256) void eval_sweep_excl_prepare_kernel(const long long* __restrict__ ei, long long E, const int* __restrict__ seg_ptr,
                                                                      const int* __restrict__ col32, const int* __restrict__ perm,
                                                                      const unsigned* __restrict__ flags, const float* __restrict__ scores,
                                                                      int* __restrict__ rev, excl_u64* __restrict__ keys, int edge_blocks,
                                                                      const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int G,
                                                                      int N_all, int P, double* __restrict__ lf_ws) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < edge_blocks) {
        const long long k = (long long)blockIdx.x * 256 + tid;
        if (k >= E) return;
        const int r = excl_reverse_edge(ei, E, k, seg_ptr, col32, perm, flags[0]);
        rev[k] = r;
        excl_u64 key = 0;
        if (r >= 0) {
            int g = 0, above = G;   // the last g in [0, G) with edge_ptr[g] <= k (empty frames in front of k's are stepped over)
            while (above - g > 1) {
                const int mid = (g + above) >> 1;
                if (edge_ptr[mid] <= k) g = mid;
                else above = mid;
            }
            const long long k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
            const int v0 = node_ptr[g], v1 = node_ptr[g + 1];
            if (k0 <= k && k < k1 && r >= k0 && r < k1 && excl_frame_ok(v0, v1, k0, k1, N_all, E, P)) {
                const long long a = ei[k] - v0, b = ei[E + k] - v0;
                if (a >= 0 && a < b && b < v1 - v0) {   // one key per pair; an edge that leaves its frame: none
                    const float sk = scores[k], sr = scores[r];
                    if (sk > 0.f && sr > 0.f) key = excl_key(fminf(sk, sr), (int)a, (int)b);   // (false for a NaN)
                }
            }
        }
        keys[k] = key;
        return;
    }
    const int g = (int)blockIdx.x - edge_blocks;
    const int v0 = node_ptr[g], v1 = node_ptr[g + 1];
    const int n = v1 - v0;
    if (v0 < 0 || n < 0 || n > kEvalMaxNodes || v1 > N_all) return;   // a NaN row: nobody reads its table
    fill_lgamma_table(lf_ws + v0 + g, n, tid, 256);
}

// "is edge k predicted" of the exclusive sweep -- the epilogue of excl_cluster_kernel: the reverse edge is the frame's own, both are
// active at th, both ends lie in the frame and differ, and the ends have one root.  `dead`: a camera id outside [0, 64) (predictions 0).
struct SweepExclPred {
    const long long* __restrict__ ei;
    long long E;
    const float* __restrict__ scores;
    const int* __restrict__ rev;
    const unsigned short* lab16;
    double th;
    long long k0, k1;
    int v0, n;
    bool dead;
    __device__ __forceinline__ long long operator()(long long k) const {
        if (dead) return 0;
        const long long r = rev[k];
        if (r < k0 || r >= k1 || !excl_active(scores[k], th) || !excl_active(scores[r], th)) return 0;
        const long long a = ei[k] - v0, b = ei[E + k] - v0;
        if (a < 0 || a >= n || b < 0 || b >= n || a == b) return 0;
        return lab16[a] == lab16[b] ? 1 : 0;
    }
};

// Workgroup (g, t): frame g at thresholds[t].  Dynamic LDS, 20 P bytes (80 KiB at 4096 nodes, excl_cluster_kernel's footprint):
//   the rounds   best u64 [P] at [0, 8P) | mask u64 [P] at [8P, 16P) | parent int [P] at [16P, 20P)
//   the scoring  eval_frame_body's three int regions at [0, 12P) | the 16-bit labels SweepLabel reads at [12P, 14P)
// `best` and `mask` are dead when the rounds end, `parent` (depth one: parent[v] IS v's root) lies above everything the scoring touches:
// after the last round's barrier the roots go from `parent` into the label words -- over the middle of `mask` -- and after one more
// barrier the body starts and initialises its own regions, as it does for every caller.  Nothing is copied twice and nothing is added to
// the 20 P the rounds need anyway, so two workgroups of the largest frame fit a CU's 160 KiB, as with excl_cluster_kernel.
// A frame whose ranges do not fit: a NaN row (eval_sweep_kernel's test and its identity labels).  A camera id outside [0, 64): every
// node its own cluster, predictions 0, scored as such -- what the loop over gnncca_post_exclusive_frames + gnncca_eval_frames gives.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void eval_sweep_excl_kernel(const long long* __restrict__ ei, long long E, const float* __restrict__ elab,
                                                                const float* __restrict__ scores, const int* __restrict__ cam,
                                                                const int* __restrict__ rev, const excl_u64* __restrict__ keys,
                                                                const double* __restrict__ thresholds, int N_all,
                                                                const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int P,
                                                                double* __restrict__ rows_out, int* __restrict__ labels_out,
                                                                double* __restrict__ lf_ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_sweep_excl[];   // (the same bytes as eval_frame_body's s_dyn)
    __shared__ int s_flag[2];   // [0] a merge happened this round, [1] a camera id out of range
    excl_u64* best = reinterpret_cast<excl_u64*>(s_sweep_excl);
    excl_u64* mask = best + P;
    int* parent = reinterpret_cast<int*>(mask + P);
    unsigned short* lab16 = reinterpret_cast<unsigned short*>(s_sweep_excl + (size_t)12 * P);
    const int g = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const SweepOut out = sweep_out(rows_out, labels_out, g, t, gridDim.x, N_all);
    const int v0 = node_ptr[g], v1 = node_ptr[g + 1];
    const long long k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
    const int n = v1 - v0;
    if (!excl_frame_ok(v0, v1, k0, k1, N_all, E, P)) {   // eval_sweep_frame's test and answer: a NaN row, identity labels
        if (tid < 16) out.row[tid] = __builtin_nan("");
        if (out.lab_t && v0 >= 0 && v1 <= N_all)
            for (int v = v0 + tid; v < v1; v += BLOCK) out.lab_t[v] = v;
        return;
    }
    const double th = thresholds[t];
    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    for (int v = tid; v < n; v += BLOCK) {
        const int c = cam[v0 + v];
        if ((unsigned)c >= (unsigned)kExclMaxCams) s_flag[1] = 1;
        parent[v] = v;
        mask[v] = 1ull << (c & 63);
        best[v] = 0;
    }
    __syncthreads();
    const bool dead = s_flag[1] != 0;
    for (int round = 0; round < n && !dead; ++round) {   // (excl_cluster_kernel's loop: the bound is never the reason to stop)
        if (tid == 0) s_flag[0] = 0;                     // (last read before the barrier that ended the previous round)
        for (long long k = k0 + tid; k < k1; k += BLOCK) {
            const excl_u64 key = keys[k];
            if (key == 0 || !excl_active(excl_key_weight(key), th)) continue;   // no pair here, or not a candidate at this threshold
            const int lo = excl_key_lo(key), hi = excl_key_hi(key);
            if (hi >= n) continue;                        // (lo < hi; never true for ranges that ascend)
            const int ra = parent[lo], rb = parent[hi];   // roots: nothing writes `parent` in this phase
            if (ra != rb && (mask[ra] & mask[rb]) == 0) {
                atomicMax(&best[ra], key);
                atomicMax(&best[rb], key);
            }
        }
        __syncthreads();
        excl_merge_phase<BLOCK>(parent, best, mask, n, tid, &s_flag[0]);
        __syncthreads();
        excl_compress_phase<BLOCK>(parent, best, n, tid);
        const int merged = s_flag[0];
        __syncthreads();
        if (!merged) break;
    }
    for (int v = tid; v < n; v += BLOCK) {   // (`mask` is dead: its last read lies before the barrier above)
        const int r = parent[v];
        lab16[v] = (unsigned short)r;
        if (out.lab_t) out.lab_t[v0 + v] = v0 + r;
    }
    __syncthreads();
    const SweepExclPred pred{ei, E, scores, rev, lab16, th, k0, k1, v0, n, dead};
    eval_frame_body<BLOCK, false, false>(g, out.row, ei, E, elab, pred, SweepLabel{lab16}, N_all, node_ptr, edge_ptr, P, nullptr, lf_ws, nullptr,
                                         nullptr);
}

}  // namespace gnncca
