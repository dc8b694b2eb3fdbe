#pragma once
// strong.cuh -- identity clusters WITHOUT pruning (gnncca_post_strong_frames): the strongly connected components of the digraph of a
// frame's active edges, which is what the reference's utils.compute_SCC_and_Clusters (libs/utils.py:295-317) returns when PRUNING is
// False (config_inference.yaml:7; inference.py:302-304, 733-738, 904-908): a directed cycle without a single mutual pair is one identity.
// post_cc_kernel (postprocess.cuh) computes the components of a SYMMETRIC edge set and is only ever fed pruned edges; this is the other
// half.  Part of the translation unit mpn_post.hip.
//
// One workgroup per frame, no graph plan, no CSR, the edge list in any order, the frame's contiguous edge range read once.
//   active       edge k of frame g is ACTIVE iff predictions[k] == 1 and both ends lie in [node_ptr[g], node_ptr[g + 1]) (post_cc_kernel's
//                rule: everything else is ignored).  Self loops and duplicate edges are harmless.
//   reachability a bit matrix R in LDS: n_pad rows of W = n_pad / 32 words, n_pad = the frame's node count rounded up to 32.  The diagonal
//                is set, an active edge (a, b) sets bit b of row a (atomicOr on LDS).
//   closure      repeated squaring IN PLACE: the owner of (row i, word w) ORs in word w of every row j whose bit is set in row i.  Every
//                word has exactly one writer.  A reader may see another row before or after that row's update of the same round; both are
//                sound, because every set bit is a true reachability fact at all times -- so the in-place form reaches the fixpoint at
//                least as fast as the two-buffer form, which covers paths of 2^r edges after round r.  A simple path has fewer than n_pad
//                edges: ceil(log2(n_pad)) rounds complete the closure whatever the data, and one more detects it.  The loop is COUNTED,
//                `for (round = 0; round < ceil(log2(n_pad)) + 1; ++round)` (11 rounds at 1024 nodes), with an early exit after a round that
//                changed nothing; there is no "until fixpoint".  (Label propagation would need O(n^2) barrier rounds on a chain of 2-cycles.)
//   labels       labels[v] = the smallest batch-global node id u with R[v][u] && R[u][v]: the set bits of row v are scanned ascending and
//                the scan ends at the first hit, v itself at the latest.  post_cc_kernel's label convention (csrc/post_host.cpp and every
//                consumer of labels rely on it).
//   counters     flow_out[v] / flow_in[v] of the active (unpruned) edges: integer atomic adds in global memory; the returned old value tells
//                the adding thread whether the count went above 3 (counts only grow, so SOME add sees the final count): trigger bit 0
//                without a second pass.  Bit 1: a component with more than four members, counted over the labels in the first n words of
//                R once the matrix is no longer needed.  *n_clusters += the frame's nodes with labels[v] == v.
// Nothing depends on the order in which threads or edges arrive (ORs, integer adds, a scan in id order): two runs give the same bits, and
// a frame's result does not depend on the rest of the batch.  flow_out / flow_in / *n_clusters must be zero on entry.
// flags_out[g] = GNNCCA_STRONG_BAD_RANGE: the frame's ranges do not fit (excl_frame_ok, the LDS capacity P included); every node of such a
// frame is its own cluster, its flows and its trigger word are 0 -- as far as the ranges allow writing at all.
#include "excl_common.cuh"   // frame_range, excl_frame_ok, frame_singletons: one reading, one test and one refusal of a frame's ranges in this unit
#include "strong_closure.cuh"   // the matrix's diagonal, its closure and a node's label: shared with the sweep over this partition

namespace gnncca {

constexpr int kStrongMaxNodes = GNNCCA_STRONG_MAX_FRAME_NODES;

// Workgroup g: frame g (node_ptr / edge_ptr null: the whole graph is the one frame).  Dynamic LDS: R, P * (P / 32) words, P = the largest
// frame rounded up to 32 (128 B at 32 nodes, 2 KiB at 128, 128 KiB at 1024).  The launcher picks BLOCK >= P, so a thread owns at most one
// node in the label phase; a frame uses its own n_pad and row stride, not P's.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void strong_cluster_kernel(const long long* __restrict__ ei, const long long* __restrict__ pred, long long E,
                                                               int N_all, const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr,
                                                               int P, int* __restrict__ flow_out, int* __restrict__ flow_in,
                                                               int* __restrict__ labels, int* __restrict__ n_clusters,
                                                               int* __restrict__ triggers, unsigned* __restrict__ flags_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_strong[];
    __shared__ int s_round[kStrongMaxRounds];   // [r]: round r changed a word
    __shared__ int s_misc[2];                   // [0] roots, [1] trigger bits
    unsigned* R = reinterpret_cast<unsigned*>(s_strong);
    const int g = blockIdx.x, tid = threadIdx.x;
    const FrameRange fr = frame_range(node_ptr, edge_ptr, g, N_all, E);
    const int v0 = fr.v0, v1 = fr.v1, n = v1 - v0;
    const long long k0 = fr.k0, k1 = fr.k1;
    if (!excl_frame_ok(v0, v1, k0, k1, N_all, E, min(P, BLOCK))) {
        frame_singletons<BLOCK>(labels, n_clusters, v0, v1, N_all, tid);
        if (tid == 0) triggers[g] = 0, flags_out[g] = GNNCCA_STRONG_BAD_RANGE;
        return;
    }
    const int W = (n + 31) >> 5;   // n_pad = 32 W (n <= P: W * n_pad words fit the launch's LDS)
    if (tid < kStrongMaxRounds) s_round[tid] = 0;
    if (tid < 2) s_misc[tid] = 0;
    strong_diagonal<BLOCK>(R, n, W);
    __syncthreads();
    int trig = 0;
    for (long long k = k0 + tid; k < k1; k += BLOCK) {
        if (pred[k] != 1) continue;
        const long long a = ei[k], b = ei[E + k];
        if (a < v0 || a >= v1 || b < v0 || b >= v1) continue;   // out of range, or an edge that leaves its frame: ignored
        const int la = (int)a - v0, lb = (int)b - v0;
        atomicOr(&R[la * W + (lb >> 5)], 1u << (lb & 31));
        // counts only grow: the add that brings a count to its final value sees it
        if (atomicAdd(&flow_out[a], 1) >= 3) trig = GNNCCA_POST_TRIGGER_ROUNDING;
        if (atomicAdd(&flow_in[b], 1) >= 3) trig = GNNCCA_POST_TRIGGER_ROUNDING;
    }
    __syncthreads();
    strong_close<BLOCK>(R, n, W, s_round);
    // labels: one node per thread (n <= BLOCK)
    const int v = tid;
    int lab = v;
    if (v < n) {
        lab = strong_root(R, W, v);
        labels[v0 + v] = v0 + lab;
    }
    __syncthreads();   // R is no longer read as a matrix: its first n words (words >= n_pad >= n) count the members of every root
    if (v < n) R[v] = 0;
    __syncthreads();
    if (v < n) atomicAdd(&R[lab], 1u);
    __syncthreads();
    if (v < n && lab == v) {
        atomicAdd(&s_misc[0], 1);
        if (R[v] > 4u) trig |= GNNCCA_POST_TRIGGER_SPLITTING;
    }
    if (trig) atomicOr(&s_misc[1], trig);
    __syncthreads();
    if (tid == 0) {
        if (s_misc[0]) atomicAdd(n_clusters, s_misc[0]);
        triggers[g] = s_misc[1];
        flags_out[g] = 0;
    }
}

}  // namespace gnncca
