#pragma once
// eval_sweep.cuh -- every operating point of a batch in one pass (gnncca_eval_sweep): what the reference's threshold sweeps do one
// threshold at a time on the host (main.py:124-319, MODE REID: 100 thresholds over the ReID distances, compute_P_R_F at each, the
// threshold of maximal F; the OPT_TH / GEOM_TH tables of config_inference.yaml are such sweeps' results).  Part of the translation unit
// evaluate.hip (compiled with fp contract(off)): the scoring is eval_frame_body itself, not a copy.
//
// The rule for threshold t and frame g -- exactly what threshold -> prune_and_cluster -> evaluate_frames compute one threshold at a time:
//   activity   edge k is ACTIVE iff (double)scores[k] >= thresholds[t] (keep_le: <=).  The comparison is made in fp64 against the
//              widened fp32 score; a NaN score is never active.
//   pruning    edge k is KEPT iff it is active and an edge (dst k, src k) of the same frame exists and is active (post_prune_kernel).
//   partition  labels[t] = the connected components of the kept edges inside the frame, a node's label the smallest batch-global id
//              of its component (post_cc_kernel's convention).
//   scores     rows[t][g] = the 16 columns of gnncca_eval_frames for those kept predictions and that partition.
// Edge lists with duplicate ordered pairs are unspecified (the first reverse edge found in the plan's order is the one consulted).
//
// Launches (their number does not depend on T): the graph plan (plan_only + plan finish, as gnncca_post_prune_cluster makes it without
// a handed-over plan), eval_sweep_prepare_kernel (the reverse edge of every edge from the plan's CSR, and the per-frame lgamma tables
// the scoring reads), eval_sweep_kernel with grid (G, T).  No prediction vector exists anywhere: a workgroup judges an edge from its
// score and its reverse edge's score when it needs it.  The workgroup's work is written for any such judgement (eval_sweep_frame,
// eval_sweep_body<BLOCK, PredF>): eval_sweep_joint.cuh runs it with a conjunction of conditions.
namespace gnncca {

// rev[k] = the edge (dst k, src k), or -1.  Blocks [0, edge_blocks): one edge per thread, searched in the CSR segment of dst k as
// post_prune_kernel does (a plan with GNNCCA_GRAPH_BAD_INDEX prunes everything there: no edge has a reverse here).
// Blocks [edge_blocks, edge_blocks + G): frame g's lgamma table, lf[k] = lgamma(k + 1) for k <= n_g at lf_ws + node_ptr[g] + g, written
// by fill_lgamma_table like eval_frame_body<.., FILL_LF = true>'s.
__global__ __launch_bounds__(256) void eval_sweep_prepare_kernel(const long long* __restrict__ ei, long long E, const int* __restrict__ seg_ptr,
                                                                 const int* __restrict__ col32, const int* __restrict__ perm,
                                                                 const unsigned* __restrict__ flags, int* __restrict__ rev, int edge_blocks,
                                                                 const int* __restrict__ node_ptr, int N_all, double* __restrict__ lf_ws) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < edge_blocks) {
        const long long k = (long long)blockIdx.x * 256 + tid;
        if (k >= E) return;
        rev[k] = excl_reverse_edge(ei, E, k, seg_ptr, col32, perm, flags[0]);   // (excl_common.cuh: one search for every prepare kernel)
        return;
    }
    const int g = (int)blockIdx.x - edge_blocks;
    const int v0 = node_ptr[g], v1 = node_ptr[g + 1];
    const int n = v1 - v0;
    if (v0 < 0 || n < 0 || n > kEvalMaxNodes || v1 > N_all) return;   // a NaN row: nobody reads its table
    fill_lgamma_table(lf_ws + v0 + g, n, tid, 256);
}

// "is edge k predicted" of the sweep: active, and the reverse edge of the same frame is active too
struct SweepPred {
    const float* __restrict__ scores;
    const int* __restrict__ rev;
    double th;
    long long k0, k1;   // the frame's edges
    bool le;
    __device__ __forceinline__ bool active(long long k) const {
        const double s = (double)scores[k];
        return le ? s <= th : s >= th;   // (false for a NaN either way)
    }
    __device__ __forceinline__ long long operator()(long long k) const {
        if (!active(k)) return 0;
        const long long r = rev[k];
        return (r >= k0 && r < k1 && active(r)) ? 1 : 0;
    }
};
// "label of node v" of the sweep: the frame-local root the workgroup left in LDS (12-bit ids in 16-bit words)
struct SweepLabel {
    const unsigned short* lab16;
    __device__ __forceinline__ int operator()(int v0, int v) const { return v0 + (int)lab16[v]; }
};

// Where workgroup (g, t) of a sweep writes: its row of rows_out [T][G][16] and point t's labels in labels_out [T][N_all] (null: none).
struct SweepOut {
    double* row;
    int* lab_t;
};
__device__ __forceinline__ SweepOut sweep_out(double* rows_out, int* labels_out, int g, int t, int n_frames, int N_all) {
    return SweepOut{rows_out + ((size_t)t * n_frames + g) * 16, labels_out ? labels_out + (size_t)t * N_all : nullptr};
}

// The part of a sweep workgroup that comes before the predicate exists: the frame's ranges.  A frame whose ranges do not fit
// (eval_frame_body's test) gets a NaN row and identity labels, and the workgroup is done (false).
struct SweepFrame {
    int v0, n;
    long long k0, k1;
};
template <int BLOCK>
__device__ __forceinline__ bool eval_sweep_frame(int g, int N_all, long long E, const int* __restrict__ node_ptr,
                                                 const int* __restrict__ edge_ptr, int P_lds, double* __restrict__ row, int* __restrict__ lab_t,
                                                 SweepFrame& f) {
    const int tid = threadIdx.x;
    const int v0 = node_ptr[g], v1 = node_ptr[g + 1];
    const long long k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
    const int n = v1 - v0;
    f = SweepFrame{v0, n, k0, k1};
    if (v0 < 0 || n < 0 || n > P_lds || v1 > N_all || k0 < 0 || k1 < k0 || k1 > E) {   // eval_frame_body's test: a NaN row
        if (tid < 16) row[tid] = __builtin_nan("");
        if (lab_t && v0 >= 0 && v1 <= N_all)
            for (int v = v0 + tid; v < v1; v += BLOCK) lab_t[v] = v;
        return false;
    }
    return true;
}

// The workgroup body of every sweep over the connected components, written once for every predicate (`pred(k)`: 1 iff edge k is kept at
// this workgroup's operating point -- SweepPred here, SweepJointPred in eval_sweep_joint.cuh).  The partition first -- union-find over
// the kept edges in eval_frame_body's `parent` region (which the body initialises again), the larger root hooked under the smaller by
// compare-and-swap, so that a component's root is its smallest node, then every node's root into a fourth LDS region of P_lds 16-bit
// words -- then the scoring body.  LDS: 3.5 x P_lds ints (56 KiB at 4096 nodes) + the body's ~2 KiB.
template <int BLOCK, class PredF>
__device__ __forceinline__ void eval_sweep_body(int g, const SweepFrame f, const PredF pred, const long long* __restrict__ ei, long long E,
                                                const float* __restrict__ elab, int N_all, const int* __restrict__ node_ptr,
                                                const int* __restrict__ edge_ptr, int P_lds, double* __restrict__ row,
                                                int* __restrict__ lab_t, double* __restrict__ lf_ws) {
    extern __shared__ int s_dyn[];
    int* parent = s_dyn;
    unsigned short* lab16 = reinterpret_cast<unsigned short*>(s_dyn + 3 * P_lds);
    const int tid = threadIdx.x;
    const int v0 = f.v0, n = f.n;
    const long long k0 = f.k0, k1 = f.k1;
    for (int v = tid; v < n; v += BLOCK) parent[v] = v;
    __syncthreads();
    for (long long k = k0 + tid; k < k1; k += BLOCK) {
        if (pred(k) != 1) continue;
        const long long a = ei[k] - v0, b = ei[E + k] - v0;
        if (a < 0 || a >= n || b < 0 || b >= n) continue;   // an edge that leaves its frame: ignored (post_cc_kernel)
        int ra = (int)a, rb = (int)b;
        while (true) {   // (a failed swap means another thread hooked that root: at most n hooks in all)
            for (int q = lds_load(&parent[ra]); q != ra; q = lds_load(&parent[ra])) ra = q;
            for (int q = lds_load(&parent[rb]); q != rb; q = lds_load(&parent[rb])) rb = q;
            if (ra == rb) break;
            const int hi = max(ra, rb), lo = min(ra, rb);
            if (atomicCAS(&parent[hi], hi, lo) == hi) break;
        }
    }
    __syncthreads();
    for (int v = tid; v < n; v += BLOCK) {   // (the forest no longer changes: nothing below writes `parent`)
        int r = v;
        for (int q = parent[r]; q != r; q = parent[r]) r = q;
        lab16[v] = (unsigned short)r;
        if (lab_t) lab_t[v0 + v] = v0 + r;
    }
    __syncthreads();
    eval_frame_body<BLOCK, false, false>(g, row, ei, E, elab, pred, SweepLabel{lab16}, N_all, node_ptr, edge_ptr, P_lds, nullptr, lf_ws,
                                         nullptr, nullptr);
}

// Workgroup (g, t): frame g at thresholds[t].  labels_out (nullable): int32 [T][N_all].
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void eval_sweep_kernel(const long long* __restrict__ ei, long long E, const float* __restrict__ elab,
                                                           const float* __restrict__ scores, const int* __restrict__ rev,
                                                           const double* __restrict__ thresholds, int keep_le, int N_all,
                                                           const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int P_lds,
                                                           double* __restrict__ rows_out, int* __restrict__ labels_out,
                                                           double* __restrict__ lf_ws) {
    const int g = blockIdx.x, t = blockIdx.y;
    const SweepOut out = sweep_out(rows_out, labels_out, g, t, gridDim.x, N_all);
    SweepFrame f;
    if (!eval_sweep_frame<BLOCK>(g, N_all, E, node_ptr, edge_ptr, P_lds, out.row, out.lab_t, f)) return;
    const SweepPred pred{scores, rev, thresholds[t], f.k0, f.k1, keep_le != 0};
    eval_sweep_body<BLOCK>(g, f, pred, ei, E, elab, N_all, node_ptr, edge_ptr, P_lds, out.row, out.lab_t, lf_ws);
}

}  // namespace gnncca
