#pragma once
// eval_sweep_joint.cuh -- every operating point of a CONJUNCTION of per-edge conditions in one pass (gnncca_eval_sweep_joint), and the
// running sums of such rows over a data set (gnncca_eval_rows_accumulate).  The reference's position baselines are such rules:
// geometrical_association keeps an edge iff its ground distance < GEOM_TH / max_dist (inference.py:722-724), and
// geometrical_appearance_association iff that holds AND its ReID distance < th (inference.py:896); the GEOM_TH / OPT_TH tables they read
// were swept one axis at a time on the host.  Part of the translation unit evaluate.hip (fp contract(off)): the workgroup body is
// eval_sweep_body (eval_sweep.cuh), the one gnncca_eval_sweep runs, instantiated with another predicate; the prepare kernel is
// eval_sweep_prepare_kernel itself.
//
// The rule for point t and frame g:
//   threshold  th[k] = points[t][k] / frame_div[k][g] (one IEEE fp64 division; points[t][k] itself when frame_div is null)
//   activity   edge e is ACTIVE iff for every k < K: (double)score_k[e] cmp_k th[k], cmp_k one of >=, >, <=, <.  Compared in fp64 against
//              the widened fp32 score; a NaN score is never active under any comparator.
//   pruning, partition, scores   gnncca_eval_sweep's: kept iff the reverse edge of the same frame is active too, the connected
//              components of the kept edges, the 16 columns of gnncca_eval_frames.
// Not reproduced by THIS kernel: the reference clusters with the strongly connected components of the digraph of active edges and does not
// prune, so a directed cycle without a mutual pair joins nodes there (possible when a score is not symmetric: F.pairwise_distance adds
// eps to a - b); here only mutual pairs join.  eval_sweep_strong.cuh is that rule, on the same arguments.  And inference.py:892,896 use
// the LAST graph's labels and max_dist[0] for a whole batch; here every frame has its own labels and its own divisor.
//
// Launches (their number depends on neither T nor K): the graph plan, the plan finish, eval_sweep_prepare_kernel, eval_sweep_joint_kernel
// with grid (G, T).  Workspace: gnncca_eval_sweep's layout, O(E + N).
namespace gnncca {

constexpr int kJointMaxScores = GNNCCA_EVAL_JOINT_MAX_SCORES;

// the K score arrays of a joint sweep, by value in the kernel's arguments: element e of array k is p[k][e * stride[k]]
struct JointScores {
    const float* p[kJointMaxScores];
    long long stride[kJointMaxScores];
    int cmp[kJointMaxScores];   // GNNCCA_CMP_*
    int K;
};

__device__ __forceinline__ bool joint_compare(double s, int cmp, double th) {   // (false for a NaN under every comparator)
    return cmp == GNNCCA_CMP_GE ? s >= th : cmp == GNNCCA_CMP_GT ? s > th : cmp == GNNCCA_CMP_LE ? s <= th : s < th;
}

// "is edge k active" at one operating point: every condition holds on it.  The test every joint predicate is made of (the sweep over
// the strongly connected components, eval_sweep_strong.cuh, uses it alone).
struct JointActive {
    JointScores sc;
    double th[kJointMaxScores];
    __device__ __forceinline__ bool active(long long k) const {
        bool on = true;
#pragma unroll
        for (int q = 0; q < kJointMaxScores; ++q)   // (unrolled: constant indices, the arrays stay in registers)
            if (q < sc.K) on = on && joint_compare((double)sc.p[q][k * sc.stride[q]], sc.cmp[q], th[q]);
        return on;
    }
    // th[q] of workgroup (g, t): points[t][q], divided by frame_div[q][g] where given (the same operands in every thread: one value)
    __device__ __forceinline__ void set_point(const JointScores& s, const double* __restrict__ points, const double* __restrict__ frame_div,
                                              int t, int g, int n_frames) {
        sc = s;
#pragma unroll
        for (int q = 0; q < kJointMaxScores; ++q) {
            double v = 0.0;
            if (q < s.K) {
                v = points[(size_t)t * s.K + q];
                if (frame_div) v = v / frame_div[(size_t)q * n_frames + g];
            }
            th[q] = v;
        }
    }
};

// "is edge k predicted" of the joint sweep: every condition holds on it and on the reverse edge of the same frame
struct SweepJointPred : JointActive {
    const int* __restrict__ rev;
    long long k0, k1;   // the frame's edges
    __device__ __forceinline__ long long operator()(long long k) const {
        if (!active(k)) return 0;
        const long long r = rev[k];
        return (r >= k0 && r < k1 && active(r)) ? 1 : 0;
    }
};

// Workgroup (g, t): frame g at points[t].  points: fp64 [T][K]; frame_div (nullable): fp64 [K][G]; labels_out (nullable): int32 [T][N_all].
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void eval_sweep_joint_kernel(const long long* __restrict__ ei, long long E, const float* __restrict__ elab,
                                                                 const JointScores sc, const int* __restrict__ rev,
                                                                 const double* __restrict__ points, const double* __restrict__ frame_div,
                                                                 int N_all, const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr,
                                                                 int P_lds, double* __restrict__ rows_out, int* __restrict__ labels_out,
                                                                 double* __restrict__ lf_ws) {
    const int g = blockIdx.x, t = blockIdx.y;
    const int n_frames = gridDim.x;
    const SweepOut out = sweep_out(rows_out, labels_out, g, t, n_frames, N_all);
    SweepFrame f;
    if (!eval_sweep_frame<BLOCK>(g, N_all, E, node_ptr, edge_ptr, P_lds, out.row, out.lab_t, f)) return;
    SweepJointPred pred;
    pred.set_point(sc, points, frame_div, t, g, n_frames);
    pred.rev = rev, pred.k0 = f.k0, pred.k1 = f.k1;
    eval_sweep_body<BLOCK>(g, f, pred, ei, E, elab, N_all, node_ptr, edge_ptr, P_lds, out.row, out.lab_t, lf_ws);
}

// sums[t][c] = ((sums[t][c] + rows[t][0][c]) + rows[t][1][c]) + ... : one thread per (t, c), the frames in ascending g, plain fp64 adds
// (this translation unit does not contract, and there is nothing to contract).  No atomics, no tree: the order is the contract, and two
// runs give the same bits.  A NaN row makes its sums NaN.  frames (nullable): += G, by one thread.
__global__ __launch_bounds__(256) void eval_rows_accumulate_kernel(const double* __restrict__ rows, int T, int G, double* __restrict__ sums,
                                                                   long long* __restrict__ frames) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i == 0 && frames) frames[0] += G;
    if (i >= T * 16) return;
    const int t = i >> 4, c = i & 15;
    const double* r = rows + (size_t)t * G * 16 + c;
    double s = sums[i];
    for (int g = 0; g < G; ++g) s += r[(size_t)g * 16];
    sums[i] = s;
}

}  // namespace gnncca
