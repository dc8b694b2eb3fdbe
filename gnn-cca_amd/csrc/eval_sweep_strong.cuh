#pragma once
// eval_sweep_strong.cuh -- every operating point of a batch over the STRONGLY CONNECTED clusters in one pass (gnncca_eval_sweep_strong):
// the reference's rule when PRUNING is off (config_inference.yaml:7; inference.py:302-304) and the only rule of its position baselines
// (geometrical_association / geometrical_appearance_association, inference.py:733-738, 904-908): nothing is pruned, and the clusters are
// the strongly connected components of the digraph of active edges -- a directed cycle without one mutual pair is one identity.  What
// threshold -> postprocess.strong_clusters -> evaluate_frames compute one point at a time.  Part of the translation unit evaluate.hip
// (fp contract(off)): the scoring is eval_frame_body itself, the partition is strong_closure.cuh's, which strong_cluster_kernel runs.
//
// The rule for point t and frame g (K conditions; the single-score sweep is K = 1):
//   threshold    th[q] = points[t][q] / frame_div[q][g] (one IEEE fp64 division; points[t][q] itself when frame_div is null)
//   activity     edge k is ACTIVE iff for every q < K: (double)score_q[k * stride_q] cmp_q th[q] (JointActive: the fp32 score widened, the
//                comparison in fp64, a NaN score never active).  No reverse edge is consulted.
//   predictions  predictions_t[k] = active ? 1 : 0 -- the unpruned predictions
//   labels       labels_t[v] = the smallest batch-global id u of the frame with v -> u and u -> v reachable over active edges whose two
//                ends lie in the frame (an active edge that leaves its frame sets no bit; self loops and duplicates are harmless; the
//                edge list may be in any order)
//   row          rows[t][g] = the 16 columns of gnncca_eval_frames for predictions_t and labels_t
//
// One workgroup per (frame, point), grid (G, T).  Dynamic LDS, in bytes: [0, max(12 P, R bytes)) holds R first (rows of the frame's own
// W = ceil(n / 32) words; at most max(P, 32)^2 / 8 bytes) and the scoring body's three regions of P ints afterwards -- R is dead once the
// labels are written, and the body initialises its regions itself -- then P 16-bit words of labels (lab16), which nothing overlays.  P =
// the power of two >= the largest frame: 130 KiB at 1024 detections, 448 B at 32.
// Launches: eval_sweep_prepare_kernel with no edge blocks (the lgamma tables) and this kernel.  No plan, no CSR, no reverse-edge table.
#include "strong_closure.cuh"

namespace gnncca {

constexpr int kSweepStrongMaxNodes = GNNCCA_STRONG_MAX_FRAME_NODES;

// "is edge k predicted" of this sweep: active, nothing else
struct SweepStrongPred : JointActive {
    __device__ __forceinline__ long long operator()(long long k) const { return active(k) ? 1 : 0; }
};

// bytes of the region R shares with the scoring body, for LDS capacity P (a power of two)
__host__ __device__ __forceinline__ size_t sweep_strong_shared_bytes(int P) {
    const size_t pr = P < 32 ? 32 : P;
    const size_t r = pr * (pr / 32) * 4, body = (size_t)12 * P;
    return r > body ? r : body;
}

// Workgroup (g, t): frame g at points[t].  points: fp64 [T][K]; frame_div (nullable): fp64 [K][G]; labels_out (nullable): int32 [T][N_all].
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void eval_sweep_strong_kernel(const long long* __restrict__ ei, long long E, const float* __restrict__ elab,
                                                                  const JointScores sc, const double* __restrict__ points,
                                                                  const double* __restrict__ frame_div, int N_all,
                                                                  const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr,
                                                                  int P_lds, double* __restrict__ rows_out, int* __restrict__ labels_out,
                                                                  double* __restrict__ lf_ws) {
    extern __shared__ int s_dyn[];
    __shared__ int s_round[kStrongMaxRounds];   // [r]: round r changed a word
    const int g = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int n_frames = gridDim.x;
    const SweepOut out = sweep_out(rows_out, labels_out, g, t, n_frames, N_all);
    SweepFrame f;
    if (!eval_sweep_frame<BLOCK>(g, N_all, E, node_ptr, edge_ptr, min(P_lds, kSweepStrongMaxNodes), out.row, out.lab_t, f)) return;
    SweepStrongPred pred;
    pred.set_point(sc, points, frame_div, t, g, n_frames);
    unsigned* R = reinterpret_cast<unsigned*>(s_dyn);
    unsigned short* lab16 = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(s_dyn) + sweep_strong_shared_bytes(P_lds));
    const int v0 = f.v0, n = f.n;
    const int W = (n + 31) >> 5;   // n_pad = 32 W <= max(P_lds, 32): the matrix fits the launch's LDS
    if (tid < kStrongMaxRounds) s_round[tid] = 0;
    strong_diagonal<BLOCK>(R, n, W);
    __syncthreads();
    for (long long k = f.k0 + tid; k < f.k1; k += BLOCK) {   // the frame's edge range, read once
        if (!pred.active(k)) continue;
        const long long a = ei[k] - v0, b = ei[E + k] - v0;
        if (a < 0 || a >= n || b < 0 || b >= n) continue;   // an edge that leaves its frame: no bit (strong_cluster_kernel, eval_frame_body)
        atomicOr(&R[(int)a * W + ((int)b >> 5)], 1u << ((int)b & 31));
    }
    __syncthreads();
    strong_close<BLOCK>(R, n, W, s_round);
    for (int v = tid; v < n; v += BLOCK) {   // (the block is narrower than the frame)
        const int r = strong_root(R, W, v);
        lab16[v] = (unsigned short)r;
        if (out.lab_t) out.lab_t[v0 + v] = v0 + r;
    }
    __syncthreads();   // R is dead: the body takes its bytes
    eval_frame_body<BLOCK, false, false>(g, out.row, ei, E, elab, pred, SweepLabel{lab16}, N_all, node_ptr, edge_ptr, P_lds, nullptr, lf_ws,
                                         nullptr, nullptr);
}

}  // namespace gnncca
