// loss.hip -- the training loss of the reference and the statistics it logs, on gfx950: `compute_loss_acc` (train.py:51-208) and the
// per-step, per-class mean probabilities of train.py:460-469, for the criteria of main_training.py:258-268 (BCE, BCE with pos_weight,
// utils.FocalLoss_binary).  Inputs: logits [S][E] fp32 (step-major, the [S, E, 1] buffer the MPN training forward returns), labels [E]
// fp32 (0 / 1, as gnncca_build_edges writes edge_labels).
//
// Forward, two launches:
//   1. edge_loss_partials_kernel: grid (nb, ceil(S / 8)); a thread reads the label of an edge once and the logits of up to 8 steps
//      (4 when S <= 4; coalesced per step; above 8 steps each group of 8 re-reads the labels), computes the per-edge terms in fp32 (torch's stable BCE-with-logits form) and accumulates them in fp64
//      registers.  Per workgroup: butterfly per wave, then the waves in order -> 44 partials per step chunk.
//   2. edge_loss_finish_kernel: one workgroup sums the partials of every quantity over the workgroups in index order (lane-strided, then
//      a butterfly), forms the record (GNNCCA_LOSS_REC_*) and, when a history is given, appends it at the device cursor.
// Backward, one launch: grad[s][e] = g * c_s * t(x, y) / E, the label read once for all steps.
// Deterministic: nb is a function of E alone, every sum has a fixed order, no float atomics.  Capturable: no host synchronisation, no
// allocation, nothing read back.  Compiled without fp contraction: the precisions are the reference's numpy expressions bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hip_try.h"

#pragma clang fp contract(off)

namespace gnncca {

constexpr int kLossBlock = 256;
constexpr int kChunk = 8;                 // steps per workgroup row: the accumulators of 8 steps live in registers
constexpr int kVals = 5 * kChunk + 4;     // per chunk: 5 sums per step, then n_pos, n_neg, hits1, hits0
constexpr int kMaxBlocks = 512;
constexpr int kItems = 4;                 // edges in flight per thread and loop trip
enum { V_L = 0, V_N1 = kChunk, V_N0 = 2 * kChunk, V_P1 = 3 * kChunk, V_P0 = 4 * kChunk, V_NPOS = 5 * kChunk, V_NNEG, V_HIT1, V_HIT0 };

__host__ __device__ inline int loss_blocks(long long E) {
    const long long per = (long long)kLossBlock * kItems;
    const long long b = (E + per - 1) / per;
    return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);   // every lane ends with the same bits (a + b == b + a)
    return v;
}

// torch's binary_cross_entropy_with_logits per element: (1 - y) x - w log_sigmoid(x), w = 1 + (pw - 1) y (1 without pos_weight)
__device__ __forceinline__ float bce_term(float x, float y, float w) {
    const float log_sig = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
    return (1.f - y) * x - w * log_sig;
}

// CH: steps held in registers (4 when S <= 4: half the accumulators, twice the waves per SIMD); the partials keep the kChunk layout
template <int CH>
__global__ __launch_bounds__(kLossBlock) void edge_loss_partials_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                                       long long E, int S, int weighted, int focal, float pw, float gamma,
                                                                       float alpha, double* __restrict__ part) {
    __shared__ double s_red[kLossBlock / 64][kVals];
    const int chunk = blockIdx.y;
    const int s0 = chunk * kChunk;
    const int ns = S - s0 < CH ? S - s0 : CH;
    const int last = S - 1 - s0;   // local index of the last step (precision), or outside [0, ns)
    const int nb = gridDim.x;
    double acc[5][CH];
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int j = 0; j < CH; ++j) acc[q][j] = 0.0;
    long long npos = 0, nneg = 0, hit1 = 0, hit0 = 0;
    const long long stride = (long long)nb * kLossBlock;
    for (long long base = (long long)blockIdx.x * kLossBlock + threadIdx.x; base < E; base += kItems * stride) {
        float y[kItems], x[kItems][CH];
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const long long e = base + k * stride;
            y[k] = e < E ? labels[e] : -1.f;
#pragma unroll
            for (int j = 0; j < CH; ++j) x[k][j] = (e < E && j < ns) ? logits[(long long)(s0 + j) * E + e] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            if (base + k * stride >= E) continue;
            const float yk = y[k];
            const bool pos = yk == 1.f, neg = yk == 0.f;
            npos += pos;
            nneg += neg;
            const float w = weighted ? 1.f + (pw - 1.f) * yk : 1.f;
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                if (j >= ns) continue;
                const float xv = x[k][j];
                const float l = bce_term(xv, yk, w);                           // the 'mean' criterion's term (and 'none' of BCE)
                const float ln = focal ? alpha * (powf(1.f - expf(-l), gamma) * l) : l;   // FocalLoss_binary(reduction='none')
                const float p = 1.f / (1.f + expf(-xv));                       // torch.nn.Sigmoid, as postprocess.cuh
                acc[0][j] += (double)l;
                if (pos) {
                    acc[1][j] += (double)ln;
                    acc[3][j] += (double)p;
                }
                if (neg) {
                    acc[2][j] += (double)ln;
                    acc[4][j] += (double)p;
                }
                if (j == last) {
                    hit1 += pos && p >= 0.5f;
                    hit0 += neg && !(p >= 0.5f);
                }
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
            const double v = j < CH ? wave_sum(acc[q][j < CH ? j : 0]) : 0.0;
            if (lane == 0) s_red[wave][q * kChunk + j] = v;
        }
    const double cnt[4] = {(double)npos, (double)nneg, (double)hit1, (double)hit0};   // integers below 2^53: exact in any order
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double v = wave_sum(cnt[q]);
        if (lane == 0) s_red[wave][V_NPOS + q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kVals) {
        double v = s_red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kLossBlock / 64; ++w) v += s_red[w][threadIdx.x];
        part[((long long)chunk * kVals + threadIdx.x) * nb + blockIdx.x] = v;
    }
}

// one workgroup: totals over the nb partials of every value, the record, the optional history row
__global__ __launch_bounds__(kLossBlock) void edge_loss_finish_kernel(const double* __restrict__ part, int nb, long long E, int S, int focal,
                                                                     double gamma, double alpha, float* __restrict__ loss_out,
                                                                     double* __restrict__ record, double* __restrict__ history,
                                                                     long long capacity, long long* __restrict__ cursor) {
    __shared__ double s_tot[(GNNCCA_LOSS_MAX_STEPS / kChunk) * kVals];
    __shared__ double s_rec[GNNCCA_LOSS_REC_LEN(GNNCCA_LOSS_MAX_STEPS)];
    __shared__ long long s_row;
    const int nchunks = (S + kChunk - 1) / kChunk;
    const int V = nchunks * kVals;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int v = wave; v < V; v += kLossBlock / 64) {
        double t = 0.0;
        for (int b = lane; b < nb; b += 64) t += part[(long long)v * nb + b];
        t = wave_sum(t);
        if (lane == 0) s_tot[v] = t;
    }
    __syncthreads();
    const int R = GNNCCA_LOSS_REC_LEN(S);
    if (threadIdx.x == 0) {
        const double dE = (double)E;
        const double npos = s_tot[V_NPOS], nneg = s_tot[V_NNEG];
        const int cl = (S - 1) / kChunk;
        const double hit1 = s_tot[cl * kVals + V_HIT1], hit0 = s_tot[cl * kVals + V_HIT0];
        double loss = 0.0, l1 = 0.0, l0 = 0.0;
        for (int s = 0; s < S; ++s) {
            const int b = (s / kChunk) * kVals, j = s % kChunk;
            const double m = s_tot[b + V_L + j] / dE;   // the criterion's 'mean' BCE of step s (NaN when E = 0)
            double term = m, coef = 1.0;
            if (focal) {   // FocalLoss_binary(reduction='mean'): alpha (1 - e^-m)^gamma m, applied to the MEAN BCE
                const double pt = exp(-m), a = 1.0 - pt, ag = pow(a, gamma);
                term = alpha * (ag * m);
                coef = alpha * (ag + ((gamma != 0.0 && a > 0.0) ? gamma * pow(a, gamma - 1.0) * pt * m : 0.0));
            }
            loss += term;
            l1 += s_tot[b + V_N1 + j] / npos;   // torch.mean over an empty class: NaN
            l0 += s_tot[b + V_N0 + j] / nneg;
            s_rec[GNNCCA_LOSS_REC_MEAN_PROB + 2 * s] = nneg > 0.0 ? s_tot[b + V_P0 + j] / nneg : 0.5;
            s_rec[GNNCCA_LOSS_REC_MEAN_PROB + 2 * s + 1] = npos > 0.0 ? s_tot[b + V_P1 + j] / npos : 0.5;
            s_rec[GNNCCA_LOSS_REC_MEAN_PROB + 2 * S + s] = coef;
        }
        // train.py:106-133: (hits / count) * 100.0 in float64, 0 when there is no hit
        const double hits = hit1 + hit0;
        s_rec[GNNCCA_LOSS_REC_LOSS] = loss;
        s_rec[GNNCCA_LOSS_REC_LOSS1] = l1;
        s_rec[GNNCCA_LOSS_REC_LOSS0] = l0;
        s_rec[GNNCCA_LOSS_REC_PREC1] = hit1 == 0.0 ? 0.0 : (hit1 / npos) * 100.0;
        s_rec[GNNCCA_LOSS_REC_PREC0] = hit0 == 0.0 ? 0.0 : (hit0 / nneg) * 100.0;
        s_rec[GNNCCA_LOSS_REC_PREC] = hits == 0.0 ? 0.0 : (hits / dE) * 100.0;
        s_rec[GNNCCA_LOSS_REC_NPOS] = npos;
        s_rec[GNNCCA_LOSS_REC_NNEG] = nneg;
        loss_out[0] = (float)loss;
        long long row = -1;
        if (history) {
            const long long c = cursor[0];
            if (c >= 0 && c < capacity) {
                row = c;
                cursor[0] = c + 1;
            } else {
                cursor[1] = 1;   // overflow: the row is dropped, nothing is written out of bounds
            }
        }
        s_row = row;
    }
    __syncthreads();
    const long long row = s_row;
    for (int q = threadIdx.x; q < R; q += kLossBlock) {
        record[q] = s_rec[q];
        if (row >= 0) history[row * R + q] = s_rec[q];
    }
}

__global__ __launch_bounds__(kLossBlock) void edge_loss_backward_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                                       long long E, int S, int weighted, float pw,
                                                                       const float* __restrict__ grad_loss, const double* __restrict__ record,
                                                                       float* __restrict__ grad) {
    const double g = (double)grad_loss[0];
    const double dE = (double)E;
    const double* coef = record + GNNCCA_LOSS_REC_MEAN_PROB + 2 * S;
    for (long long e = (long long)blockIdx.x * kLossBlock + threadIdx.x; e < E; e += (long long)gridDim.x * kLossBlock) {
        const float y = labels[e];
        const float w = 1.f + (pw - 1.f) * y;
        for (int s = 0; s < S; ++s) {
            const float x = logits[(long long)s * E + e];
            // d/dx of the BCE-with-logits term: (1 - y) - w sigma(-x) with pos_weight, sigma(x) - y without
            const float t = weighted ? (1.f - y) - w * (1.f / (1.f + expf(x))) : 1.f / (1.f + expf(-x)) - y;
            grad[(long long)s * E + e] = (float)(g * coef[s] / dE) * t;
        }
    }
}

}  // namespace gnncca

using namespace gnncca;

extern "C" {

size_t gnncca_edge_loss_workspace_bytes(int32_t n_steps, int64_t n_edges) {
    if (n_steps < 1 || n_steps > GNNCCA_LOSS_MAX_STEPS || n_edges < 0) return 0;
    const size_t nchunks = (size_t)((n_steps + kChunk - 1) / kChunk);
    const size_t bytes = nchunks * kVals * (size_t)(n_edges > 0 ? loss_blocks(n_edges) : 0) * sizeof(double);
    return bytes < 256 ? 256 : (bytes + 255) / 256 * 256;
}

static int edge_loss_check(const float* logits, const float* labels, int32_t n_steps, int64_t n_edges, int32_t criterion, float pos_weight) {
    if (n_steps < 1 || n_edges < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n_steps > GNNCCA_LOSS_MAX_STEPS) return GNNCCA_ERR_UNSUPPORTED;
    if (criterion != GNNCCA_LOSS_BCE && criterion != GNNCCA_LOSS_BCE_WEIGHTED && criterion != GNNCCA_LOSS_FOCAL) return GNNCCA_ERR_INVALID_ARG;
    if (criterion == GNNCCA_LOSS_BCE_WEIGHTED && !(pos_weight > 0.f && pos_weight <= 3.0e38f)) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!logits || !labels)) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > (int64_t)1 << 40) return GNNCCA_ERR_UNSUPPORTED;
    return GNNCCA_OK;
}

int gnncca_edge_loss_forward(const float* logits, const float* labels, int32_t n_steps, int64_t n_edges, int32_t criterion, int32_t validate,
                             float pos_weight, float focusing_param, float balance_param, float* loss_out, double* record,
                             double* history, int64_t capacity, int64_t* cursor, void* workspace, size_t workspace_bytes,
                             gnncca_stream_t stream) {
    const int st0 = edge_loss_check(logits, labels, n_steps, n_edges, criterion, pos_weight);
    if (st0 != GNNCCA_OK) return st0;
    if (!loss_out || !record || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (criterion == GNNCCA_LOSS_FOCAL && !(std::isfinite(focusing_param) && focusing_param >= 0.f && std::isfinite(balance_param)))
        return GNNCCA_ERR_INVALID_ARG;
    if (history && (!cursor || capacity < 0)) return GNNCCA_ERR_INVALID_ARG;
    if (workspace_bytes < gnncca_edge_loss_workspace_bytes(n_steps, n_edges)) return GNNCCA_ERR_WORKSPACE;
    // validate: plain BCE with logits whatever the configured criterion (train.py:90-95)
    const int weighted = !validate && criterion == GNNCCA_LOSS_BCE_WEIGHTED;
    const int focal = !validate && criterion == GNNCCA_LOSS_FOCAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    const int nb = n_edges > 0 ? loss_blocks(n_edges) : 0;
    const int nchunks = (n_steps + kChunk - 1) / kChunk;
    if (nb > 0) {
        const float pw = weighted ? pos_weight : 1.f;
        if (n_steps <= 4)
            hipLaunchKernelGGL(edge_loss_partials_kernel<4>, dim3((unsigned)nb, 1), dim3(kLossBlock), 0, st, logits, labels,
                               (long long)n_edges, (int)n_steps, weighted, focal, pw, focusing_param, balance_param, part);
        else
            hipLaunchKernelGGL(edge_loss_partials_kernel<kChunk>, dim3((unsigned)nb, (unsigned)nchunks), dim3(kLossBlock), 0, st, logits,
                               labels, (long long)n_edges, (int)n_steps, weighted, focal, pw, focusing_param, balance_param, part);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(edge_loss_finish_kernel, dim3(1), dim3(kLossBlock), 0, st, part, nb, (long long)n_edges, (int)n_steps, focal,
                       (double)focusing_param, (double)balance_param, loss_out, record, history, (long long)capacity,
                       reinterpret_cast<long long*>(cursor));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_edge_loss_backward(const float* logits, const float* labels, int32_t n_steps, int64_t n_edges, int32_t criterion, int32_t validate,
                              float pos_weight, const float* grad_loss, const double* record, float* grad, gnncca_stream_t stream) {
    const int st0 = edge_loss_check(logits, labels, n_steps, n_edges, criterion, pos_weight);
    if (st0 != GNNCCA_OK) return st0;
    if (!grad_loss || !record || (n_edges > 0 && !grad)) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges == 0) return GNNCCA_OK;
    const int weighted = !validate && criterion == GNNCCA_LOSS_BCE_WEIGHTED;
    const long long want = (n_edges + kLossBlock - 1) / kLossBlock;
    const unsigned blocks = (unsigned)(want < 16384 ? want : 16384);
    hipLaunchKernelGGL(edge_loss_backward_kernel, dim3(blocks), dim3(kLossBlock), 0, static_cast<hipStream_t>(stream), logits, labels,
                       (long long)n_edges, (int)n_steps, weighted, weighted ? pos_weight : 1.f, grad_loss, record, grad);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
