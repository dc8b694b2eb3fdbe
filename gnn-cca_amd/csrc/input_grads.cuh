#pragma once
// SURVEY.md 8f row N3, input gradients: d loss / d x and d loss / d edge_attr of a train-mode forward (the reference's
// module backpropagates to its inputs, models/mpn.py:266-297; fine-tuning a ReID head through the association loss asks for it).
// Both are products of a gradient the backward already holds with the first encoder layer's weight, so they are overwritten,
// never accumulated: no atomics, and each is a deterministic function of that gradient.
// Part of the translation unit mpn_train.hip.

namespace gnncca {

// dx[n][k] = sum_o G[n][o] * W[o][k]      G = d loss / d (first node-encoder layer's pre-activation) [N][O], W [O][K] row-major
// (nn.Linear's layout), dx [N][K].  The largest product of the backward and the only one that writes N x K floats.
// Arithmetic: v_mfma_f32_32x32x2_f32, exact fp32 -- bit for bit an fmaf chain over o in ascending order, so the result
// does not depend on the launch shape.  (The forward's split-bf16 form would need W re-split per training step, and this pipe
// is not what bounds the kernel at the sizes training sees: the N x K x 4-byte write and the launch are.)
// A workgroup owns one 32-row tile of G, staged once in LDS in chunks of 128 columns (row stride 129 words: the 32 rows a
// wave reads land in 32 different banks), and 128 output columns; each of its four waves owns one 32 x 32 output tile and
// streams its 32 columns of W from global memory (L2-resident: W is O x K x 4 bytes) in the operand layout -- lane
// (l % 32, l / 32) holds G[n0 + l % 32][o + l / 32] and W[o + l / 32][k0 + l % 32] -- eight MFMA k-steps of loads in flight.
// Any N, O, K >= 1; nothing is assumed about alignment beyond 4 bytes (scalar loads and stores, 128 B per half-wave).
constexpr int kDxChunk = 128, kDxLd = kDxChunk + 1;

__global__ __launch_bounds__(256) void bwd_dx_mfma_kernel(const float* __restrict__ G, const float* __restrict__ W,
                                                          float* __restrict__ dx, int N, int O, int K) {
    __shared__ float s_g[32 * kDxLd];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
    const long long n0 = (long long)blockIdx.x * 32;
    const int k = (blockIdx.y * 4 + wave) * 32 + l32;
    const bool k_ok = k < K;   // a wave past the last column tile still takes part in the staging and the barriers
    const float* __restrict__ pw = W + (k_ok ? k : 0);
    const float* pa = s_g + l32 * kDxLd + half;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int oc = 0; oc < O; oc += kDxChunk) {
        const int ow = min(kDxChunk, O - oc), ow16 = (ow + 15) & ~15;   // staged width, zero-filled up to whole rounds of 16
        if (oc > 0) __syncthreads();
        for (int t = threadIdx.x; t < 32 * ow16; t += 256) {
            const int r = t / ow16, o = t - r * ow16;
            const long long n = n0 + r;
            s_g[r * kDxLd + o] = (n < N && o < ow) ? G[(size_t)n * O + oc + o] : 0.f;
        }
        __syncthreads();
        for (int o = 0; o < ow16; o += 16) {
            float b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int oo = oc + o + 2 * u + half;
                const bool ok = oo < O;
                const float v = pw[(size_t)(ok ? oo : 0) * K];
                b[u] = ok && k_ok ? v : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[o + 2 * u], b[u], acc, 0, 0, 0);
        }
    }
    // D layout: lane (j = l % 32) holds column j, register r row (r % 4) + 8 * (r / 4) + 4 * (l / 32)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long n = n0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (k_ok && n < N) dx[(size_t)n * K + k] = acc[r];
    }
}

static hipError_t launch_dx(const float* G, const float* W, float* dx, long long N, int O, int K, hipStream_t st) {
    if (N <= 0 || O <= 0 || K <= 0) return hipSuccess;
    const dim3 grid((unsigned)((N + 31) / 32), (unsigned)((K + 127) / 128));
    hipLaunchKernelGGL(bwd_dx_mfma_kernel, grid, dim3(256), 0, st, G, W, dx, (int)N, O, K);
    return hipGetLastError();
}

// d attr[k][a] = sum_f (e0[k][f] > 0 ? ge0[k][f] * scale : 0) * W[f][a]      (edge encoder of the MFMA family: one layer, W [6][A])
// The mask and the Dropout scale are the ones bwd_edge_enc_kernel applies inline (e0 is the saved, post-Dropout output).
// One thread per output element: neighbouring threads read the same 48 B of their edge and write consecutive words.
__global__ __launch_bounds__(256) void bwd_edge_attr_kernel(const float* __restrict__ ge0, const float* __restrict__ e0,
                                                            const float* __restrict__ W, float* __restrict__ dattr, int A,
                                                            long long E, float scale) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= E * A) return;
    const long long k = t / A;
    const int a = (int)(t - k * A);
    float acc = 0.f;
#pragma unroll
    for (int f = 0; f < kEF; ++f) {
        const float g = e0[k * kEF + f] > 0.f ? ge0[k * kEF + f] * scale : 0.f;
        acc = fmaf(g, W[f * A + a], acc);
    }
    dattr[t] = acc;
}

}  // namespace gnncca
