// optim.hip -- the optimizer step of the reference's training loop (`optimizer.step()`, train.py:492-494) on gfx950, for the two
// optimizers main_training.py:220-256, 349-370 builds: torch.optim.SGD and torch.optim.Adam.  One launch updates every tensor of a
// parameter group (up to kOptimMaxTensors per launch; a larger group takes several).  Every hyperparameter and every step count is READ
// FROM DEVICE MEMORY by the kernel (the "block", GNNCCA_OPTIM_BLOCK_*): a HIP graph that captured the launch follows a learning-rate
// schedule written into the block between replays.  Tensor addresses travel BY VALUE in the launch arguments: each captured graph keeps
// the gradient addresses it was captured with.
//
// Operation order, per element, fp32, one correctly rounded operation per line, NO contraction (the pragma below).  The hyperparameters
// are stored as fp64 and rounded to fp32 once per thread: lr, wd, mom = (float)double; omd = (float)(1.0 - dampening) (fp64 subtraction).
//   SGD (p parameter, g gradient, b momentum buffer, `first` = this tensor's step count is 0):
//     if wd != 0:   t1 = wd * p;   g = g + t1
//     if mom != 0:  if first:  b = g
//                   else:      t2 = mom * b;   t3 = omd * g;   b = t2 + t3
//                   if nesterov:  t4 = mom * b;   g = g + t4      else:  g = b
//     t5 = lr * g;   p = p - t5
//   Adam (m exp_avg, v exp_avg_sq, vm max_exp_avg_sq; t = step count + 1; on t == 1 the state is taken as zero, not read):
//     fp64, once per thread: bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, ss = (float)(lr / bc1), rs = (float)sqrt(bc2),
//                            b1 = (float)beta1, c1 = (float)(1 - beta1), b2 = (float)beta2, c2 = (float)(1 - beta2), e = (float)eps
//     if wd != 0:   g = fma(wd, p, g)
//     m = fma(b1, m, c1 * g);   v = fma(b2, v, c2 * (g * g));   if amsgrad:  vm = max(vm, v), u = vm   else u = v
//     d = sqrt(u) / rs + e;   p = p - ss * (m / d)                  (explicit fma only: it saves a rounding, the compiler adds none)
//
// Step counts: int32 per tensor slot in the block.  Every workgroup reads the counts of its tensor first; after its elements are
// written the workgroup draws a ticket (one relaxed agent-scope atomic add), and the workgroup that draws the LAST ticket of the launch
// -- hence after every other workgroup has read -- advances the counts of the launch's tensors and clears the ticket word.  No
// workgroup can see a count advanced by its own launch; a replay needs no host code.  Elementwise otherwise: no float atomics, no
// reductions, results do not depend on the grid.  Capturable: no allocation, no synchronisation, nothing read back.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hip_try.h"

#pragma clang fp contract(off)

namespace gnncca {

constexpr int kOptimBlock = 256;
constexpr int kOptimChunk = 4 * kOptimBlock;   // elements per workgroup: one float4 per thread
constexpr int kOptimMaxTensors = GNNCCA_OPTIM_MAX_TENSORS_PER_LAUNCH;

struct OptimHeader {       // GNNCCA_OPTIM_BLOCK_*: the layout include/gnncca_mpn.h documents
    double h[8];           // lr, weight_decay, a, b, c, flag, rule, (unused)
    unsigned int ticket;
    unsigned int pad[3];
};
static_assert(sizeof(OptimHeader) == GNNCCA_OPTIM_BLOCK_STEPS_OFFSET, "block layout");
static_assert(offsetof(OptimHeader, ticket) == GNNCCA_OPTIM_BLOCK_TICKET_OFFSET, "block layout");

struct OptimTensor {
    float* p;
    const float* g;
    float* s0;             // SGD momentum_buffer / Adam exp_avg          (null: the tensor has none)
    float* s1;             // Adam exp_avg_sq
    float* s2;             // Adam max_exp_avg_sq                         (null without amsgrad)
    unsigned int n;        // elements
    int slot;              // index of the tensor's step count in the block
};

struct OptimArgs {         // by value: 64 * 48 + 64 * 4 + 8 bytes of kernel arguments
    OptimTensor t[kOptimMaxTensors];
    unsigned int first[kOptimMaxTensors];   // first workgroup of tensor i; 0xffffffff behind the last tensor
    int n_tensors;
    int pad;
};

__global__ void optim_set_hyper_kernel(OptimHeader* __restrict__ blk, double lr, double wd, double a, double b, double c, double flag,
                                       double rule) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        blk->h[0] = lr;
        blk->h[1] = wd;
        blk->h[2] = a;
        blk->h[3] = b;
        blk->h[4] = c;
        blk->h[5] = flag;
        blk->h[6] = rule;
    }
}

struct SgdRule {
    float lr, wd, mom, omd;
    bool nesterov, first;
    __device__ __forceinline__ void load(const OptimHeader* blk, int count) {
        lr = (float)blk->h[0];
        wd = (float)blk->h[1];
        mom = (float)blk->h[2];
        omd = (float)(1.0 - blk->h[3]);
        nesterov = blk->h[5] != 0.0;
        first = count == 0;
    }
    // one element; b: the momentum buffer's value (ignored when !has_b or first)
    __device__ __forceinline__ void apply(float& p, float g, float& b, bool has_b) const {
        if (wd != 0.f) {
            const float t1 = wd * p;
            g = g + t1;
        }
        if (mom != 0.f && has_b) {
            if (first) {
                b = g;
            } else {
                const float t2 = mom * b;
                const float t3 = omd * g;
                b = t2 + t3;
            }
            if (nesterov) {
                const float t4 = mom * b;
                g = g + t4;
            } else {
                g = b;
            }
        }
        const float t5 = lr * g;
        p = p - t5;
    }
};

struct AdamRule {
    float ss, rs, b1, c1, b2, c2, eps, wd;
    bool amsgrad, first;
    __device__ __forceinline__ void load(const OptimHeader* blk, int count) {
        const double t = (double)count + 1.0;
        const double beta1 = blk->h[2], beta2 = blk->h[3];
        const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
        ss = (float)(blk->h[0] / bc1);
        rs = (float)sqrt(bc2);
        b1 = (float)beta1;
        c1 = (float)(1.0 - beta1);
        b2 = (float)beta2;
        c2 = (float)(1.0 - beta2);
        eps = (float)blk->h[4];
        wd = (float)blk->h[1];
        amsgrad = blk->h[5] != 0.0;
        first = count == 0;
    }
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v, float& vm, bool has_vm) const {
        if (wd != 0.f) g = fmaf(wd, p, g);
        m = fmaf(b1, m, c1 * g);
        v = fmaf(b2, v, c2 * (g * g));
        float u = v;
        if (amsgrad && has_vm) {
            vm = fmaxf(vm, v);
            u = vm;
        }
        const float d = sqrtf(u) / rs + eps;
        p = p - ss * (m / d);
    }
};

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

template <int RULE>
__global__ __launch_bounds__(kOptimBlock) void optim_step_kernel(OptimHeader* __restrict__ blk, const OptimArgs a) {
    int* __restrict__ steps = reinterpret_cast<int*>(reinterpret_cast<char*>(blk) + GNNCCA_OPTIM_BLOCK_STEPS_OFFSET);
    // the tensor of this workgroup: the number of tensors that start at or before it (unused entries are 0xffffffff), all in SGPRs
    int ti = -1;
#pragma unroll
    for (int i = 0; i < kOptimMaxTensors; ++i) ti += a.first[i] <= blockIdx.x;
    const OptimTensor T = a.t[ti];
    const int count = steps[T.slot];
    const unsigned int base = (blockIdx.x - a.first[ti]) * (unsigned)kOptimChunk;
    const unsigned int n = T.n;
    const bool vec = aligned16(T.p) && aligned16(T.g) && aligned16(T.s0) && aligned16(T.s1) && aligned16(T.s2);
    const unsigned int i4 = base + 4u * threadIdx.x;

    if (RULE == GNNCCA_OPTIM_SGD) {
        SgdRule r;
        r.load(blk, count);
        const bool has_b = T.s0 != nullptr;
        const bool rd_b = has_b && !r.first && r.mom != 0.f, wr_b = has_b && r.mom != 0.f;
        if (vec && i4 + 4u <= n) {
            float4 p = *reinterpret_cast<const float4*>(T.p + i4);
            const float4 g = *reinterpret_cast<const float4*>(T.g + i4);
            float4 b = rd_b ? *reinterpret_cast<const float4*>(T.s0 + i4) : make_float4(0.f, 0.f, 0.f, 0.f);
            r.apply(p.x, g.x, b.x, has_b);
            r.apply(p.y, g.y, b.y, has_b);
            r.apply(p.z, g.z, b.z, has_b);
            r.apply(p.w, g.w, b.w, has_b);
            *reinterpret_cast<float4*>(T.p + i4) = p;
            if (wr_b) *reinterpret_cast<float4*>(T.s0 + i4) = b;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned int i = vec ? i4 + k : base + threadIdx.x + k * kOptimBlock;   // scalar tail / unaligned tensor
                if (i >= n || i >= base + kOptimChunk) continue;
                float p = T.p[i];
                float b = rd_b ? T.s0[i] : 0.f;
                r.apply(p, T.g[i], b, has_b);
                T.p[i] = p;
                if (wr_b) T.s0[i] = b;
            }
        }
    } else {
        AdamRule r;
        r.load(blk, count);
        const bool has_vm = T.s2 != nullptr;
        const bool wr_vm = has_vm && r.amsgrad, rd_vm = wr_vm && !r.first;
        if (T.s0 != nullptr && T.s1 != nullptr) {   // (checked by the host too: a tensor without moments is not stepped)
            if (vec && i4 + 4u <= n) {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                float4 p = *reinterpret_cast<const float4*>(T.p + i4);
                const float4 g = *reinterpret_cast<const float4*>(T.g + i4);
                float4 m = r.first ? z : *reinterpret_cast<const float4*>(T.s0 + i4);
                float4 v = r.first ? z : *reinterpret_cast<const float4*>(T.s1 + i4);
                float4 vm = rd_vm ? *reinterpret_cast<const float4*>(T.s2 + i4) : z;
                r.apply(p.x, g.x, m.x, v.x, vm.x, has_vm);
                r.apply(p.y, g.y, m.y, v.y, vm.y, has_vm);
                r.apply(p.z, g.z, m.z, v.z, vm.z, has_vm);
                r.apply(p.w, g.w, m.w, v.w, vm.w, has_vm);
                *reinterpret_cast<float4*>(T.p + i4) = p;
                *reinterpret_cast<float4*>(T.s0 + i4) = m;
                *reinterpret_cast<float4*>(T.s1 + i4) = v;
                if (wr_vm) *reinterpret_cast<float4*>(T.s2 + i4) = vm;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned int i = vec ? i4 + k : base + threadIdx.x + k * kOptimBlock;
                    if (i >= n || i >= base + kOptimChunk) continue;
                    float p = T.p[i];
                    float m = r.first ? 0.f : T.s0[i];
                    float v = r.first ? 0.f : T.s1[i];
                    float vm = rd_vm ? T.s2[i] : 0.f;
                    r.apply(p, T.g[i], m, v, vm, has_vm);
                    T.p[i] = p;
                    T.s0[i] = m;
                    T.s1[i] = v;
                    if (wr_vm) T.s2[i] = vm;
                }
            }
        }
    }

    // hand-over of the step counts: every thread's read of `steps` has returned before the barrier, the ticket is drawn after it
    __shared__ int s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int tk = __hip_atomic_fetch_add(&blk->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = tk == gridDim.x - 1;
    }
    __syncthreads();
    if (s_last) {
        if ((int)threadIdx.x < a.n_tensors) {
            const OptimTensor U = a.t[threadIdx.x];
            // SGD counts the steps a momentum buffer has seen (its first one copies the gradient); Adam counts every step
            if (RULE == GNNCCA_OPTIM_ADAM ? (U.s0 != nullptr && U.s1 != nullptr) : (U.s0 != nullptr && (float)blk->h[2] != 0.f)) {
                const int c = steps[U.slot];
                steps[U.slot] = c < 0x7fffffff ? c + 1 : c;
            }
        }
        if (threadIdx.x == 0) __hip_atomic_store(&blk->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

}  // namespace gnncca

using namespace gnncca;

extern "C" {

size_t gnncca_optim_block_bytes(int32_t n_slots) {
    if (n_slots < 0) return 0;
    const size_t bytes = GNNCCA_OPTIM_BLOCK_STEPS_OFFSET + sizeof(int32_t) * (size_t)n_slots;
    return (bytes + 255) / 256 * 256;
}

int gnncca_optim_set_hyper(void* block, int32_t rule, double lr, double weight_decay, double a, double b, double c, int32_t flag,
                           gnncca_stream_t stream) {
    if (!block) return GNNCCA_ERR_INVALID_ARG;
    if (rule != GNNCCA_OPTIM_SGD && rule != GNNCCA_OPTIM_ADAM) return GNNCCA_ERR_INVALID_ARG;
    // the ranges torch.optim.SGD / Adam accept in their constructors
    if (!finite_nonneg(lr) || !finite_nonneg(weight_decay)) return GNNCCA_ERR_INVALID_ARG;
    if (rule == GNNCCA_OPTIM_SGD) {
        if (!finite_nonneg(a) || !std::isfinite(b)) return GNNCCA_ERR_INVALID_ARG;          // momentum, dampening
        if (flag && (!(a > 0.0) || b != 0.0)) return GNNCCA_ERR_INVALID_ARG;                // Nesterov: momentum > 0, no dampening
    } else {
        if (!(a >= 0.0 && a < 1.0) || !(b >= 0.0 && b < 1.0) || !finite_nonneg(c)) return GNNCCA_ERR_INVALID_ARG;   // betas, eps
    }
    hipLaunchKernelGGL(optim_set_hyper_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<OptimHeader*>(block), lr,
                       weight_decay, a, b, c, flag ? 1.0 : 0.0, (double)rule);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

static int optim_step(void* block, int32_t rule, int32_t n_slots, int32_t n_tensors, void* const* params, const void* const* grads,
                      void* const* s0, void* const* s1, void* const* s2, const int64_t* numel, const int32_t* slots, hipStream_t st) {
    if (!block || n_slots < 0 || n_tensors < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n_tensors == 0) return GNNCCA_OK;
    if (!params || !grads || !numel || !slots) return GNNCCA_ERR_INVALID_ARG;
    if (rule == GNNCCA_OPTIM_ADAM && (!s0 || !s1)) return GNNCCA_ERR_INVALID_ARG;
    for (int i = 0; i < n_tensors; ++i) {   // everything is checked before the first launch
        if (numel[i] < 0 || slots[i] < 0 || slots[i] >= n_slots) return GNNCCA_ERR_INVALID_ARG;
        if (numel[i] > 0 && (!params[i] || !grads[i])) return GNNCCA_ERR_INVALID_ARG;
        if (numel[i] > 0 && rule == GNNCCA_OPTIM_ADAM && (!s0[i] || !s1[i])) return GNNCCA_ERR_INVALID_ARG;
        if (numel[i] > (int64_t)0x7fffffff) return GNNCCA_ERR_UNSUPPORTED;
        for (int j = 0; j < i; ++j)
            if (slots[j] == slots[i]) return GNNCCA_ERR_INVALID_ARG;   // one step count per tensor
    }
    int i = 0;
    while (i < n_tensors) {
        OptimArgs a;
        for (int k = 0; k < kOptimMaxTensors; ++k) {
            a.t[k] = OptimTensor{nullptr, nullptr, nullptr, nullptr, nullptr, 0u, 0};
            a.first[k] = 0xffffffffu;
        }
        a.pad = 0;
        unsigned int groups = 0;
        int k = 0;
        for (; i < n_tensors && k < kOptimMaxTensors; ++i) {
            if (numel[i] == 0) continue;
            const unsigned int need = (unsigned int)((numel[i] + kOptimChunk - 1) / kOptimChunk);
            if (groups + need > 0x7fff0000u) break;   // the grid limit: the rest goes to the next launch
            a.t[k] = OptimTensor{static_cast<float*>(params[i]), static_cast<const float*>(grads[i]), s0 ? static_cast<float*>(s0[i]) : nullptr,
                                 s1 ? static_cast<float*>(s1[i]) : nullptr, s2 ? static_cast<float*>(s2[i]) : nullptr,
                                 (unsigned int)numel[i], slots[i]};
            a.first[k] = groups;
            groups += need;
            ++k;
        }
        a.n_tensors = k;
        if (k == 0) continue;
        if (rule == GNNCCA_OPTIM_SGD)
            hipLaunchKernelGGL(optim_step_kernel<GNNCCA_OPTIM_SGD>, dim3(groups), dim3(kOptimBlock), 0, st, static_cast<OptimHeader*>(block), a);
        else
            hipLaunchKernelGGL(optim_step_kernel<GNNCCA_OPTIM_ADAM>, dim3(groups), dim3(kOptimBlock), 0, st, static_cast<OptimHeader*>(block), a);
        HIP_TRY(hipGetLastError());
    }
    return GNNCCA_OK;
}

int gnncca_optim_sgd_step(void* block, int32_t n_slots, int32_t n_tensors, void* const* params, const void* const* grads,
                          void* const* momentum_bufs, const int64_t* numel, const int32_t* slots, gnncca_stream_t stream) {
    return optim_step(block, GNNCCA_OPTIM_SGD, n_slots, n_tensors, params, grads, momentum_bufs, nullptr, nullptr, numel, slots,
                      static_cast<hipStream_t>(stream));
}

int gnncca_optim_adam_step(void* block, int32_t n_slots, int32_t n_tensors, void* const* params, const void* const* grads,
                           void* const* exp_avg, void* const* exp_avg_sq, void* const* max_exp_avg_sq, const int64_t* numel,
                           const int32_t* slots, gnncca_stream_t stream) {
    return optim_step(block, GNNCCA_OPTIM_ADAM, n_slots, n_tensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, slots,
                      static_cast<hipStream_t>(stream));
}

}  // extern "C"
