#pragma once
// Included by mpn_forward.hip ONLY, ahead of its kernel headers: the diagnostic stamps of the encoder / step kernels and the per-kernel
// profiler of gnncca_mpn_forward_profiled.  `g_stamps` is a __device__ global, i.e. one copy per translation unit (the library is built
// without relocatable device code), and gnncca_debug_set_stamps sets the copy of mpn_forward.hip: a kernel of another unit cannot stamp,
// and since the macros live here it does not compile if it tries.
#include "common.cuh"

namespace gnncca {

// Diagnostic build only (-DGNNCCA_STAMPS, tools/stamps.py): s_memtime stamps of every wave at named points, written to
// a buffer of their own that no kernel reads.  The product build compiles these to nothing.
#ifdef GNNCCA_STAMPS
__device__ unsigned long long* g_stamps = nullptr;
#define GNNCCA_STAMP(kslot, id)                                                                              \
    do {                                                                                                     \
        if (g_stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 4096) {                                      \
            g_stamps[((((size_t)(kslot)) * 4096 + blockIdx.x) * 4 + (threadIdx.x >> 6)) * 16 + (id)] =       \
                __builtin_amdgcn_s_memtime();                                                                \
        }                                                                                                    \
    } while (0)
#else
#define GNNCCA_STAMP(kslot, id) \
    do {                        \
    } while (0)
#endif

// Diagnostic build only: per-wave TOTALS of the cycles spent in up to 8 phases of a loop (s_memtime deltas accumulated in registers,
// written once at the end: g_stamps[slot][block < 4096][wave & 3][0..7]).  Nothing in the product build.
#ifdef GNNCCA_STAMPS
#define PHASE_T_DECL unsigned long long pt_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt_last = __builtin_amdgcn_s_memtime(), pt_real0 = __builtin_amdgcn_s_memrealtime()
#define PHASE_T(i)                                                      \
    do {                                                                \
        const unsigned long long pt_now = __builtin_amdgcn_s_memtime(); \
        pt_acc[i] += pt_now - pt_last;                                  \
        pt_last = pt_now;                                               \
    } while (0)
#define PHASE_T_FLUSH(slot)                                                                                                   \
    do {                                                                                                                      \
 pt_acc[7] = __builtin_amdgcn_s_memrealtime() - pt_real0; /* 100 MHz */                                              \
        if (g_stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 2048 && (threadIdx.x >> 6) < 8)   /* waves 4-7: block + 2048 */  \
            for (int q = 0; q < 8; ++q)                                                                                       \
                g_stamps[((((size_t)(slot)) * 4096 + blockIdx.x + 2048 * (threadIdx.x >> 8)) * 4 + ((threadIdx.x >> 6) & 3)) * 16 + q] = pt_acc[q]; \
    } while (0)
#else
#define PHASE_T_DECL do { } while (0)
#define PHASE_T(i) do { } while (0)
#define PHASE_T_FLUSH(slot) do { } while (0)
#endif

// Per-kernel timing for bench.py / rocprof cross-checks (diagnostic entry point only).  The events are ATTACHED TO
// THE DISPATCH (hipExtLaunchKernelGGL start / stop events), so a slot's elapsed time is the kernel's own execution
// time, the quantity rocprofv3 --kernel-trace reports -- not launch-to-launch time with the cost of an event packet
// in it (which is 2-3 us, more than half of a 5 us launch).
struct Profiler {
    gnncca_profile* out;
    hipEvent_t start[GNNCCA_PROFILE_MAX], stop[GNNCCA_PROFILE_MAX];
    int n;
};
static thread_local Profiler* t_prof = nullptr;  // non-null only inside gnncca_mpn_forward_profiled

static int prof_begin(Profiler* p) {
    p->n = 0;
    for (int i = 0; i < GNNCCA_PROFILE_MAX; ++i) {
        HIP_TRY(hipEventCreate(&p->start[i]));
        HIP_TRY(hipEventCreate(&p->stop[i]));
    }
    t_prof = p;
    return GNNCCA_OK;
}

// the launch that precedes this call used slot n (GNNCCA_LAUNCH): name it and move on
static int prof_mark(Profiler* p, int kind) {
    if (!p || p->n >= GNNCCA_PROFILE_MAX) return GNNCCA_OK;
    p->out->kind[p->n] = kind;
    p->n++;
    return GNNCCA_OK;
}

static int prof_end(Profiler* p, hipStream_t st) {
    t_prof = nullptr;
    HIP_TRY(hipStreamSynchronize(st));
    p->out->count = p->n;
    for (int i = 0; i < p->n; ++i) HIP_TRY(hipEventElapsedTime(&p->out->ms[i], p->start[i], p->stop[i]));
    for (int i = 0; i < GNNCCA_PROFILE_MAX; ++i) {
        HIP_TRY(hipEventDestroy(p->start[i]));
        HIP_TRY(hipEventDestroy(p->stop[i]));
    }
    return GNNCCA_OK;
}

#define PROF_MARK(kind)                                  \
    do {                                                 \
        int _s = prof_mark(prof, (kind));                \
        if (_s != GNNCCA_OK) return _s;                  \
    } while (0)

// Kernel launch of the forward path: plain, or with the profiler's events attached to this very dispatch.
#define GNNCCA_LAUNCH(kernel, grid, block, lds, st, ...)                                                              \
    do {                                                                                                              \
        if (t_prof != nullptr && t_prof->n < GNNCCA_PROFILE_MAX)                                                      \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, st, t_prof->start[t_prof->n], t_prof->stop[t_prof->n], 0, \
                                  __VA_ARGS__);                                                                       \
        else                                                                                                          \
            hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);                                            \
    } while (0)

}  // namespace gnncca
