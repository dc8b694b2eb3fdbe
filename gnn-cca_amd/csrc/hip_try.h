#pragma once
// The error macro of every HIP translation unit of the library: a failed HIP call records its hipError_t in the thread's error
// word (pack.cpp defines it; gnncca_last_hip_error reads it) and returns GNNCCA_ERR_HIP from the enclosing function.
#include <hip/hip_runtime.h>

#include "internal.h"

#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) {                            \
            ::gnncca::g_last_hip_error = (int)_e;          \
            return GNNCCA_ERR_HIP;                         \
        }                                                  \
    } while (0)

// Above 64 KiB of dynamic LDS a kernel needs hipFuncAttributeMaxDynamicSharedMemorySize before its launch.  lds_opt_in<kernel>(max_bytes)
// sets it to the largest size the caller ever launches with, at most once per (kernel, host thread, device), and hands the hipError_t to
// the caller's HIP_TRY:   if (lds > 64 * 1024) HIP_TRY(lds_opt_in<some_kernel<256>>(max_bytes));
namespace gnncca {
template <auto Kernel>
inline hipError_t lds_opt_in(size_t max_bytes) {
    static thread_local int attr_dev = -1;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && attr_dev != dev) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes);
        if (e == hipSuccess) attr_dev = dev;
    }
    return e;
}
}  // namespace gnncca
