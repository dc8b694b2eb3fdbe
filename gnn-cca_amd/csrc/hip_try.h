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
