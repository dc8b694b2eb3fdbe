#pragma once
// Shared by every kernel file: vector typedefs, the error macro, launch helpers, train-mode Dropout.  Holds no non-inline definition, so any
// translation unit may include it (the stamps and the profiler of the forward live in forward_diag.cuh).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "hip_try.h"

namespace gnncca {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// One scalar load per 64-byte line of the kernel-argument segment, all in flight behind the kernel's FIRST scalar wait.  The compiler fetches
// kernel arguments lazily, cluster by cluster, each right before its first use; the scalar cache is cold at a launch's start, so every cluster
// on a new line is an L2 round trip of its own -- four or five of them, one after the other, between a wave's start and its first vector
// load in the latency-bound step kernels.  Touched up front the lines arrive together and the later fetches hit the scalar cache.
// (A value, not a statement: the caller hands it to the asm that pins its first round of scalar loads -- an `asm volatile` AHEAD of those
// loads would make the compiler treat the memory behind them as clobbered and turn them into vector loads.)
__device__ __forceinline__ int touch_kernargs(unsigned bytes) {
    typedef const int __attribute__((address_space(4))) cint;
    cint* ka = (cint*)__builtin_amdgcn_kernarg_segment_ptr();
    int t = 0;
    if (bytes > 64) t |= ka[16];
    if (bytes > 128) t |= ka[32];
    if (bytes > 192) t |= ka[48];
    if (bytes > 256) t |= ka[64];
    if (bytes > 320) t |= ka[80];
    if (bytes > 384) t |= ka[96];
    return t;
}

static inline dim3 grid1(size_t n, int b) { return dim3((unsigned)((n + b - 1) / b)); }

// ---- train-mode Dropout (models/mlp.py:20-21: nn.Dropout after the ReLU of every MLP layer wider than 1) ---------------------------
// Masks are never stored: element `idx` of the activation tensor identified by `stream` is kept iff a counter-based hash of
// (seed, stream, idx) says so, and forward and backward evaluate the same hash.  idx = row * width + column with row = the node
// id or the CALLER's edge id.  oracle/mpn_oracle.py:dropout_keep is the numpy twin (tests, goldens).
enum : unsigned {
    kDropEncNode1 = 1, kDropEncNode2 = 2, kDropEncEdge = 3,
    kDropEdgeStep = 16,   // + step (1-based)
    kDropNodeStep = 48,   // + step
    kDropCls = 80,        // + index of the classified step (0-based)
};
struct DropCfg {          // device-side view of gnncca_dropout; p == 0 everywhere when dropout is off
    float p_enc, p_edge, p_node, p_cls;
    const unsigned long long* seed;   // device word, read by the kernels (a captured training step replays with fresh masks)
};
__device__ __forceinline__ unsigned drop_hash(unsigned long long seed, unsigned stream, unsigned long long idx) {
    unsigned long long x = idx * 0x9E3779B97F4A7C15ull + (seed ^ ((unsigned long long)stream * 0xD1B54A32D192ED03ull));
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    return (unsigned)x;
}
// 0 (dropped) or 1 / (1 - p) (kept): uniform u = (hash >> 8) * 2^-24 in [0, 1), kept iff u >= p
__device__ __forceinline__ float drop_scale(unsigned long long seed, unsigned stream, unsigned long long idx, float p) {
    const float u = (float)(drop_hash(seed, stream, idx) >> 8) * (1.0f / 16777216.0f);
    return u >= p ? 1.0f / (1.0f - p) : 0.0f;
}

}  // namespace gnncca
