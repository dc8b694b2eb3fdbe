#pragma once
// Part of the translation unit mpn_train.hip.
// Device-side weight packing: interprets the PackProgram of pack.cpp on the GPU, so that a training step (the
// optimizer has just changed every parameter) or a load_state_dict() never moves the parameters through the host.
// The arithmetic and the layouts are pack_elem.h's, the ones the host packer goes through: this file is the loop alone.
#include "pack_elem.h"

namespace gnncca {

constexpr int kMaxPackParams = 96;
struct PackPtrs {
    const float* p[kMaxPackParams];
};

__global__ __launch_bounds__(256) void pack_device_kernel(const PackProgram* __restrict__ prog, const PackPtrs ptrs,
                                                          float* __restrict__ blob) {
    const int n_segs = prog->n_segs;
    if ((int)blockIdx.y == n_segs) {  // the header
        const unsigned* h = reinterpret_cast<const unsigned*>(&prog->header);
        for (unsigned t = blockIdx.x * 256 + threadIdx.x; t < sizeof(BlobHeader) / 4; t += gridDim.x * 256)
            reinterpret_cast<unsigned*>(blob)[t] = h[t];
        return;
    }
    const PackSeg g = prog->segs[blockIdx.y];
    const PackSrc src = pack_src(g, ptrs.p);
    const long long total = (long long)g.rows * g.cols;
    int f16_bad = 0;   // kind 4: an element of this block does not fit fp16
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int r = (int)(t / g.cols), c = (int)(t - (long long)r * g.cols);
        if (pack_store(blob, g, r, c, pack_value(src, g, r, c, pack_scale(src, g, r)))) f16_bad = 1;
    }
    if (g.kind == 4) {   // (block-uniform) this block's overflow word: written every time, so a repack needs no reset and no atomics.
        // Element t belongs to block (t / 256) % 64: the grid is kW2hBadWords wide, which is the host packer's rule
        const int any = __syncthreads_or(f16_bad);
        if (threadIdx.x == 0 && blockIdx.x < kW2hBadWords) reinterpret_cast<unsigned*>(blob + g.plane)[blockIdx.x] = any ? 1u : 0u;
    }
}

}  // namespace gnncca
