// pack_elem.h -- what is true of ONE element of ONE segment of the pack program (internal.h: PackSeg): where its value comes from, the
// BatchNorm fold, the piece splits and where it lands in the blob.  The host packer (pack.cpp) and the device packer (pack_device.cuh)
// are two loops over the same program that both go through these functions, so a blob converted on the host and one refreshed on the
// device after an optimiser step agree to the byte.  Compiles as device code, as host code of a HIP unit and as plain C++.
#pragma once
#include <math.h>
#include <stdint.h>

#include "internal.h"

#ifdef __HIP__
#define GNNCCA_HD __host__ __device__
#else
#define GNNCCA_HD
#endif

namespace gnncca {

// ---- the BatchNorm fold -----------------------------------------------------------------------------------------------------------
// eval-mode BatchNorm1d (models/mlp.py:14-15, eps = 1e-5: torch's default) folded into the Linear in front of it:
//     y = ((W x + b) - mean) / sqrt(var + 1e-5) * gamma + beta  ==  (s W) x + ((b - mean) s + beta),   s = gamma / sqrt(var + 1e-5)
// in double, every operation rounded on its own and the result rounded once to fp32: the device spells the operations as intrinsics, the
// host switches contraction off, so that no compiler flag can fuse a multiply with an add on one side only.
GNNCCA_HD inline double bn_scale(float gamma, float var) {
#ifdef __HIP_DEVICE_COMPILE__
    return __ddiv_rn((double)gamma, __dsqrt_rn(__dadd_rn((double)var, 1e-5)));
#else
#pragma clang fp contract(off)
    return (double)gamma / sqrt((double)var + 1e-5);
#endif
}
GNNCCA_HD inline float bn_fold_weight(float w, double s) {
#ifdef __HIP_DEVICE_COMPILE__
    return (float)__dmul_rn((double)w, s);
#else
#pragma clang fp contract(off)
    return (float)((double)w * s);
#endif
}
GNNCCA_HD inline float bn_fold_bias(float b, float mean, double s, float beta) {
#ifdef __HIP_DEVICE_COMPILE__
    return (float)__dadd_rn(__dmul_rn(__dsub_rn((double)b, (double)mean), s), (double)beta);
#else
#pragma clang fp contract(off)
    return (float)(((double)b - (double)mean) * s + (double)beta);
#endif
}

// ---- where a segment's values come from -------------------------------------------------------------------------------------------
struct PackSrc {
    const float *v, *gamma, *beta, *mean, *var;   // the Linear's tensor; its BatchNorm's four, or gamma == nullptr
};
GNNCCA_HD inline PackSrc pack_src(const PackSeg& g, const float* const* params) {
    PackSrc s = {params[g.param], nullptr, nullptr, nullptr, nullptr};
    if (g.bn >= 0) s.gamma = params[g.bn], s.beta = params[g.bn + 1], s.mean = params[g.bn + 2], s.var = params[g.bn + 3];
    return s;
}
// the fold scale of row r (the same for every column: an interpreter that walks a row may compute it once)
GNNCCA_HD inline double pack_scale(const PackSrc& s, const PackSeg& g, int r) {
    return s.gamma ? bn_scale(s.gamma[g.unit0 + r], s.var[g.unit0 + r]) : 1.0;
}
// the value of element (r, c): the parameter element, through the fold where the layer has a BatchNorm
GNNCCA_HD inline float pack_value(const PackSrc& s, const PackSeg& g, int r, int c, double scale) {
    const float v = s.v[(size_t)g.src_off + (size_t)r * g.srs + (size_t)c * g.scs];
    if (!s.gamma) return v;
    return g.kind == 1 ? bn_fold_bias(v, s.mean[g.unit0 + r], scale, s.beta[g.unit0 + r]) : bn_fold_weight(v, scale);
}

// ---- piece splits -----------------------------------------------------------------------------------------------------------------
// fp32 -> bf16, round to nearest even by the integer rule (finite inputs; weights are finite)
GNNCCA_HD inline uint16_t bf16_rne(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
GNNCCA_HD inline float bf16_to_float(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// v = h0 + h1 + h2 with bf16 pieces (24 mantissa bits in all): the split-bf16 GEMM and message multiply the pieces on the bf16 MFMA
// pipe and recover fp32-level accuracy
struct Bf16x3 {
    uint16_t h0, h1, h2;
};
GNNCCA_HD inline Bf16x3 split_bf16x3(float v) {
    Bf16x3 p;
    p.h0 = bf16_rne(v);
    const float r1 = v - bf16_to_float(p.h0);
    p.h1 = bf16_rne(r1);
    p.h2 = bf16_rne(r1 - bf16_to_float(p.h1));
    return p;
}
// v = w0 + w1 / 2048 with fp16 pieces (w1 = the residual scaled into w0's exponent range; 22 significant bits in all): the fp16-split GEMM
// of enc_f16.cuh needs THREE piece products where the bf16 form needs six.  `(_Float16)` is round to nearest even with subnormals kept
// and |v| >= 65520 -> infinity on both sides (v_cvt_f16_f32 in the default float mode; the compiler's conversion on the host).  `bad`: v is
// beyond fp16's range (or not a number), and the GEMM must hand its tiles to the bf16 arm.
struct F16x2 {
    _Float16 w0, w1;
    bool bad;
};
GNNCCA_HD inline F16x2 split_f16x2(float v) {
    F16x2 p;
    p.w0 = (_Float16)v;
    p.w1 = (_Float16)((v - (float)p.w0) * 2048.0f);
    p.bad = !(fabsf(v) < kF16Limit);
    return p;
}

// ---- destination addressing -------------------------------------------------------------------------------------------------------
// kind 2, in bf16 elements from BlobHeader::enc_w3: [in/32][3 pieces][out][32], g.plane = out * 32 between the pieces.  The 32-deep k-chunk
// a GEMM workgroup stages per iteration (all three pieces of all output columns, 24 KB for out = 128) is one contiguous run -- full-line
// coalesced loads.  (o, i) = (output column, input).
GNNCCA_HD inline size_t w3_index(const PackSeg& g, int o, int i) {
    return (size_t)(i / 32) * 3 * (size_t)g.plane + (size_t)o * 32 + (size_t)(i % 32);
}
// kind 3, in bf16 elements from BlobHeader::wne_bf16: the B operands of the split-bf16 message (msg_bf16.cuh: MsgB).  Dword
// [plane * 3 + k / 2][lane] holds the pieces of (W_ne[ch][k], W_ne[ch][k + 1]), k even, ch = lane & 31.  Plane 0 = first pieces in both
// lane halves, plane 1 = second pieces, plane 2 = third pieces in lanes < 32 and FIRST pieces in lanes >= 32.
GNNCCA_HD inline size_t msgb_index(int plane, int lane, int k) { return ((size_t)(plane * 3 + k / 2) * 64 + lane) * 2 + (k & 1); }
// kind 4, in halfs from BlobHeader::enc_w2h: position of piece 0 of weight element (output column o, input i); piece 1 sits 128 * 32 halfs
// further.  FRAGMENT-major inside a 32-deep chunk: [piece][column tile c = o / 32][k-step s = (i % 32) / 16][lane = o % 32 + 32 * ((i % 16) / 8)][i % 8] --
// the 1 KB the 64 lanes of one B operand of v_mfma_f32_32x32x16_f16 hold is one contiguous run, so the same image serves the LDS ring of
// the 256-row kernel (ds_read_b128 at consecutive addresses: conflict-free without a swizzle) and the straight-to-register loads of the
// 32-row kernel (one fully coalesced 1 KB load per fragment)
GNNCCA_HD inline size_t w2h_index(int o, int i) {
    const int kk = i % 32, lane = (o % 32) + 32 * ((kk % 16) / 8);
    return (size_t)(i / 32) * (2 * 128 * 32) + (size_t)((((o / 32) * 2 + kk / 16) * 64 + lane) * 8 + (kk % 8));
}

// ---- the one store ----------------------------------------------------------------------------------------------------------------
// Stores element (r, c) of segment g, whose value is v, into the blob.  Returns whether the element does not fit fp16 (kind 4 only): the
// caller owns the flag words (BlobHeader::enc_w2h_bad; element t = r * cols + c belongs to word (t / 256) % kW2hBadWords).
GNNCCA_HD inline bool pack_store(float* blob, const PackSeg& g, int r, int c, float v) {
    if (g.kind <= 1) {   // plain strided
        blob[(size_t)g.dst + (size_t)r * g.drs + (size_t)c * g.dcs] = v;
        return false;
    }
    uint16_t* h = reinterpret_cast<uint16_t*>(blob + g.dst);
    if (g.kind == 4) {
        const F16x2 p = split_f16x2(v);
        const size_t k = w2h_index(r, c);
        __builtin_memcpy(h + k, &p.w0, 2);
        __builtin_memcpy(h + k + 128 * 32, &p.w1, 2);
        return p.bad;
    }
    const Bf16x3 p = split_bf16x3(v);
    if (g.kind == 2) {
        const size_t k = w3_index(g, r, c);
        h[k] = p.h0, h[(size_t)g.plane + k] = p.h1, h[2 * (size_t)g.plane + k] = p.h2;
    } else {   // kind 3: row = channel
        h[msgb_index(0, r, c)] = h[msgb_index(0, r + 32, c)] = p.h0;
        h[msgb_index(1, r, c)] = h[msgb_index(1, r + 32, c)] = p.h1;
        h[msgb_index(2, r, c)] = p.h2;
        h[msgb_index(2, r + 32, c)] = p.h0;
    }
    return false;
}

}  // namespace gnncca
