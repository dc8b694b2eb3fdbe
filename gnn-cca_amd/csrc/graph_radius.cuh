#pragma once
// Graph build with a ground-plane gate: of the dense build's cross-camera candidates (inference.py:207-212) a source keeps those within a
// radius on the ground plane.  The enumeration, the four (or two) attributes and the label of a kept edge are gnncca_build_edges' -- the
// same device statements, so a kept edge carries the dense build's bits -- but THE GATE HAS NO COUNTERPART IN THE REFERENCE'S GRAPH BUILD,
// which only builds complete graphs (its GEOM_TH is a baseline's threshold, not a graph gate).
//
// The gate (include/gnncca_mpn.h states it; gnncca_plan_frames_radius evaluates the identical IEEE sequence on the host):
//   s = dx * dx + dy * dy, dx = xw[i] - xw[j], dy = yw[i] - yw[j]   two products and one sum, each rounded once in float64, no FMA
//   t = radius (GNNCCA_RADIUS_UNIT_GROUND) or radius * max_dist[g] (GNNCCA_RADIUS_UNIT_MAX_DIST, one rounded product);  t2 = t * t
//   kept iff s <= t2   (a NaN compares false: a pair with a NaN position is dropped; radius = inf keeps every pair without one)
// s(i, j) == s(j, i) bit for bit (the difference only changes sign), so the list is closed under reversal by construction, and E is the
// host plan's count: no device-dependent size, no wait, no closure pass.
//
// Shape: build_edges_kernel with a stricter `valid` -- one wave per (source position, slice of its frame's 64-candidate chunks), one
// candidate per lane, the slot a ballot prefix, reid_sums_wave on the GATED mask only (the reid rows of dropped candidates are never read:
// where the dense kernel spends its time).  A wave first counts its source's kept candidates over the whole frame (positions and camera ids
// only) and compares the count with the plan's run edge_ptr[p + 1] - edge_ptr[p]: a source whose count disagrees (a plan of another batch
// or radius) is left unwritten rather than overrunning its run.  One launch, no workspace, no LDS, no atomics.
// Part of the translation unit graph_build.hip.

namespace gnncca {

__device__ __forceinline__ double radius_gate_t2(double radius, int unit, double md) {
    const double t = unit == GNNCCA_RADIUS_UNIT_MAX_DIST ? __dmul_rn(radius, md) : radius;
    return __dmul_rn(t, t);
}
__device__ __forceinline__ bool within_radius(double xi, double yi, double xj, double yj, double t2) {
    const double dx = __dsub_rn(xi, xj), dy = __dsub_rn(yi, yj);
    return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) <= t2;
}

template <int MODE>
__global__ __launch_bounds__(256) void build_edges_radius_kernel(const gnncca_frames fr, const float* __restrict__ reid, int R, int N,
                                                                 long long E, double radius, int unit, long long* __restrict__ ei_out,
                                                                 float* __restrict__ attr_out, float* __restrict__ lab_out,
                                                                 int* __restrict__ zero_ptr, int zero_n) {
    constexpr int NA = MODE == GNNCCA_EDGE_ATTR_FULL ? 4 : 2;
    // (gnncca_frames_forward_radius: the post-processing counters of the same batch are zeroed here, as build_edges_kernel does for the
    // dense chain -- ahead of the early returns: a wave without a source, or a source without a kept candidate, still does its share)
    if (zero_ptr && blockIdx.y == 0)
        for (int t = blockIdx.x * 256 + threadIdx.x; t < zero_n; t += gridDim.x * 256) zero_ptr[t] = 0;
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= N) return;
    const long long out0 = fr.edge_ptr[p];
    const int n_keep = fr.edge_ptr[p + 1] - fr.edge_ptr[p];
    if (n_keep <= 0 || out0 < 0 || out0 + n_keep > E) return;
    const int i = fr.src_order[p];
    const int g = fr.graph_of[i];
    const int gs = fr.graph_ptr[g], ge = fr.graph_ptr[g + 1];
    const int ci = fr.cam[i], pi = fr.person_id[i];
    const double xi = fr.xw[i], yi = fr.yw[i], md = fr.max_dist[g];
    const double t2 = radius_gate_t2(radius, unit, md);
    const float* __restrict__ ri = reid + (size_t)i * R;
    const bool vec4 = (R & 3) == 0;
    // the gate of the 64 candidates from j0 on: cross-camera (inference.py:210-211) and within the radius
    auto gated = [&](int j0) {
        const int j = j0 + lane;
        return j < ge && fr.cam[j] != ci && within_radius(xi, yi, fr.xw[j], fr.yw[j], t2);
    };
    // ---- 1. the source's kept candidates against the plan's run ----
    int total = 0;
    for (int j0 = gs; j0 < ge; j0 += 64) total += __popcll(__ballot(gated(j0)));
    if (total != n_keep) return;   // the device count disagrees with the plan: nothing is written for this source
    // ---- 2. emit, chunk by chunk, in the dense order.  The gate is evaluated again (positions and camera ids are in cache): carrying
    // pass 1's mask of a one-chunk frame over instead made the compiler serialise reid_sums_wave's five row loads per round -- one wait per
    // load where the dense kernel has all five in flight -- and the launch took 1.8x the dense one's time at the same E ----
    long long pos = out0;
    for (int c = 0, j0 = gs; j0 < ge; ++c, j0 += 64) {
        const int j = j0 + lane;
        const bool valid = gated(j0);
        const unsigned long long mask = __ballot(valid);
        const int n_valid = __popcll(mask);
        if (c % (int)gridDim.y == (int)blockIdx.y && mask != 0ull) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, lab = 0.f;
            if (valid) {
                lab = fr.person_id[j] == pi ? 1.f : 0.f;
                if (MODE != GNNCCA_EDGE_ATTR_ONLY_APPEARANCE) {
                    // sklearn paired_distances on float64 rows, / max_dist, .type(float32); no FMA contraction
                    double l2, l1;
                    ground_dists(xi, yi, fr.xw[j], fr.yw[j], l2, l1);
                    a0 = (float)__ddiv_rn(l2, md);
                    a1 = (float)__ddiv_rn(l1, md);
                }
            }
            if (MODE != GNNCCA_EDGE_ATTR_ONLY_DIST) {
                float sd = 0.f, sab = 0.f, saa = 1.f, sbb = 1.f;  // this lane's candidate: raw sums over the reid row
                reid_sums_wave(reid, ri, R, vec4, mask, lane, [&](int t) { return j0 + t; }, sd, sab, saa, sbb);
                const float emb = reid_emb(sd), cosv = reid_cos(sab, saa, sbb);
                if (MODE == GNNCCA_EDGE_ATTR_FULL) {
                    a2 = emb;
                    a3 = cosv;
                } else {
                    a0 = emb;
                    a1 = cosv;
                }
            }
            if (valid) {
                const long long k = pos + __popcll(mask & ((1ull << lane) - 1ull));
                ei_out[k] = i;
                ei_out[E + k] = j;
                if (NA == 4) {
                    *reinterpret_cast<float4*>(attr_out + k * 4) = make_float4(a0, a1, a2, a3);
                } else {
                    *reinterpret_cast<float2*>(attr_out + k * 2) = make_float2(a0, a1);
                }
                lab_out[k] = lab;
            }
        }
        pos += n_valid;
    }
}

}  // namespace gnncca
