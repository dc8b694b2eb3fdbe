#pragma once
// Graph build with a ground-plane gate: of the dense build's cross-camera candidates (inference.py:207-212) a source keeps those within a
// radius on the ground plane.  The enumeration, the four (or two) attributes and the label of a kept edge are gnncca_build_edges': this
// kernel calls graph_build.hip's emit_edges, as the dense one does, so a kept edge carries the dense build's bits -- but THE GATE HAS NO
// COUNTERPART IN THE REFERENCE'S GRAPH BUILD, which only builds complete graphs (its GEOM_TH is a baseline's threshold, not a graph gate).
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
    zero_counters(zero_ptr, zero_n, blockIdx.y == 0, 256);
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= N) return;
    const long long out0 = fr.edge_ptr[p];
    const int n_keep = fr.edge_ptr[p + 1] - fr.edge_ptr[p];
    if (n_keep <= 0 || out0 < 0 || out0 + n_keep > E) return;
    const EdgeSource s = load_edge_source(fr, reid, R, p);
    const double t2 = radius_gate_t2(radius, unit, s.md);
    // the gate of the 64 candidates from j0 on: cross-camera (inference.py:210-211) and within the radius
    auto gated = [&](int j0) {
        const int j = j0 + lane;
        return j < s.ge && fr.cam[j] != s.ci && within_radius(s.xi, s.yi, fr.xw[j], fr.yw[j], t2);
    };
    // ---- 1. the source's kept candidates against the plan's run ----
    int total = 0;
    for (int j0 = s.gs; j0 < s.ge; j0 += 64) total += __popcll(__ballot(gated(j0)));
    if (total != n_keep) return;   // the device count disagrees with the plan: nothing is written for this source
    // ---- 2. emit, chunk by chunk, in the dense order.  The gate is evaluated again (positions and camera ids are in cache): carrying
    // pass 1's mask of a one-chunk frame over instead made the compiler serialise reid_sums_wave's five row loads per round -- one wait per
    // load where the dense kernel has all five in flight -- and the launch took 1.8x the dense one's time at the same E ----
    long long pos = out0;
    for (int c = 0, j0 = s.gs; j0 < s.ge; ++c, j0 += 64) {
        const int j = j0 + lane;
        const bool valid = gated(j0);
        const unsigned long long mask = __ballot(valid);
        if (c % (int)gridDim.y == (int)blockIdx.y && mask != 0ull)
            emit_edges<MODE>(fr, reid, R, s, j, valid, mask, lane, [&](int t) { return j0 + t; }, pos, [](long long) { return true; }, E,
                             ei_out, attr_out, lab_out);
        pos += __popcll(mask);
    }
}

}  // namespace gnncca
