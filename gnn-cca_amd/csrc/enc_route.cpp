// enc_route.cpp -- the node encoder's route: which GEMM form each layer runs on, where the graph plan goes, which tail follows.
// Pure C++ (no HIP, no pointer dereferenced but the dims / header / workspace structs): a handful of integer compares per forward,
// testable on a machine without a GPU (tests/test_encoder_route.py).  launch_node_encoder (mpn_forward.hip) carries the result out.
#include <algorithm>

#include "internal.h"

namespace gnncca {

const EncTuning& enc_tuning() {
    static const EncTuning tuning = [] {
        EncTuning t;
        const int inf = 0x7FFFFFFF;
        t.split_min = diag_env_int("GNNCCA_GEMM_SPLIT_MIN", t.split_min, 0, inf);
        t.lds_min = diag_env_int("GNNCCA_GEMM_LDS_MIN", t.lds_min, 0, inf);
        t.r32f_min = diag_env_int("GNNCCA_GEMM_R32F_MIN", t.r32f_min, 0, inf);
        t.r32f_max = diag_env_int("GNNCCA_GEMM_R32F_MAX", t.r32f_max, 0, inf);
        t.slices_min = diag_env_int("GNNCCA_GEMM_SLICES_MIN", t.slices_min, 0, inf);
        t.slices_max = diag_env_int("GNNCCA_GEMM_SLICES_MAX", t.slices_max, 0, inf);
        t.slices_nks = diag_env_int("GNNCCA_GEMM_SLICES_NKS", t.slices_nks, 1, 32);
        t.slices_wgs = diag_env_int("GNNCCA_GEMM_SLICES_WGS", t.slices_wgs, 1, 1 << 20);
        t.tail_mfma_min = diag_env_int("GNNCCA_TAIL_MFMA_MIN", t.tail_mfma_min, 0, inf);
        t.gemm_bf16 = diag_env("GNNCCA_GEMM_BF16") != nullptr;
        t.f16_force_arm = diag_env_int("GNNCCA_GEMM_F16_ARM", t.f16_force_arm, 0, 1);
        t.f16_x_nt = diag_env_int("GNNCCA_GEMM_F16_XNT", t.f16_x_nt, -1, 1);
        return t;
    }();
    return tuning;
}

static int fold(int plan_blocks, int span) { return span > 1 ? (plan_blocks + span - 1) / span : plan_blocks; }

// Layer 0: the form, its slab count and where the plan goes.  (Every later GEMM layer is kEncPlanGemm in one slab, no plan.)
static void route_first_layer(const EncRouteIn& in, const EncTuning& t, EncRoute& r) {
    const gnncca_mpn_dims* d = in.d;
    const BlobHeader& hdr = *in.hdr;
    const int N = in.N, nl = d->enc_node.n_layers, ksplit = in.ws->ksplit;
    EncGemmRoute& g = r.gemm[0];
    const int K = g.K, O = g.O;
    const bool unsplit = (in.options & GNNCCA_OPT_ENC_UNSPLIT) != 0;
    // The fp16-split image of the first layer (enc_f16.cuh) is usable: it is the default wherever it applies; the bf16 forms stay for
    // GNNCCA_OPT_ENC_UNSPLIT (whose bitwise batch independence is stated on the bf16 arithmetic of all three un-split kernels), for
    // GNNCCA_OPT_ENC_SPLIT3 (an option of that form) and as the A/B reference (GNNCCA_GEMM_BF16).
    const bool f16_ok = hdr.enc_w2h != 0 && !r.split3 && !t.gemm_bf16 && !unsplit;
    // Fusable: un-split and the shipped encoder shape (in -> 128 -> 32, no reattach): the rest of the encoder, the step-1
    // projections and the plan fold run in the GEMM's epilogue, on the tile while it is on chip
    const bool fusable = !in.dropping && nl == 2 && d->enc_node.layers[1].in_dim == 128 && d->enc_node.layers[1].out_dim == kH &&
                         !d->reattach_nodes && hdr.proj_wT != 0;
    const int plan_place_riding = in.E > 0 ? kPlanRides : kPlanNone;

    // round 6: below 4096 nodes the first layer runs on the fp16-split GEMM in 32-row tiles with K split over one round of workgroups
    // (enc_f16_slices.cuh): a fraction of the slabs of the two forms above (dense1024: 8 x 0.5 MB instead of 16 x 0.5 MB written and read
    // back; dense256: 16 instead of 32) and half the matrix work of the six-product form.  nks: at least K / 256, then powers of two
    // while one round of workgroups holds the tiles (nrt * nks <= 256), a slice stays >= 64 deep and the workspace has the slabs.
    // The minimum K / 256 is taken even where nrt * nks exceeds one round (K = 2048 near N = 4095: 128 x 8 = 1024 workgroups).
    if (f16_ok && O == 128 && K >= 64 && (K & (K - 1)) == 0 && K / kEncSliceMaxK <= ksplit && N >= t.slices_min && N <= t.slices_max &&
        in.x_aligned) {
        const int nrt = (N + 31) / 32;
        // slices: at least K / 256 (a workgroup's x tile is 32 KB of LDS), then powers of two while one round of workgroups holds the tiles, a
        // slice stays >= 64 deep and the workspace has the slabs (dense1024 -> 8, dense256 and below -> 16: 32 slices of 64 measured 0.7 us slower per dense256 forward, 8 of 256 1.4 us)
        int nks = 1;
        while (K / nks > kEncSliceMaxK) nks *= 2;
        while (nks * 2 <= std::min(t.slices_nks, ksplit) && nrt * nks * 2 <= t.slices_wgs && K / (nks * 2) >= 64 && (K / (nks * 2)) % 64 == 0) nks *= 2;
        g.form = kEncSlices, g.slabs = nks, g.kslice = K / nks;
        r.plan_place = plan_place_riding;
        r.plan_span = in.plan_span;
        r.plan_wgs = (fold(in.plan_blocks, in.plan_span) + 1) / 2;   // two plan blocks per 512-thread workgroup
        return;
    }
    // From 384 nodes on the first encoder layer runs on the split-bf16 MFMA GEMM, the plan riding in its launch.  (Round 3 lowered this
    // from 4096 to 1024 -- f32 MFMA GEMM + plan 19.5 us at dense1024, 43 at dense2048; 128-row split kernel + a plan launch 11.0 + 5.8
    // and 17.4 + 17.1, r3_gemm_split_min.log -- and, once the plan rode along, to 384: GEMM 11.5 / 12.1 / 17.7 / 20.8 -> 9.3 / 9.2 /
    // 10.5 / 13.2 us at 384 / 512 / 768 / 896 nodes, 3 x dense256 17.0 -> 10.0; at 256 nodes the f32 form stays ahead, 6.6 vs 7.6;
    // r3_split_min2.log)
    if (!(hdr.enc_w3 != 0 && N >= t.split_min && in.x_aligned)) {
        // the f32 plan GEMM keeps the slab count carve() chose; the graph plan rides in its launch, always in the narrow form
        r.plan_place = plan_place_riding;
        r.plan_span = 0;
        r.plan_wgs = in.plan_blocks;
        return;
    }
    // big batches: split-bf16 MFMA GEMM.  256-row workgroups, both operands through LDS (144 KB: one workgroup per CU, 8 waves), from
    // 6144 nodes; split-K by whole rounds of 256 workgroups (enc_lds_ksplit)
    const bool use_lds = N >= t.lds_min && O == 128;
    const int lds_ks = use_lds ? std::min(enc_lds_ksplit(N, K), ksplit) : 1;
    // the 32-row forms: un-split, fused epilogue, where the 256-row form would run split-K
    const bool rows32_fit = fusable && O == 128 && K % 256 == 0 && !(use_lds && lds_ks == 1);
    // GNNCCA_OPT_ENC_UNSPLIT: batches of >= 4096 nodes never split K -- where the 256-row form would, 32-row workgroups run
    // un-split with the same fused epilogue (enc_rows32.cuh), so a node's encoder output is bit for bit independent of the batch
    // around it (a shard of a sharded batch reproduces the union's logits exactly).  Not the default: one wave per SIMD at
    // N <= 8192 (N = 8192: 41-43.5 us against 28 + 9 for split-K + tail; enc_rows32.cuh says where the time goes)
    const bool use_r32 = unsplit && rows32_fit && N >= 4096;
    // round 5: mid-size batches on the fp16-split form take 32-row workgroups that split K over their WAVES and finish the encoder in
    // the epilogue (enc_f16.cuh: enc_gemm_f16_rows32_kernel) -- no slabs, no tail launch.  Range: 4096 ... 8192 nodes, i.e. while the
    // row tiles fit ONE round of workgroups: every 32-row workgroup pulls all 1 MB of W through its CU's L2 path (~70 GB/s: 14 us), which
    // a second round doubles (plan + GEMM + tail, same box: 25.3 / 26.4 / 27.4 / 28.6 / 30.4 us at 4096 / 5120 / 6144 / 7168 / 8192 nodes
    // against 26.6 / 35.0 / 31.2 / 33.0 / 38.3 for the split-K forms; 47.4 against 39.2 at 9216; profiles/r05_logs/ab_r32f_2.log)
    const bool use_r32f = !use_r32 && rows32_fit && f16_ok && N >= t.r32f_min && N <= t.r32f_max;
    g.slabs = 1;
    if (use_r32f) {
        g.form = kEncR32F16;
    } else if (use_r32) {
        g.form = kEncR32Bf16;
        g.nst = (N + 31) / 32 <= 256 ? 8 : 4;
    } else if (use_lds) {
        // K / slabs is a multiple of 32 on this path
        g.form = (f16_ok && K % 32 == 0 && (K / lds_ks) % 32 == 0) ? kEncLdsF16 : kEncLdsBf16;
        g.slabs = lds_ks;
    } else {
        // 128-row workgroups (a wave = 32 rows x 128 columns); split-K until >= 512 workgroups are in flight
        g.form = kEncD128;
        while (g.slabs < ksplit && ((N + 127) / 128) * g.slabs < 512 && (K / (g.slabs * 2)) % 32 == 0) g.slabs *= 2;
    }
    g.kslice = K / g.slabs;
    r.fused = g.form == kEncR32F16 || g.form == kEncR32Bf16 || (use_lds && fusable && lds_ks == 1);
    // Where the plan goes.  Fused: FIRST, so that one extra workgroup of the GEMM launch can fold its findings (and repair an unsorted
    // graph): no tail launch is left in this regime.  128-row form: it rides (extra workgroups beyond the GEMM tiles), narrow (0) or
    // pair form by the edge count and alignment.  256-row forms that are not fused: a launch of its own behind the GEMM.
    // (The plan does not ride in the 256-row launch.  As extra workgroups: every workgroup reserves the 144 KB of dynamic LDS, so the
    // plan's queue one per CU behind the GEMM tiles, 29 -> 45 us at N = 8192.  Inside the GEMM waves, a 1024-edge block per wave
    // under the first operands' round trip: the block's own two dependent round trips are then exposed in every workgroup,
    // 29.5 + 6.4 -> 37.6 us.  profiles/r03_logs/r3_ride2.log, r3_ride4.log.)
    // (Round 4 re-measured the plan BESIDE this GEMM on a side stream, fork / join by events, now under HIP-graph replay: 64 x dense128
    // 98 -> 108 us per forward, 96 x dense128 130 -> 140, 64 x dense256 239 -> 244 -- both kernels slow each other down (GEMM 26.5 ->
    // 29, plan 5.9 -> 10 us) and the cross-queue hand-offs cost more than the plan's launch; round 1 had found the same with eager
    // launches.  profiles/r04_logs/ab_planfork1.log)
    // (Round 4 also let the plan ride in the TAIL launch of this regime -- plan workgroups behind enc_tail_mfma_kernel's, the last one
    // to arrive folding: the bare co-run, with no arrival count at all, takes 14.4 us against 5.9 + 9.7 at N = 8192 and 35-37 against
    // 17.6 + 14.8 at 64 x dense256 (the plan's stream at the tail's 192-VGPR occupancy); the arrival count costs ~15 ns per plan
    // workgroup (one address, eight L2s: 22.9 us) and the release fence in front of it ~95 ns (an L2 write-back each: 117-120 us).
    // profiles/r04_logs/ab_tailride{1,2,3}.log)
    r.plan_place = in.E <= 0 ? kPlanNone : r.fused ? kPlanBefore : g.form == kEncD128 ? kPlanRides : kPlanAfter;
    r.plan_span = in.plan_span;
    r.plan_wgs = fold(in.plan_blocks, in.plan_span);
}

EncRoute encoder_route(const EncRouteIn& in, const EncTuning& t) {
    const gnncca_mpn_dims* d = in.d;
    const int N = in.N, nl = d->enc_node.n_layers;
    EncRoute r{};
    r.n_gemm = nl == 1 ? 1 : nl - 1;
    r.split3 = (in.options & GNNCCA_OPT_ENC_SPLIT3) != 0;
    r.force_arm = t.f16_force_arm;
    for (int g = 0; g < r.n_gemm; ++g) {   // every layer as the f32 plan GEMM first: layer 0 in carve()'s slab count, the others in one
        const gnncca_layer& l = d->enc_node.layers[g];
        EncGemmRoute& q = r.gemm[g];
        q.form = kEncPlanGemm, q.K = l.in_dim, q.O = l.out_dim;
        q.slabs = g == 0 ? in.ws->ksplit : 1;
        q.kslice = ((q.K + q.slabs - 1) / q.slabs + 63) / 64 * 64;
        // layer g > 0 reads the activation buffer: aligned with the workspace wherever K % 4 == 0
        q.vec_ok = q.K % 4 == 0 && (g == 0 ? in.x_aligned : in.ws_aligned);
    }
    route_first_layer(in, t, r);
    // x stream of the fp16-split GEMMs: NON-TEMPORAL from 128 MB of x on (N >= 16 384 at K = 2048).  Inside a real forward the caches are full
    // of what the previous forward's step kernels left (dirty edge state), and a default-policy x stream fights it for every line: BASELINE
    // config 4 in situ 174 -> 137 us for this launch (0.516 -> 0.485 ms per forward), while an encoder timed alone on clean caches hides
    // the difference (121 us either way); at the 8 192-node share the policy costs 1 us, so small batches keep the default
    // (profiles/r05_logs/ab_config4_nt.log).  GNNCCA_GEMM_F16_XNT = 0 / 1 forces it off / on.
    r.x_nt = t.f16_x_nt >= 0 ? t.f16_x_nt : ((double)N * r.gemm[0].K * 4.0 >= 128.0 * 1024 * 1024 ? 1 : 0);

    // ---- the tail: sums the last GEMM's slabs, applies the last layer, writes h0 and the step-1 projections ----
    const int F = d->enc_node.layers[r.n_gemm - 1].out_dim, hin = (d->reattach_nodes ? 2 : 1) * kH;
    const bool has_last = nl >= 2;
    r.tail_vec = (F % 4 == 0) && (F / 4 <= 64) && (64 % (F / 4) == 0);
    const size_t lds = ((size_t)hin * kProjOut + (has_last ? (size_t)F * kH : 0) + 4 * (size_t)F + 4 * 256) * sizeof(float);
    r.tail_lds = std::max<size_t>(lds, 4096);
    // graphs and batches whose GEMM ran split-K: the tail on the matrix pipe, 32 nodes per workgroup, from 2560 nodes (round 3 lowered this
    // from 6144: 8.7 -> 6.9 us at N = 4096, 10.3 -> 7.5 at 5120, 10.4 -> 7.0 at 4000, 9.2 -> 7.2 at 3000, 8.6 -> 6.4 at 3072; equal at 2048
    // (6.2), the register-resident tail ahead at 1024 (5.0 vs 7.6); profiles/r03_logs/r3_thresh1.log, r3_thresh2.log)
    const bool tail_mfma = !r.fused && !in.dropping && N >= t.tail_mfma_min && nl == 2 && d->enc_node.layers[0].out_dim == 128 &&
                           !d->reattach_nodes && in.ws_aligned;
    // register-resident tail in the latency-bound regime only: on big batches it is VALU-bound (readlane traffic) and
    // measured 15 % slower than the LDS form (72 vs 62 us at N = 65 536)
    const bool tail_fast = !tail_mfma && !in.dropping && N < 4096 && F == 128 && has_last && !d->reattach_nodes && !in.trace_h && r.tail_vec &&
                           in.ws_aligned;
    // nodes per workgroup of the fast tail: one up to 320 nodes, two up to 640, four beyond (a block of 200 forwards in one HIP graph:
    // dense256 28.07 -> 27.4 us per forward with one, dense64 24.7 -> 24.1; dense512 39.97 -> 39.5-39.8 with two; dense1024 best with four;
    // profiles/r03_logs/r3_tailnpw1.log)
    r.tail_npw = N <= 320 ? 1 : (N <= 640 ? 2 : 4);
    r.tail = lds > 160 * 1024 ? kTailRefused : r.fused ? kTailNone : tail_fast ? kTailFast : tail_mfma ? kTailMfma : kTailLds;
    return r;
}

}  // namespace gnncca
