// step_route.cpp -- the message steps' route: which instantiation of which step kernel every step of a forward launches.
// Pure C++ (no HIP, no pointer dereferenced but the dims / header / workspace structs), testable on a machine without a GPU
// (tests/test_step_route.py).  step_setup and launch_step_variant (mpn_forward.hip) carry the result out.
#include <algorithm>

#include "internal.h"

namespace gnncca {

const StepTuning& step_tuning() {
    static const StepTuning tuning = [] {
        StepTuning t;
        const int inf = 0x7FFFFFFF;
        t.force_wps = diag_env_int("GNNCCA_WPS", t.force_wps, 1, 4);
        t.force_npw = diag_env_int("GNNCCA_NPW", t.force_npw, 1, 2);
        t.npw_min_n = diag_env_int("GNNCCA_NPW_MIN_N", t.npw_min_n, 0, inf);
        t.npw_min_n_first = diag_env_int("GNNCCA_NPW_MIN_N_FIRST", t.npw_min_n_first, 0, inf);
        t.pd_lds_max = diag_env_int("GNNCCA_PD_LDS_MAX", t.pd_lds_max, 0, 1024);
        t.pd_lds_min = diag_env_int("GNNCCA_PD_LDS_MIN", t.pd_lds_min, 0, inf);
        t.force_nt = diag_env_int("GNNCCA_STEP_NT", t.force_nt, -1, 2);
        return t;
    }();
    return tuning;
}

StepPlan step_plan(const StepRouteIn& in, const StepTuning& t) {
    const gnncca_mpn_dims* d = in.d;
    const BlobHeader& hdr = *in.hdr;
    const Workspace& ws = *in.ws;
    const int N = in.N, E = in.E, L = d->num_enc_steps;
    StepPlan p{};
    p.launches = E <= 0 ? 0 : (L == 0 ? 1 : L);
    p.N = N, p.L = L;
    p.first_cls = L - d->num_class_steps + 1;  // models/mpn.py:277
    p.cls_layers = hdr.cls_layers;
    p.hin = (d->reattach_nodes ? 2 : 1) * kH;
    p.RE = d->reattach_edges != 0, p.MX = d->agg == GNNCCA_AGG_MAX;
    p.trace_h_steps = in.traced && in.trace_h_steps;
    // which arithmetic the node message uses (StepParams::msg_f32): the traced (general) and the fast kernels follow ONE rule
    p.msg_f32 = (N <= t.msg_f32_max_n || !step_pipe_fits(N, E, ws.e_stride, ws.total)) ? 1 : 0;
    p.attr_vec = d->edge_in == 4 && in.attr_aligned;
    // the specialised kernels: the shipped shape (fast_consts), 16-byte rows of edge_attr, no trace, 'sum' / 'mean'; L == 0 classifies
    // the encoded edge features once, on the general kernel (models/mpn.py:295-297)
    const bool special = hdr.fast_consts != 0 && p.attr_vec && !in.traced && !p.MX;
    p.family = (L == 0 || !special) ? kStepGeneral : (p.msg_f32 ? kStepFast : kStepPipe);
    // big, nearly regular batches keep the edge state in the padded layout (StepParams::ell_S); the decision is a pure
    // function of (dims, N, E) made in carve(); the plan validates the degrees against it on the device
    p.ell_S = (ws.ell_S > 0 && special && E > 0) ? ws.ell_S : 0;

    // waves per source-node segment: split a segment over 2 or 4 waves only while that is needed to put ~4 waves on
    // every SIMD (small graphs are latency-bound); big batches keep one wave per node, which amortises the
    // per-node prologue / projection epilogue over all of the node's chunks
    const long long avg_deg = (E + (long long)N - 1) / N;
    const int chunks = (int)((avg_deg + 63) / 64);
    const int by_chunks = chunks >= 4 ? 4 : (chunks >= 2 ? 2 : 1);
    // waves per node that would fill the chip; graphs whose nodes average >= 32 chunks (degree ~2000+) get four times that: the
    // tail of a launch is then a few long segments (dense3000: 0.4315 -> 0.4039 ms with four waves per node, dense2048 equal;
    // profiles/r03_logs/r3_wps1.log)
    const long long want = (chunks >= t.long_chunks ? t.fill_waves_long : t.fill_waves) / (long long)N;
    int wps = by_chunks;
    while (wps > 1 && wps > want) wps >>= 1;
    // GNNCCA_OPT_ENC_UNSPLIT promises logits that do not depend on the batch around a graph for batches of >= 4096 nodes: the
    // cross-wave combine sums in another order with another wave count, and `want` above depends on N (a shard of 2 x dense2048
    // would get four waves per node, the union of 8 one), so the option pins one wave per node there, the rule of every round
    // before the four-wave one (tests/test_gpu_sharded.py: dense2048 shard against its union, bitwise)
    if ((in.options & GNNCCA_OPT_ENC_UNSPLIT) != 0 && N >= 4096) wps = 1;
    if (t.force_wps == 1 || t.force_wps == 2 || t.force_wps == 4) wps = std::min(t.force_wps, by_chunks);
    p.wps = wps;
    // two nodes per wave (step_pipe.cuh: NPW): batches whose nodes average one round (<= 128 edges) and that still fill the chip with
    // half as many waves.
    // thresholds: from 16 384 nodes (step 1 at 8192: 14.9 -> 15.7 us; at 16 384: 29.8 -> 28.2).  The later steps alone from 8192 nodes, with
    // the classification deferred, move 64 x dense128 from 17.2 / 15.3 / 6.4 to 14.5 / 14.6 / 8.9 us per step: a tie per forward
    // (profiles/r04_logs/ab_npw{6,7}.log), so one threshold serves both
    p.npw_later = (wps == 1 && chunks <= 2 && (t.force_npw == 2 || (t.force_npw == 0 && N >= t.npw_min_n))) ? 2 : 1;
    p.npw_first = (p.npw_later == 2 && (t.force_npw == 2 || N >= t.npw_min_n_first)) ? 2 : 1;
    // column ranges instead of the col32 stream on steps 2 ... L of the specialised kernels (StepParams::rng)
    p.ranges = L >= 2 && (in.options & GNNCCA_OPT_COLUMN_RANGES) != 0;
    // The P_dst gather table staged whole in LDS: OFF by default since round 4.  Rounds 1-2 staged it for every N <= 1024; round 3 found
    // gathers straight from L2 ahead below 801 nodes (dense32 ... dense768 -1.3 ... -4 % per forward, r3_pdlds2.log, r3_pdlds3.log) and
    // kept it for 801 ... 1024; with four waves per node and the kernels as they are now the table loses there as well -- dense1024,
    // L = 8 (BASELINE config 5): 120.4 -> 118.3 us per forward with the fp32 edge state, 112.8 -> 110.1 with bf16
    // (profiles/r04_logs/ab_config5.log; with ONE wave per node the table still wins, 141 vs 151 us, but that form is slower anyway).
    // The switches keep the variant reachable for A/B runs: GNNCCA_PD_LDS_MIN / _MAX name the node range that stages it.
    p.pd_lds = (N >= t.pd_lds_min && N <= t.pd_lds_max) && L > 0;
    p.e_bf16 = (in.options & GNNCCA_OPT_EDGE_STATE_BF16) != 0;  // honoured by the specialised kernels only
    // cache policy of the edge-state streams, by the bytes of state a step leaves for the next one (step_fast.cuh has the measurements)
    const double state_bytes = (double)(p.e_bf16 ? kEF / 2 : kEF) * (double)ws.e_stride * 4.0;
    p.nt = state_bytes > t.nt_load_bytes ? 2 : (state_bytes > t.nt_store_bytes ? 1 : 0);
    if (t.force_nt >= 0) p.nt = t.force_nt;
    // DEFERRED classification (step_pipe.cuh: CIN): a message step that produces a classified state does not classify it; the step that reads
    // the state back does (the last step: its input and its output).  The classifying message steps then run the variant without the
    // classifier -- lighter, and eligible for two nodes per wave.  Where it pays: forwards whose message steps run two nodes per wave;
    // fp32 edge state only (the bf16 state is rounded after its step classified it); logits bit for bit the same.
    p.defer = p.family == kStepPipe && !p.e_bf16 && !p.pd_lds && !p.ranges && p.first_cls < L && !in.dropping && p.npw_later == 2;
    return p;
}

StepLaunch step_launch(const StepPlan& p, int step) {
    const int L = p.L;
    StepLaunch l{};
    l.family = p.family, l.RE = p.RE, l.MX = p.MX, l.NPW = 1;
    l.first = step <= 1, l.update = step >= 1, l.store_e = step >= 1 && step < L;
    l.npw = step == 1 ? p.npw_first : p.npw_later;
    l.stamp_slot = step >= 1 ? 2 + std::min(step - 1, 5) : 0;
    l.MSG = step >= 1 && (step < L || p.trace_h_steps);
    // the tables of per-node projections alternate: step s reads what the encoder (s == 1) or step s - 1 wrote
    l.buf_in = step >= 1 ? (step - 1) & 1 : -1;
    l.buf_out = l.store_e ? step & 1 : -1;
    // logit slots.  Not deferred: classifying step s writes slot s - first_cls.  Deferred: message steps do not classify their output;
    // step s classifies its INPUT (step s - 1's output) where that is a classified state, the last step its output as well
    const bool classifies = step == 0 || step >= p.first_cls;
    l.slot_out = l.slot_in = -1;
    if (p.defer) {
        if (step == L) l.slot_out = L - p.first_cls;
        if (step - 1 >= p.first_cls) l.slot_in = step - 1 - p.first_cls;
    } else if (classifies) {
        l.slot_out = l.cls_no = std::max(0, step - std::max(p.first_cls, 1));
    }
    l.cls_layers = l.slot_out >= 0 ? p.cls_layers : 0;
    l.CLS = l.cls_layers != 0;

    const int npg = 4 / p.wps;   // nodes per workgroup
    l.blocks = (unsigned)((p.N + npg - 1) / npg);
    if (p.family == kStepGeneral) {
        l.lds = ((l.MSG ? (size_t)p.hin * kProjOut : 0) + 4 * kH + (p.pd_lds ? (size_t)p.N * kPdStride : 0)) * sizeof(float);
        return l;
    }
    const bool two = l.npw == 2 && p.wps == 1;   // this step of this forward would run two nodes per wave
    if (l.slot_in >= 0) {   // the nine CIN forms (deferral implies fp32 state, no table, no ranges)
        l.FIRST = false, l.CIN = true, l.NT = p.nt;
        l.NPW = l.MSG && two ? 2 : 1;
    } else {
        l.FIRST = l.first, l.PDL = p.pd_lds, l.EB = p.e_bf16;
        l.NT = l.PDL ? 0 : p.nt;                                                // no non-temporal variant with the LDS table
        if (p.family == kStepPipe) {
            l.RNG = p.ranges && l.NT == 0 && (!l.FIRST || l.MSG);               // not under a non-temporal policy; not where step 1 has nothing to derive for
            l.NPW = two && !p.ranges && step_variant_exists(kStepPipe, l.FIRST, l.CLS, l.MSG, l.PDL, l.EB, l.NT, false, 2, false) ? 2 : 1;
        }
    }
    if (l.NPW == 2) l.blocks = (unsigned)((p.N + 7) / 8);
    // [32][48] projection (MSG) + [4][32] partials + [4][4] range findings + the P_dst table (the pipe kernel's with a zero row behind it)
    const size_t pd_rows = !l.PDL ? 0 : (size_t)p.N + (p.family == kStepPipe ? 1 : 0);
    l.lds = ((l.MSG ? (size_t)kH * kProjOut : 0) + 4 * kH + 16 + pd_rows * kPdStride) * sizeof(float);
    return l;
}

}  // namespace gnncca
