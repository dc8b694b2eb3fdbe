// mpn_forward.hip -- gfx950 (MI355X / CDNA4) inference kernels and the C-ABI forward of the GNN-CCA message-passing path.
//
// Algebra (derived from models/mpn.py:48,68-69,97-99): with the edge-MLP weight split by the
// cat order [x[row] | x[col] | e] and the node-MLP weight by [x[row] | e'],
//     P_src = h W_src^T + b_e,  P_dst = h W_dst^T,  Q = h W_nx^T + b_n            (per node, tiny)
//     e'[k] = ReLU(P_src[row k] + P_dst[col k] + W_ee e[k])                         (per edge, VALU)
//     m[k]  = ReLU(Q[row k] + W_ne e'[k])                                           (per edge, MFMA 32x32x2 f32)
//     h'[i] = agg_{k : row k = i} m[k]                                              (in-register, per segment)
// so no [E,70] / [E,38] concatenation is ever materialised.  The aggregation index is `row` (the SOURCE node),
// exactly as the reference does it (mpn.py:99).
//
// Data layout in HBM (all fp32):
//   edge state   e      : 6 feature planes [6][E_pad]  in ROW-SORTED edge order  -> coalesced 256-B wave loads
//   gather table Pd     : [N][8]   (P_dst, 32-B rows)                             -> L1/L2-resident random reads
//   segment table PsQ   : [N][40]  (P_src | pad | Q)                              -> wave-uniform reads
//   topology     seg_ptr: [N+1] int32 CSR offsets by source node;  col32 [E] int32 (sorted order)
// One wave owns (a share of) one source node's contiguous edge segment, so the per-destination reduction needs
// no atomics and is bitwise reproducible.
//
// This translation unit is INFERENCE: the graph plan, the node encoder's GEMM forms, the message-passing step kernels, the generic family
// and the forward itself (forward_impl: checks, carve-up, the node encoder as encoder_route() of enc_route.cpp decided it, the steps).
// Post-processing and the one-call frame pipeline are mpn_post.hip, training (fused backward, layer-by-layer engine, device packer) is
// mpn_train.hip; every __global__ kernel is compiled in exactly one of the three, and the few that
// another unit launches too have host launchers (internal.h).
#include "forward_diag.cuh"
#include "wave_reduce.cuh"
#include "plan.cuh"
#include "encoder.cuh"
#include "enc_rows32.cuh"
#include "msg_bf16.cuh"
#include "step_general.cuh"
#include "step_fast.cuh"
#include "step_pipe.cuh"
#include "enc_f16.cuh"
#include "enc_f16_slices.cuh"
#include "generic_fused.cuh"
#include "generic.cuh"
#include "with_flag.h"

using namespace gnncca;

extern "C" {

#ifdef GNNCCA_STAMPS
__attribute__((visibility("default"))) int gnncca_debug_set_stamps(void* dev_buf) {
    unsigned long long* p = static_cast<unsigned long long*>(dev_buf);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &p, sizeof(p)));
    return GNNCCA_OK;
}
#endif

int gnncca_last_hip_error(void) { return g_last_hip_error; }

int gnncca_read_graph_flags(const void* workspace, uint32_t* flags_out, gnncca_stream_t stream) {
    if (!workspace || !flags_out) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(flags_out, workspace, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return GNNCCA_OK;
}

int gnncca_read_graph_flags2(const void* workspace, uint32_t flags_out[2], gnncca_stream_t stream) {
    if (!workspace || !flags_out) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(flags_out, workspace, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return GNNCCA_OK;
}

}  // extern "C"

static_assert(kEncSliceMaxK == kF16SlMaxKs, "encoder_route() sizes the slices of enc_f16_slices.cuh");

// The regions of the forward's workspace (carve(): internal.h) as pointers.
struct FwdBuffers {
    char* base;
    unsigned *flags, *blockflags;
    int *seg_ptr, *col32, *perm, *cursor;
    float *h0, *act, *part, *pd[2], *psq[2], *e, *e0;
};
static FwdBuffers carve_pointers(void* workspace, const Workspace& ws) {
    char* base = static_cast<char*>(workspace);
    auto f = [base](size_t off) { return reinterpret_cast<float*>(base + off); };
    auto i = [base](size_t off) { return reinterpret_cast<int*>(base + off); };
    auto u = [base](size_t off) { return reinterpret_cast<unsigned*>(base + off); };
    return FwdBuffers{base, u(ws.flags), u(ws.blockflags), i(ws.seg_ptr), i(ws.col32), i(ws.perm), i(ws.cursor), f(ws.h0), f(ws.act), f(ws.partial),
                      {f(ws.pd[0]), f(ws.pd[1])}, {f(ws.psq[0]), f(ws.psq[1])}, f(ws.e), f(ws.e0)};
}

// the second half of the graph plan (plan_finish / the repair of an unsorted graph), which EncFuseParams and TailParams both carry
template <class P>
static void fill_plan_finish(P& p, const FwdBuffers& b, const int64_t* edge_index, int E) {
    p.ei = reinterpret_cast<const long long*>(edge_index);
    p.seg_ptr = b.seg_ptr, p.col32 = b.col32, p.perm = b.perm, p.cursor = b.cursor, p.flags = b.flags, p.blockflags = b.blockflags;
    p.E = E;
}

// dynamic LDS beyond 64 KB of the big-batch GEMMs: once per device and thread (the attribute is per device)
static int enc_gemm_attributes() {
    static thread_local int attr_dev = -1;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (attr_dev == dev) return GNNCCA_OK;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_gemm_f16_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF16LdsBytes));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_gemm_f16_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF16LdsBytes));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_gemm_f16_rows32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF16R32LdsBytes));
    const void* fns[4] = {reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<false, false>),
                          reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<true, false>),
                          reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<false, true>),
                          reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<true, true>)};
    for (const void* fn : fns) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsGemmBytes));
    attr_dev = dev;
    return GNNCCA_OK;
}

// The node encoder as encoder_route() (enc_route.cpp) decided it: fills parameter structs and launches, compares no sizes.  Per GEMM
// layer: [plan launch in front of a fused GEMM] GEMM [plan launch behind an un-fused 256-row GEMM] [reduce, when another GEMM follows];
// then the tail, unless the GEMM's epilogue was it.
static int launch_node_encoder(const EncRoute& r, const gnncca_mpn_dims* d, const BlobHeader& hdr, const float* blob, const float* x,
                               const int64_t* edge_index, int N, int E, int ell_S, const FwdBuffers& b, float* trace_h, const DropCfg& drop,
                               hipStream_t st, Profiler* prof) {
    const int nl = d->enc_node.n_layers;
    // what the plan blocks read, wherever they run (the riding forms and plan_only_kernel read nothing else of EncPlanParams)
    EncPlanParams pl;
    std::memset(&pl, 0, sizeof(pl));
    if (r.plan_place != kPlanNone) {
        pl.ei = reinterpret_cast<const long long*>(edge_index);
        pl.seg_ptr = b.seg_ptr, pl.col32 = b.col32, pl.blockflags = b.blockflags;
        pl.E = E, pl.N = N, pl.ell_S = ell_S, pl.plan_span = r.plan_span;
    }
    const int ride = r.plan_place == kPlanRides ? r.plan_wgs : 0;   // plan workgroups behind the first GEMM's tiles
    const float* cur_in = x;
    for (int g = 0; g < r.n_gemm; ++g) {
        const EncGemmRoute& q = r.gemm[g];
        const gnncca_layer& l = d->enc_node.layers[g];
        const int K = q.K, O = q.O;
        if (q.form == kEncPlanGemm) {
            EncPlanParams ep = g == 0 ? pl : EncPlanParams{};
            ep.in = cur_in, ep.W = blob + hdr.enc_node_w[g], ep.part = b.part;
            ep.M = N, ep.K = K, ep.O = O, ep.kslice = q.kslice, ep.vec_ok = q.vec_ok;
            ep.nrt = (N + 31) / 32, ep.nks = q.slabs, ep.gemm_blocks = ep.nrt * q.slabs * ((O + 127) / 128);
            GNNCCA_LAUNCH(enc_gemm_plan_kernel, dim3(ep.gemm_blocks + (g == 0 ? ride : 0)), dim3(256), 0, st, ep);
        } else if (q.form == kEncSlices) {
            EncF16SlicesParams s;
            std::memset(&s, 0, sizeof(s));
            s.x = cur_in;
            s.w2h = reinterpret_cast<const unsigned short*>(blob + hdr.enc_w2h);
            s.w_bad = reinterpret_cast<const unsigned*>(blob + hdr.enc_w2h_bad);
            s.w32 = blob + hdr.enc_node_w[0];
            s.part = b.part;
            s.M = N, s.K = K, s.nrt = (N + 31) / 32, s.nks = q.slabs, s.Ks = q.kslice;
            s.force_arm = r.force_arm;   // (here: every wave on the fp32 arm)
            const dim3 sgrid((unsigned)(s.nrt * s.nks + ride));
            if (s.Ks == 256)
                GNNCCA_LAUNCH(enc_gemm_f16_slices8_kernel, sgrid, dim3(kF16SlThreads), 0, st, s, pl);
            else if (s.Ks == 128)
                GNNCCA_LAUNCH(enc_gemm_f16_slices4_kernel, sgrid, dim3(kF16SlThreads), 0, st, s, pl);
            else
                GNNCCA_LAUNCH(enc_gemm_f16_slices2_kernel, sgrid, dim3(kF16SlThreads), 0, st, s, pl);
        } else {   // big batches: the split-bf16 / fp16-split MFMA GEMMs
            const unsigned short* w3 = reinterpret_cast<const unsigned short*>(blob + hdr.enc_w3);
            // k rotation of the big-batch GEMMs (every workgroup starting its walk over k at another chunk): NOT done (round 5 measured it and
            // the code is gone).  A bare streaming loop of this access shape gains 20 % from it (tools/ubench_xring.hip: 5.0 -> 6.2 TB/s), the kernels themselves 0-3 % at N = 65 536 and LOSE 4 % at 32 768 (their waves are
            // not in lockstep across CUs the way the microbenchmark's are; profiles/r05_logs/ab_krot{1,2}.log) -- and it makes a node's encoder
            // output depend on WHICH row block of the batch it sits in (the summation starts elsewhere), which the un-rotated kernels do not
            // (tests/test_gpu_fuzz.py: 512 copies of one graph, bitwise).
            EncFuseParams fp;
            std::memset(&fp, 0, sizeof(fp));
            if (r.fused) {
                fp.b1 = blob + hdr.enc_node_b[0], fp.W2 = blob + hdr.enc_node_w[1], fp.b2 = blob + hdr.enc_node_b[1];
                fp.projwT = blob + hdr.proj_wT, fp.projb = blob + hdr.proj_b;
                fp.h0 = b.h0, fp.trace_h = trace_h, fp.pd_out = b.pd[0], fp.psq_out = b.psq[0];
                fp.relu_prev = l.relu;
                fill_plan_finish(fp, b, edge_index, E);
            }
            if (r.plan_place == kPlanBefore) {
                GNNCCA_LAUNCH(plan_only_kernel, dim3(r.plan_wgs), dim3(256), 0, st, pl);
                HIP_TRY(hipGetLastError());
                PROF_MARK(GNNCCA_K_PLAN_ROWS);
            }
            int s = enc_gemm_attributes();
            if (s != GNNCCA_OK) return s;
            EncF16Params f;   // the two fp16-split forms (enc_f16.cuh): three piece products, x and W by LDS-DMA rings
            std::memset(&f, 0, sizeof(f));
            f.x = cur_in;
            f.w2h = reinterpret_cast<const unsigned short*>(blob + hdr.enc_w2h);
            f.w_bad = reinterpret_cast<const unsigned*>(blob + hdr.enc_w2h_bad);
            f.w3 = w3;
            f.out = q.form == kEncLdsF16 ? b.part : nullptr;
            f.M = N, f.K = K, f.kslice = q.kslice;
            f.force_arm = r.force_arm;   // (every tile on the bf16 arm)
            f.x_nt = r.x_nt;
            // (Round 4 measured a 64-ROW split-K tiling for the mid-size batches -- 128 row blocks at 8192 nodes, split-K 4, two 64-KB-LDS
            // workgroups per CU, half the slabs: correct, and slower at every size: 32.1 vs 27.8 us at N = 8192 with a 7.0 instead of 9.3 us
            // tail, 59 vs 46 at 16 384, 129 vs 96 at 32 768 -- 4x the W traffic from L2 and one accumulation chain per wave; the kernel and
            // the log are kept under profiles/r04_logs/: enc_rows64.cuh.txt, ab_enc64_1.log.)
            const dim3 rgrid((unsigned)((N + 31) / 32) + 1);                                       // 32-row forms: + the plan workgroup
            const dim3 lgrid = r.fused ? dim3((N + 255) / 256 + 1, 1) : dim3((N + 255) / 256, q.slabs);   // 256-row forms: same, or split-K
            if (q.form == kEncR32F16) {
                GNNCCA_LAUNCH(enc_gemm_f16_rows32_kernel, rgrid, dim3(kF16R32Threads), kF16R32LdsBytes, st, f, fp);
            } else if (q.form == kEncR32Bf16) {
                with_flag(q.nst == 8, [&](auto N8) { with_flag(r.split3, [&](auto S3) {
                    GNNCCA_LAUNCH((enc_gemm_rows32_fused_kernel<S3(), N8() ? 8 : 4>), rgrid, dim3(256), 0, st, cur_in, w3, N, K, fp);
                }); });
            } else if (q.form == kEncLdsF16) {
                if (r.fused)
                    GNNCCA_LAUNCH(enc_gemm_f16_fused_kernel, lgrid, dim3(512), kF16LdsBytes, st, f, fp);
                else
                    GNNCCA_LAUNCH(enc_gemm_f16_split_kernel, lgrid, dim3(512), kF16LdsBytes, st, f, fp);
            } else if (q.form == kEncLdsBf16) {
                with_flag(r.fused, [&](auto FU) { with_flag(r.split3, [&](auto S3) {
                    GNNCCA_LAUNCH((enc_gemm_split_lds_kernel<FU(), S3()>), lgrid, dim3(512), kLdsGemmBytes, st, cur_in, w3, b.part, N, K, O, q.kslice, fp);
                }); });
            } else {   // kEncD128
                const int rb = (N + 127) / 128;
                with_flag(r.split3, [&](auto S3) {
                    GNNCCA_LAUNCH(enc_gemm_split_direct_kernel<S3()>, dim3((unsigned)(rb * q.slabs + ride)), dim3(256), 0, st, cur_in, w3, b.part, N, K, O,
                                  q.kslice, rb, q.slabs, pl);
                });
            }
        }
        HIP_TRY(hipGetLastError());
        PROF_MARK(GNNCCA_K_ENC_GEMM);
        if (g == 0 && r.plan_place == kPlanAfter) {   // several blocks per workgroup (plan_span)
            GNNCCA_LAUNCH(plan_only_kernel, dim3(r.plan_wgs), dim3(256), 0, st, pl);
            HIP_TRY(hipGetLastError());
            PROF_MARK(GNNCCA_K_PLAN_ROWS);
        }
        if (g < r.n_gemm - 1) {   // sums the slabs the GEMM above wrote; the rest of the slab region holds what an earlier forward left
            float* dst = b.act + (size_t)(g & 1) * N * O;
            GNNCCA_LAUNCH(reduce_bias_act_kernel, grid1((size_t)N * O, 256), dim3(256), 0, st, (const float*)b.part, blob + hdr.enc_node_b[g], dst, N, O,
                          q.slabs, l.relu);
            HIP_TRY(hipGetLastError());
            PROF_MARK(GNNCCA_K_ENC_REDUCE);
            cur_in = dst;
        }
    }
    if (r.tail == kTailNone) return GNNCCA_OK;   // h0, the projections and the plan's flag word all came out of the GEMM launch
    if (r.tail == kTailRefused) return GNNCCA_ERR_UNSUPPORTED;
    const gnncca_layer& lprev = d->enc_node.layers[r.n_gemm - 1];
    TailParams tp;
    std::memset(&tp, 0, sizeof(tp));
    tp.blob = blob, tp.part = b.part;
    tp.h0 = b.h0, tp.trace_h = trace_h, tp.pd_out = b.pd[0], tp.psq_out = b.psq[0];
    tp.off_prev_b = hdr.enc_node_b[r.n_gemm - 1], tp.off_lastWT = hdr.enc_last_wT, tp.off_last_b = hdr.enc_node_b[nl - 1];
    tp.off_projwT = hdr.proj_wT, tp.off_projb = hdr.proj_b;
    tp.ks = r.gemm[r.n_gemm - 1].slabs;   // the slabs the last GEMM wrote
    tp.F = lprev.out_dim, tp.N = N, tp.has_last = nl >= 2, tp.relu_prev = lprev.relu;
    tp.reatt_n = d->reattach_nodes, tp.hin = (d->reattach_nodes ? 2 : 1) * kH, tp.vec_reduce = r.tail_vec;
    fill_plan_finish(tp, b, edge_index, E);
    tp.drop = drop;
    auto blocks = [N](int per_wg) { return dim3((unsigned)std::min<size_t>(((size_t)N + per_wg - 1) / per_wg, 2048) + 1); };   // + plan-repair workgroup
    if (r.tail == kTailFast) {
        tp.npw = r.tail_npw;
        GNNCCA_LAUNCH(enc_tail_fast_kernel, blocks(tp.npw), dim3(256), 0, st, tp);
    } else if (r.tail == kTailMfma) {
        GNNCCA_LAUNCH(enc_tail_mfma_kernel, dim3((unsigned)((N + 31) / 32) + 1), dim3(256), 0, st, tp, blob + hdr.enc_node_w[nl - 1]);
    } else {
        if (r.tail_lds > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)r.tail_lds));
        GNNCCA_LAUNCH(enc_tail_kernel, blocks(4), dim3(256), r.tail_lds, st, tp);
    }
    HIP_TRY(hipGetLastError());
    PROF_MARK(GNNCCA_K_ENC_TAIL);
    return GNNCCA_OK;
}

// The message steps' set-up: everything of StepParams that does not change from step to step, and the nodes-per-wave of step 1 / of
// the later steps (step_pipe.cuh: NPW).
struct StepSetup {
    StepParams sp;
    int npw_first, npw_later;
};
static StepSetup step_setup(const gnncca_mpn_dims* d, const BlobHeader& hdr, const Workspace& ws, const FwdBuffers& b, const float* blob,
                            const float* edge_attr, int N, int E, uint32_t options, bool use_ell, const DropCfg& drop) {
    const int L = d->num_enc_steps;
    const long long avg_deg = (E + (long long)N - 1) / N;
    const int chunks = (int)((avg_deg + 63) / 64);
    StepSetup out;
    StepParams& sp = out.sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.blob = blob;
    sp.seg_ptr = b.seg_ptr;
    sp.col32 = b.col32;
    sp.perm = b.perm;
    sp.flags = b.flags;
    sp.edge_attr = edge_attr;
    sp.e = b.e;
    sp.e0 = b.e0;
    sp.h0 = b.h0;
    sp.e_stride = ws.e_stride;
    sp.off_wee = hdr.wee;
    sp.off_wneb = hdr.wne_b;
    sp.off_projwT = hdr.proj_wT;
    sp.off_projb = hdr.proj_b;
    sp.off_encw = hdr.enc_edge_w;
    sp.off_encb = hdr.enc_edge_b;
    sp.off_cw1 = hdr.cls_w1;
    sp.off_cb1 = hdr.cls_b1;
    sp.off_cw2 = hdr.cls_w2;
    sp.off_cb2 = hdr.cls_b2;
    sp.off_fast = hdr.fast_consts;
    sp.off_wnebf = hdr.wne_bf16;
    // which arithmetic the node message uses (StepParams::msg_f32): the traced (general) and the fast kernels follow ONE rule
    sp.msg_f32 = (N <= 512 || !step_pipe_fits(N, E, ws.e_stride, ws.total)) ? 1 : 0;
    sp.cls_hidden = hdr.cls_hidden;
    sp.N = N;
    sp.E = E;
    sp.edge_in = d->edge_in;
    sp.attr_vec = d->edge_in == 4 && (reinterpret_cast<uintptr_t>(edge_attr) & 15) == 0;
    sp.agg = d->agg;
    sp.reatt_n = d->reattach_nodes;
    // waves per source-node segment: split a segment over 2 or 4 waves only while that is needed to put ~4 waves on
    // every SIMD (small graphs are latency-bound); big batches keep one wave per node, which amortises the
    // per-node prologue / projection epilogue over all of the node's chunks
    {
        // waves per node that would fill the chip; graphs whose nodes average >= 32 chunks (degree ~2000+) get four times that: the
        // tail of a launch is then a few long segments (dense3000: 0.4315 -> 0.4039 ms with four waves per node, dense2048 equal;
        // profiles/r03_logs/r3_wps1.log)
        const long long want = (chunks >= 32 ? 16384 : 4096) / (long long)N;
        int wps = chunks >= 4 ? 4 : (chunks >= 2 ? 2 : 1);
        while (wps > 1 && wps > want) wps >>= 1;
        // GNNCCA_OPT_ENC_UNSPLIT promises logits that do not depend on the batch around a graph for batches of >= 4096 nodes: the
        // cross-wave combine sums in another order with another wave count, and `want` above depends on N (a shard of 2 x dense2048
        // would get four waves per node, the union of 8 one), so the option pins one wave per node there, the rule of every round
        // before the four-wave one (tests/test_gpu_sharded.py: dense2048 shard against its union, bitwise)
        if ((options & GNNCCA_OPT_ENC_UNSPLIT) != 0 && N >= 4096) wps = 1;
        static const int force_wps = diag_env_int("GNNCCA_WPS", 0, 1, 4);  // diagnostics
        if (force_wps == 1 || force_wps == 2 || force_wps == 4) wps = std::min(force_wps, chunks >= 4 ? 4 : (chunks >= 2 ? 2 : 1));
        sp.wps = wps;
        // two nodes per wave (step_pipe.cuh: NPW): batches whose nodes average one round (<= 128 edges) and that still fill the chip with
        // half as many waves
        static const int force_npw = diag_env_int("GNNCCA_NPW", 0, 1, 2);   // diagnostics: 1 / 2 = never / whenever eligible
        // thresholds: from 16 384 nodes (step 1 at 8192: 14.9 -> 15.7 us; at 16 384: 29.8 -> 28.2).  The later steps alone from 8192 nodes, with
        // the classification deferred, move 64 x dense128 from 17.2 / 15.3 / 6.4 to 14.5 / 14.6 / 8.9 us per step: a tie per forward
        // (profiles/r04_logs/ab_npw{6,7}.log), so one threshold serves both
        static const int npw_min_n = diag_env_int("GNNCCA_NPW_MIN_N", 16384, 0, 0x7FFFFFFF);
        static const int npw_min_n_first = diag_env_int("GNNCCA_NPW_MIN_N_FIRST", 16384, 0, 0x7FFFFFFF);
        out.npw_later = (wps == 1 && chunks <= 2 && (force_npw == 2 || (force_npw == 0 && N >= npw_min_n))) ? 2 : 1;
        out.npw_first = (out.npw_later == 2 && (force_npw == 2 || N >= npw_min_n_first)) ? 2 : 1;
        sp.npw = out.npw_later;
    }
    sp.hin = (d->reattach_nodes ? 2 : 1) * kH;
    // column ranges instead of the col32 stream on steps 2 ... L of the specialised kernels (StepParams::rng)
    sp.rng = (L >= 2 && (options & GNNCCA_OPT_COLUMN_RANGES) != 0) ? reinterpret_cast<int*>(b.base + ws.rng) : nullptr;
    sp.ws_base = b.base;
    sp.ws_bytes = ws.total;
    sp.so_e = (unsigned)ws.e, sp.so_col = (unsigned)ws.col32, sp.so_perm = (unsigned)ws.perm;
    // The P_dst gather table staged whole in LDS: OFF by default since round 4.  Rounds 1-2 staged it for every N <= 1024; round 3 found
    // gathers straight from L2 ahead below 801 nodes (dense32 ... dense768 -1.3 ... -4 % per forward, r3_pdlds2.log, r3_pdlds3.log) and
    // kept it for 801 ... 1024; with four waves per node and the kernels as they are now the table loses there as well -- dense1024,
    // L = 8 (BASELINE config 5): 120.4 -> 118.3 us per forward with the fp32 edge state, 112.8 -> 110.1 with bf16
    // (profiles/r04_logs/ab_config5.log; with ONE wave per node the table still wins, 141 vs 151 us, but that form is slower anyway).
    // The switches keep the variant reachable for A/B runs: GNNCCA_PD_LDS_MIN / _MAX name the node range that stages it.
    static const int pd_lds_max = diag_env_int("GNNCCA_PD_LDS_MAX", 1024, 0, 1024);   // diagnostics
    static const int pd_lds_min = diag_env_int("GNNCCA_PD_LDS_MIN", 0x7FFFFFFF, 0, 0x7FFFFFFF);
    sp.pd_lds = (N >= pd_lds_min && N <= pd_lds_max) && d->num_enc_steps > 0;
    sp.e_bf16 = (options & GNNCCA_OPT_EDGE_STATE_BF16) != 0;  // honoured by the specialised kernels only
    sp.ell_S = use_ell ? ws.ell_S : 0;
    sp.drop = drop;
    {
        const double state_bytes = (double)(sp.e_bf16 ? kEF / 2 : kEF) * (double)ws.e_stride * 4.0;
        sp.nt_store = state_bytes > 150e6;
        sp.nt_load = state_bytes > 256e6;
        static const int force_nt = diag_env_int("GNNCCA_STEP_NT", -1, -1, 2);   // diagnostics: 0 / 1 / 2 = default policy / nt stores / nt loads too
        if (force_nt >= 0) sp.nt_store = force_nt >= 1, sp.nt_load = force_nt >= 2;
    }
    return out;
}

static int forward_impl(const gnncca_mpn_dims* d, const void* packed_dev, const float* x, const int64_t* edge_index,
                        const float* edge_attr, int64_t n_nodes, int64_t n_edges, void* workspace, size_t workspace_bytes,
                        float* logits_out, const gnncca_trace* trace, gnncca_stream_t stream, Profiler* prof,
                        uint32_t options, const gnncca_dropout* dropout = nullptr) {
    if (!dims_valid(d) || n_nodes < 0 || n_edges < 0) return GNNCCA_ERR_INVALID_ARG;
    const Family fam = classify(d);
    if (fam == kFamilyNone) return GNNCCA_ERR_UNSUPPORTED;
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    if (n_nodes == 0) return n_edges == 0 ? GNNCCA_OK : GNNCCA_ERR_INVALID_ARG;
    if (!packed_dev || !x || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!edge_index || !edge_attr || !logits_out)) return GNNCCA_ERR_INVALID_ARG;
    DropCfg drop;
    std::memset(&drop, 0, sizeof(drop));
    if (dropout && (dropout->p_enc > 0.f || dropout->p_edge > 0.f || dropout->p_node > 0.f || dropout->p_cls > 0.f)) {
        // train-mode Dropout lives in the general (traced) kernels of the MFMA family only
        if (fam != kFamilyMfma32x6 || !trace || !trace->h_enc || !trace->e_enc || !trace->h_steps || !trace->e_steps ||
            !dropout->seed_dev || d->enc_node.n_layers != 2)
            return fam == kFamilyMfma32x6 ? GNNCCA_ERR_INVALID_ARG : GNNCCA_ERR_UNSUPPORTED;
        const float ps[4] = {dropout->p_enc, dropout->p_edge, dropout->p_node, dropout->p_cls};
        for (float q : ps)
            if (!(q >= 0.f && q < 1.f)) return GNNCCA_ERR_INVALID_ARG;
        drop.p_enc = dropout->p_enc, drop.p_edge = dropout->p_edge, drop.p_node = dropout->p_node, drop.p_cls = dropout->p_cls;
        drop.seed = reinterpret_cast<const unsigned long long*>(dropout->seed_dev);
    }
    const bool dropping = drop.seed != nullptr;
    if (fam == kFamilyGeneric)
        return forward_generic(d, packed_dev, x, edge_index, edge_attr, n_nodes, n_edges, workspace, workspace_bytes,
                               logits_out, trace, static_cast<hipStream_t>(stream));
    const Workspace ws = carve(d, n_nodes, n_edges);
    if (workspace_bytes < ws.total) return GNNCCA_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_nodes, E = (int)n_edges;
    const float* blob = static_cast<const float*>(packed_dev);
    // The blob header is a pure function of dims: recompute it on the host instead of reading it back.
    BlobHeader hdr;
    if (!blob_header(d, &hdr)) return GNNCCA_ERR_UNSUPPORTED;
    const FwdBuffers b = carve_pointers(workspace, ws);
    auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };

    // big, nearly regular batches keep the edge state in the padded layout (StepParams::ell_S); the decision is a pure
    // function of (dims, N, E) made in carve(); the plan validates the degrees against it on the device
    const bool use_ell = ws.ell_S > 0 && hdr.fast_consts != 0 && d->edge_in == 4 && !trace && d->agg != GNNCCA_AGG_MAX && aligned16(edge_attr) && E > 0;

    // ---- node encoder: the route decided once (enc_route.cpp), then launched ---------------------------------------
    float* trace_h = trace ? trace->h_enc : nullptr;
    const EncRouteIn rin{d, &hdr, &ws, N, E, options, dropping, trace_h != nullptr, aligned16(x), aligned16(workspace),
                         E > 0 ? plan_num_blocks(E) : 0, E > 0 ? plan_span(edge_index, E) : 0};
    const EncRoute route = encoder_route(rin, enc_tuning());
    int s = launch_node_encoder(route, d, hdr, blob, x, edge_index, N, E, use_ell ? ws.ell_S : 0, b, trace_h, drop, st, prof);
    if (s != GNNCCA_OK || E == 0) return s;

    // ---- message passing steps ----------------------------------------------------------------------------
    const int L = d->num_enc_steps;
    const int first_cls = L - d->num_class_steps + 1;  // models/mpn.py:277
    StepSetup setup = step_setup(d, hdr, ws, b, blob, edge_attr, N, E, options, use_ell, drop);
    StepParams& sp = setup.sp;
    const int npw_first = setup.npw_first, npw_later = setup.npw_later;
    const bool re = d->reattach_edges != 0;
    int out_idx = 0;
    if (L == 0) {  // models/mpn.py:295-297: classify the encoded edge features once
        sp.first = 1;
        sp.update = 0;
        sp.cls_layers = hdr.cls_layers;
        sp.logits = logits_out;
        sp.trace_e_enc = trace ? trace->e_enc : nullptr;
        HIP_TRY(re ? (launch_step<true, false>(sp, st)) : (launch_step<false, false>(sp, st)));
        PROF_MARK(GNNCCA_K_STEP_LAST);
        return GNNCCA_OK;
    }
    // DEFERRED classification (step_pipe.cuh: CIN): a message step that produces a classified state does not classify it; the step that reads
    // the state back does (the last step: its input and its output).  The classifying message steps then run the variant without the
    // classifier -- lighter, and eligible for two nodes per wave.  Where it pays: forwards whose message steps run two nodes per wave
    // (sp.npw == 2); fp32 edge state only (the bf16 state is rounded after its step classified it); logits bit for bit the same.
    const bool can_defer = hdr.fast_consts != 0 && sp.attr_vec && !trace && d->agg != GNNCCA_AGG_MAX && !sp.msg_f32 && !sp.e_bf16 && !sp.pd_lds &&
                           sp.rng == nullptr && first_cls < L && !dropping;
    const bool defer = can_defer && npw_later == 2;
    for (int step = 1; step <= L; ++step) {
        const bool want_h = trace && trace->h_steps;
        const bool msg = step < L || want_h;
        sp.first = step == 1;
        sp.npw = step == 1 ? npw_first : npw_later;
        sp.step_no = step;
        sp.cls_no = out_idx;
        sp.stamp_slot = 2 + (step - 1 < 6 ? step - 1 : 5);
        sp.update = 1;
        sp.store_e = step < L;
        if (defer) {   // slot of step s: s - first_cls
            sp.cls_layers = step == L ? hdr.cls_layers : 0;
            sp.logits = step == L ? logits_out + (size_t)(L - first_cls) * E : nullptr;
            sp.logits_in = step - 1 >= first_cls ? logits_out + (size_t)(step - 1 - first_cls) * E : nullptr;
        } else {
            sp.cls_layers = step >= first_cls ? hdr.cls_layers : 0;
            sp.logits = step >= first_cls ? logits_out + (size_t)(out_idx++) * E : nullptr;
            sp.logits_in = nullptr;
        }
        sp.pd_in = b.pd[(step - 1) & 1];
        sp.so_pd = (unsigned)ws.pd[(step - 1) & 1];
        sp.psq_in = b.psq[(step - 1) & 1];
        sp.pd_out = step < L ? b.pd[step & 1] : nullptr;
        sp.psq_out = step < L ? b.psq[step & 1] : nullptr;
        sp.trace_e_enc = (trace && step == 1) ? trace->e_enc : nullptr;
        sp.trace_e = (trace && trace->e_steps) ? trace->e_steps + (size_t)(step - 1) * E * kEF : nullptr;
        sp.trace_h = want_h ? trace->h_steps + (size_t)(step - 1) * N * kH : nullptr;
        hipError_t err;
        const bool fast = hdr.fast_consts != 0 && sp.attr_vec && !trace && d->agg != GNNCCA_AGG_MAX;
        sp.diag = 0;   // nothing sets its bits any more; the step kernels keep the field for their register allocation (StepParams::diag)
        const bool pipe_ok = fast && !sp.msg_f32;
        if (pipe_ok)
            err = launch_pipe_dispatch(sp, msg, st);
        else if (fast)
            err = launch_fast_dispatch(sp, msg, st);
        else if (re)
            err = msg ? launch_step<true, true>(sp, st) : launch_step<true, false>(sp, st);
        else
            err = msg ? launch_step<false, true>(sp, st) : launch_step<false, false>(sp, st);
        HIP_TRY(err);
        PROF_MARK(msg ? GNNCCA_K_STEP : GNNCCA_K_STEP_LAST);
    }
    return GNNCCA_OK;
}

extern "C" {

int gnncca_mpn_forward(const gnncca_mpn_dims* d, const void* packed_dev, const float* x, const int64_t* edge_index,
                       const float* edge_attr, int64_t n_nodes, int64_t n_edges, void* workspace, size_t workspace_bytes,
                       float* logits_out, const gnncca_trace* trace, gnncca_stream_t stream) {
    return forward_impl(d, packed_dev, x, edge_index, edge_attr, n_nodes, n_edges, workspace, workspace_bytes, logits_out,
                        trace, stream, nullptr, 0u);
}

int gnncca_mpn_forward_ex(const gnncca_mpn_dims* d, const void* packed_dev, const float* x, const int64_t* edge_index,
                          const float* edge_attr, int64_t n_nodes, int64_t n_edges, void* workspace, size_t workspace_bytes,
                          float* logits_out, const gnncca_trace* trace, uint32_t options, gnncca_stream_t stream) {
    return forward_impl(d, packed_dev, x, edge_index, edge_attr, n_nodes, n_edges, workspace, workspace_bytes, logits_out,
                        trace, stream, nullptr, options);
}

int gnncca_mpn_forward_train(const gnncca_mpn_dims* d, const void* packed_dev, const float* x, const int64_t* edge_index,
                             const float* edge_attr, int64_t n_nodes, int64_t n_edges, void* workspace, size_t workspace_bytes,
                             float* logits_out, const gnncca_trace* trace, const gnncca_dropout* dropout, gnncca_stream_t stream) {
    return forward_impl(d, packed_dev, x, edge_index, edge_attr, n_nodes, n_edges, workspace, workspace_bytes, logits_out,
                        trace, stream, nullptr, 0u, dropout);
}

int gnncca_mpn_forward_profiled(const gnncca_mpn_dims* d, const void* packed_dev, const float* x,
                                const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                                void* workspace, size_t workspace_bytes, float* logits_out, gnncca_stream_t stream,
                                gnncca_profile* profile) {
    if (!profile) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Profiler p;
    p.out = profile;
    profile->count = 0;
    int s = prof_begin(&p);
    if (s != GNNCCA_OK) return s;
    s = forward_impl(d, packed_dev, x, edge_index, edge_attr, n_nodes, n_edges, workspace, workspace_bytes, logits_out,
                     nullptr, stream, &p, profile->options);
    const int s2 = prof_end(&p, st);
    return s != GNNCCA_OK ? s : s2;
}

}  // extern "C"
