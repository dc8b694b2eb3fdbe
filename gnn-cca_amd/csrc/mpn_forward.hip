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
// and the forward itself (forward_impl: checks, carve-up, the node encoder as encoder_route() of enc_route.cpp decided it, every step as
// step_plan() / step_launch() of step_route.cpp named it: launch_step_variant).
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

// The message steps' set-up: everything of StepParams that does not change from step to step, the decided part from the plan
// (step_route.cpp).  Every field is filled whichever kernel the steps run on, also where that kernel ignores it.
static StepParams step_setup(const StepPlan& plan, const gnncca_mpn_dims* d, const BlobHeader& hdr, const Workspace& ws, const FwdBuffers& b,
                             const float* blob, const float* edge_attr, int N, int E, const DropCfg& drop) {
    StepParams sp;
    std::memset(&sp, 0, sizeof(sp));   // (diag stays 0: nothing sets its bits any more; the step kernels keep the field, StepParams::diag)
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
    sp.cls_hidden = hdr.cls_hidden;
    sp.N = N;
    sp.E = E;
    sp.edge_in = d->edge_in;
    sp.agg = d->agg;
    sp.reatt_n = d->reattach_nodes;
    sp.hin = plan.hin;
    sp.msg_f32 = plan.msg_f32;
    sp.attr_vec = plan.attr_vec;
    sp.wps = plan.wps;
    sp.npw = plan.npw_later;
    sp.pd_lds = plan.pd_lds;
    sp.e_bf16 = plan.e_bf16;
    sp.ell_S = plan.ell_S;
    sp.nt_store = plan.nt >= 1, sp.nt_load = plan.nt >= 2;
    sp.rng = plan.ranges ? reinterpret_cast<int*>(b.base + ws.rng) : nullptr;
    sp.ws_base = b.base;
    sp.ws_bytes = ws.total;
    sp.so_e = (unsigned)ws.e, sp.so_col = (unsigned)ws.col32, sp.so_perm = (unsigned)ws.perm;
    sp.drop = drop;
    return sp;
}

// One step as step_launch() (step_route.cpp) named it: the ladders turn the run-time names into template arguments, `if constexpr` keeps
// them to the instantiations the library has (step_variant_exists: internal.h).  Compares no sizes; the grid and the LDS are the route's.
// A name the library does not have launches nothing and is hipErrorInvalidValue (step_launch never produces one: tests/test_step_route.py).
static hipError_t launch_step_variant(const StepLaunch& l, const StepParams& sp, hipStream_t st) {
    const dim3 grid(l.blocks), block(256);
    bool launched = false;
    auto with_nt = [&](auto&& f) {
        l.NT == 2 ? f(std::integral_constant<int, 2>{}) : l.NT == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
    };
    if (l.family == kStepGeneral) {
        with_flag(l.RE, [&](auto RE) { with_flag(l.MSG, [&](auto MSG) { with_flag(l.MX, [&](auto MX) {
            GNNCCA_LAUNCH((mpn_step_kernel<RE(), MSG(), MX()>), grid, block, l.lds, st, sp);
            launched = true;
        }); }); });
    } else {
        with_flag(l.FIRST, [&](auto FIRST) { with_flag(l.CLS, [&](auto CLS) { with_flag(l.MSG, [&](auto MSG) { with_flag(l.PDL, [&](auto PDL) {
        with_nt([&](auto NT) { with_flag(l.EB, [&](auto EB) {
            if (l.family == kStepFast) {
                if constexpr (step_variant_exists(kStepFast, FIRST(), CLS(), MSG(), PDL(), EB(), NT(), false, 1, false)) {
                    GNNCCA_LAUNCH((mpn_step_fast_kernel<FIRST(), CLS(), MSG(), PDL(), EB(), NT()>), grid, block, l.lds, st, sp);
                    launched = true;
                }
                return;
            }
            with_flag(l.RNG, [&](auto RNG) { with_flag(l.NPW == 2, [&](auto TWO) { with_flag(l.CIN, [&](auto CIN) {
                constexpr int NPW = TWO() ? 2 : 1;
                if constexpr (step_variant_exists(kStepPipe, FIRST(), CLS(), MSG(), PDL(), EB(), NT(), RNG(), NPW, CIN())) {
                    GNNCCA_LAUNCH((mpn_step_pipe_kernel<FIRST(), CLS(), MSG(), PDL(), EB(), NT(), RNG(), NPW, CIN()>), grid, block, l.lds, st, sp);
                    launched = true;
                }
            }); }); });
        }); });
        }); }); }); });
    }
    return launched ? hipGetLastError() : hipErrorInvalidValue;
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

    // ---- the routes: decided once (enc_route.cpp, step_route.cpp), then launched ----------------------------------
    float* trace_h = trace ? trace->h_enc : nullptr;
    const StepRouteIn sin{d, &hdr, &ws, N, E, options, dropping, trace != nullptr, trace && trace->h_steps, aligned16(edge_attr)};
    const StepPlan plan = step_plan(sin, step_tuning());
    const EncRouteIn rin{d, &hdr, &ws, N, E, options, dropping, trace_h != nullptr, aligned16(x), aligned16(workspace),
                         E > 0 ? plan_num_blocks(E) : 0, E > 0 ? plan_span(edge_index, E) : 0};
    const EncRoute route = encoder_route(rin, enc_tuning());
    int s = launch_node_encoder(route, d, hdr, blob, x, edge_index, N, E, plan.ell_S, b, trace_h, drop, st, prof);
    if (s != GNNCCA_OK || plan.launches == 0) return s;

    // ---- message passing steps (L == 0: one launch, step 0, that classifies the encoded edge features; models/mpn.py:295-297) ----
    StepParams sp = step_setup(plan, d, hdr, ws, b, blob, edge_attr, N, E, drop);
    for (int i = 0; i < plan.launches; ++i) {
        const int step = plan.L == 0 ? 0 : i + 1;
        const StepLaunch l = step_launch(plan, step);
        sp.first = l.first;
        sp.update = l.update;
        sp.store_e = l.store_e;
        sp.npw = l.npw;
        sp.step_no = step;
        sp.cls_no = l.cls_no;
        sp.stamp_slot = l.stamp_slot;
        sp.cls_layers = l.cls_layers;
        sp.logits = l.slot_out >= 0 ? logits_out + (size_t)l.slot_out * E : nullptr;
        sp.logits_in = l.slot_in >= 0 ? logits_out + (size_t)l.slot_in * E : nullptr;
        sp.pd_in = l.buf_in >= 0 ? b.pd[l.buf_in] : nullptr;
        sp.so_pd = l.buf_in >= 0 ? (unsigned)ws.pd[l.buf_in] : 0u;
        sp.psq_in = l.buf_in >= 0 ? b.psq[l.buf_in] : nullptr;
        sp.pd_out = l.buf_out >= 0 ? b.pd[l.buf_out] : nullptr;
        sp.psq_out = l.buf_out >= 0 ? b.psq[l.buf_out] : nullptr;
        sp.trace_e_enc = (trace && l.first) ? trace->e_enc : nullptr;
        sp.trace_e = (trace && trace->e_steps && l.update) ? trace->e_steps + (size_t)(step - 1) * E * kEF : nullptr;
        sp.trace_h = (plan.trace_h_steps && l.update) ? trace->h_steps + (size_t)(step - 1) * N * kH : nullptr;
        HIP_TRY(launch_step_variant(l, sp, st));
        PROF_MARK(l.MSG ? GNNCCA_K_STEP : GNNCCA_K_STEP_LAST);
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
