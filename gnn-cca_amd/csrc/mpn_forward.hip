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
// and the forward's route (forward_impl).  Post-processing and the one-call frame pipeline are mpn_post.hip, training (fused backward,
// layer-by-layer engine, device packer) is mpn_train.hip; every __global__ kernel is compiled in exactly one of the three, and the few that
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
    char* base = static_cast<char*>(workspace);
    const int N = (int)n_nodes, E = (int)n_edges;
    const float* blob = static_cast<const float*>(packed_dev);

    // The blob header is a pure function of dims: recompute it on the host instead of reading it back.
    BlobHeader hdr;
    if (!blob_header(d, &hdr)) return GNNCCA_ERR_UNSUPPORTED;

    unsigned* flags = reinterpret_cast<unsigned*>(base + ws.flags);
    int* seg_ptr = reinterpret_cast<int*>(base + ws.seg_ptr);
    int* col32 = reinterpret_cast<int*>(base + ws.col32);
    int* perm = reinterpret_cast<int*>(base + ws.perm);
    int* cursor = reinterpret_cast<int*>(base + ws.cursor);
    unsigned* blockflags = reinterpret_cast<unsigned*>(base + ws.blockflags);
    float* h0 = reinterpret_cast<float*>(base + ws.h0);
    float* act = reinterpret_cast<float*>(base + ws.act);
    float* part = reinterpret_cast<float*>(base + ws.partial);
    float* pd[2] = {reinterpret_cast<float*>(base + ws.pd[0]), reinterpret_cast<float*>(base + ws.pd[1])};
    float* psq[2] = {reinterpret_cast<float*>(base + ws.psq[0]), reinterpret_cast<float*>(base + ws.psq[1])};
    float* ebuf = reinterpret_cast<float*>(base + ws.e);
    float* e0buf = reinterpret_cast<float*>(base + ws.e0);

    // big, nearly regular batches keep the edge state in the padded layout (StepParams::ell_S); the decision is a pure
    // function of (dims, N, E) made in carve(); the plan validates the degrees against it on the device
    const bool use_ell = ws.ell_S > 0 && hdr.fast_consts != 0 && d->edge_in == 4 && !trace && d->agg != GNNCCA_AGG_MAX &&
                         (reinterpret_cast<uintptr_t>(edge_attr) & 15) == 0 && E > 0;
    // ---- node encoder -------------------------------------------------------------------------------------
    const int nl = d->enc_node.n_layers;
    const int n_gemm = nl == 1 ? 1 : nl - 1;
    const float* cur_in = x;
    int ks_last = 1;
    bool fused_tail = false;   // the GEMM launch already produced h0 and the step-1 projections
    const bool split3 = (options & GNNCCA_OPT_ENC_SPLIT3) != 0;
    const bool unsplit = (options & GNNCCA_OPT_ENC_UNSPLIT) != 0;
    // diagnostics, read once for every encoder form below: the bf16 form as the A/B reference of the fp16-split GEMMs; every tile / wave of
    // the fp16-split GEMMs on its fallback arm (tests)
    static const bool gemm_bf16 = diag_env("GNNCCA_GEMM_BF16") != nullptr;
    static const int f16_force_arm = diag_env_int("GNNCCA_GEMM_F16_ARM", 0, 0, 1);
    // graphs and batches whose GEMM ran split-K: the tail on the matrix pipe, 32 nodes per workgroup, from 2560 nodes (round 3 lowered this
    // from 6144: 8.7 -> 6.9 us at N = 4096, 10.3 -> 7.5 at 5120, 10.4 -> 7.0 at 4000, 9.2 -> 7.2 at 3000, 8.6 -> 6.4 at 3072; equal at 2048
    // (6.2), the register-resident tail ahead at 1024 (5.0 vs 7.6); profiles/r03_logs/r3_thresh1.log, r3_thresh2.log)
    static const int kTailMfmaMin = diag_env_int("GNNCCA_TAIL_MFMA_MIN", 2560, 0, 0x7FFFFFFF);   // diagnostics
    const bool tail_mfma_ok = !dropping && N >= kTailMfmaMin && nl == 2 && d->enc_node.layers[0].out_dim == 128 &&
                              !d->reattach_nodes && (reinterpret_cast<uintptr_t>(part) & 15) == 0;
    for (int g = 0; g < n_gemm; ++g) {
        const gnncca_layer& l = d->enc_node.layers[g];
        const int K = l.in_dim, O = l.out_dim;
        const int ks = g == 0 ? ws.ksplit : 1;
        int kslice = (K + ks - 1) / ks;
        kslice = (kslice + 63) / 64 * 64;
        // From 384 nodes on the first encoder layer runs on the split-bf16 MFMA GEMM, the plan riding in its launch.  (Round 3 lowered this
        // from 4096 to 1024 -- f32 MFMA GEMM + plan 19.5 us at dense1024, 43 at dense2048; 128-row split kernel + a plan launch 11.0 + 5.8
        // and 17.4 + 17.1, r3_gemm_split_min.log -- and, once the plan rode along, to 384: GEMM 11.5 / 12.1 / 17.7 / 20.8 -> 9.3 / 9.2 /
        // 10.5 / 13.2 us at 384 / 512 / 768 / 896 nodes, 3 x dense256 17.0 -> 10.0; at 256 nodes the f32 form stays ahead, 6.6 vs 7.6;
        // r3_split_min2.log)
        static const int split_min = diag_env_int("GNNCCA_GEMM_SPLIT_MIN", 384, 0, 0x7FFFFFFF);   // diagnostics
        // round 6: below 4096 nodes the first layer runs on the fp16-split GEMM in 32-row tiles with K split over one round of workgroups
        // (enc_f16_slices.cuh): a fraction of the slabs of the two forms above (dense1024: 8 x 0.5 MB instead of 16 x 0.5 MB written and read
        // back; dense256: 16 instead of 32) and half the matrix work of the six-product form.  nks: at least K / 256, then powers of two
        // while one round of workgroups holds the tiles (nrt * nks <= 256), a slice stays >= 64 deep and the workspace has the slabs.
        // The minimum K / 256 is taken even where nrt * nks exceeds one round (K = 2048 near N = 4095: 128 x 8 = 1024 workgroups).
        static const int slices_min = diag_env_int("GNNCCA_GEMM_SLICES_MIN", 1, 0, 0x7FFFFFFF);
        static const int slices_max = diag_env_int("GNNCCA_GEMM_SLICES_MAX", 4095, 0, 0x7FFFFFFF);
        const bool use_slices = g == 0 && hdr.enc_w2h != 0 && O == 128 && K >= 64 && (K & (K - 1)) == 0 && K / kF16SlMaxKs <= ws.ksplit && N >= slices_min && N <= slices_max && !split3 &&
                                !gemm_bf16 && !unsplit && (reinterpret_cast<uintptr_t>(cur_in) & 15) == 0;
        const bool split = !use_slices && g == 0 && hdr.enc_w3 != 0 && N >= split_min && (reinterpret_cast<uintptr_t>(cur_in) & 15) == 0;
        EncPlanParams ep;
        std::memset(&ep, 0, sizeof(ep));
        ep.in = cur_in;
        ep.W = blob + hdr.enc_node_w[g];
        ep.part = part;
        ep.M = N;
        ep.K = K;
        ep.O = O;
        ep.kslice = kslice;
        ep.vec_ok = (K % 4 == 0) && ((reinterpret_cast<uintptr_t>(cur_in) & 15) == 0);
        ep.nrt = (N + 31) / 32;
        ep.nks = ks;
        ep.gemm_blocks = split ? 0 : ep.nrt * ks * ((O + 127) / 128);
        int plan_blocks = 0;
        bool plan_launched = false;
        if (g == 0 && E > 0) {  // the graph plan rides in the first GEMM launch (small graphs) or gets its own (batches)
            ep.ei = reinterpret_cast<const long long*>(edge_index);
            ep.seg_ptr = seg_ptr;
            ep.col32 = col32;
            ep.blockflags = blockflags;
            ep.E = E;
            ep.N = N;
            ep.ell_S = use_ell ? ws.ell_S : 0;
            plan_blocks = plan_num_blocks(E);
        }
        int ks_split = 1;
        if (use_slices) {
            const int nrt = (N + 31) / 32;
            // slices: at least K / 256 (a workgroup's x tile is 32 KB of LDS), then powers of two while one round of workgroups holds the tiles, a
            // slice stays >= 64 deep and the workspace has the slabs (dense1024 -> 8, dense256 and below -> 16: 32 slices of 64 measured 0.7 us slower per dense256 forward, 8 of 256 1.4 us)
            static const int nks_cap = diag_env_int("GNNCCA_GEMM_SLICES_NKS", 16, 1, 32);       // diagnostics: cap of the slice count
            static const int wg_cap = diag_env_int("GNNCCA_GEMM_SLICES_WGS", 256, 1, 1 << 20);    // diagnostics: workgroups one round may hold
            int nks = 1;
            while (K / nks > kF16SlMaxKs) nks *= 2;
            while (nks * 2 <= std::min(nks_cap, ws.ksplit) && nrt * nks * 2 <= wg_cap && K / (nks * 2) >= 64 && (K / (nks * 2)) % 64 == 0) nks *= 2;
            EncF16SlicesParams q;
            std::memset(&q, 0, sizeof(q));
            q.x = cur_in;
            q.w2h = reinterpret_cast<const unsigned short*>(blob + hdr.enc_w2h);
            q.w_bad = reinterpret_cast<const unsigned*>(blob + hdr.enc_w2h_bad);
            q.w32 = blob + hdr.enc_node_w[0];
            q.part = part;
            q.M = N, q.K = K, q.nrt = nrt, q.nks = nks, q.Ks = K / nks;
            q.force_arm = f16_force_arm;   // (here: every wave on the fp32 arm)
            EncPlanParams pl = ep;
            int ride = 0;
            if (plan_blocks > 0) {   // the plan rides in this launch (extra workgroups beyond the GEMM tiles)
                pl.plan_span = plan_span(edge_index, E);
                ride = pl.plan_span > 1 ? (plan_blocks + pl.plan_span - 1) / pl.plan_span : plan_blocks;
                ride = (ride + 1) / 2;   // two plan blocks per 512-thread workgroup
            } else {
                pl.E = 0;
            }
            const dim3 sgrid((unsigned)(nrt * nks + ride));
            if (q.Ks == 256)
                GNNCCA_LAUNCH(enc_gemm_f16_slices8_kernel, sgrid, dim3(kF16SlThreads), 0, st, q, pl);
            else if (q.Ks == 128)
                GNNCCA_LAUNCH(enc_gemm_f16_slices4_kernel, sgrid, dim3(kF16SlThreads), 0, st, q, pl);
            else
                GNNCCA_LAUNCH(enc_gemm_f16_slices2_kernel, sgrid, dim3(kF16SlThreads), 0, st, q, pl);
            HIP_TRY(hipGetLastError());
            PROF_MARK(GNNCCA_K_ENC_GEMM);
            plan_launched = true;
            ep.gemm_blocks = 0;
            plan_blocks = 0;
            ks_split = nks;
        }
        if (split) {  // big batches: split-bf16 MFMA GEMM; the plan gets its own launch
            const unsigned short* w3 = reinterpret_cast<const unsigned short*>(blob + hdr.enc_w3);
            static const int lds_min = diag_env_int("GNNCCA_GEMM_LDS_MIN", 6144, 0, 0x7FFFFFFF);   // diagnostics
            const bool fusable = !dropping && nl == 2 && d->enc_node.layers[1].in_dim == 128 && d->enc_node.layers[1].out_dim == kH &&
                                 !d->reattach_nodes && hdr.proj_wT != 0;
            const bool use_lds = N >= lds_min && O == 128;
            if (use_lds) ks_split = std::min(enc_lds_ksplit(N, K), ws.ksplit);
            // mid-size batches, where the 256-row form would run split-K: 32-row workgroups, un-split, fused epilogue (enc_rows32.cuh)
            // GNNCCA_OPT_ENC_UNSPLIT: batches of >= 4096 nodes never split K -- where the 256-row form would, 32-row workgroups run
            // un-split with the same fused epilogue (enc_rows32.cuh), so a node's encoder output is bit for bit independent of the batch
            // around it (a shard of a sharded batch reproduces the union's logits exactly).  Not the default: one wave per SIMD at
            // N <= 8192 (N = 8192: 41-43.5 us against 28 + 9 for split-K + tail; enc_rows32.cuh says where the time goes)
            const bool use_r32 = unsplit && fusable && O == 128 && K % 256 == 0 && N >= 4096 &&
                                 !(use_lds && ks_split == 1);
            if (use_r32) ks_split = 1;
            // round 5: mid-size batches on the fp16-split form take 32-row workgroups that split K over their WAVES and finish the encoder in
            // the epilogue (enc_f16.cuh: enc_gemm_f16_rows32_kernel) -- no slabs, no tail launch.  Range: 4096 ... 8192 nodes, i.e. while the
            // row tiles fit ONE round of workgroups: every 32-row workgroup pulls all 1 MB of W through its CU's L2 path (~70 GB/s: 14 us), which
            // a second round doubles (plan + GEMM + tail, same box: 25.3 / 26.4 / 27.4 / 28.6 / 30.4 us at 4096 / 5120 / 6144 / 7168 / 8192 nodes
            // against 26.6 / 35.0 / 31.2 / 33.0 / 38.3 for the split-K forms; 47.4 against 39.2 at 9216; profiles/r05_logs/ab_r32f_2.log)
            static const int r32f_min = diag_env_int("GNNCCA_GEMM_R32F_MIN", 4096, 0, 0x7FFFFFFF);
            static const int r32f_max = diag_env_int("GNNCCA_GEMM_R32F_MAX", 8192, 0, 0x7FFFFFFF);
            const bool use_r32f = !use_r32 && fusable && O == 128 && K % 256 == 0 && hdr.enc_w2h != 0 && !split3 && !gemm_bf16 &&
                                  !unsplit && N >= r32f_min && N <= r32f_max && !(use_lds && ks_split == 1);
            if (use_r32f) ks_split = 1;
            // un-split and the shipped encoder shape (2048 -> 128 -> 32, no reattach): the rest of the encoder, the step-1
            // projections and the plan fold run in the GEMM's epilogue, on the tile while it is on chip
            fused_tail = (use_lds && fusable && ks_split == 1) || use_r32 || use_r32f;
            EncFuseParams fp;
            std::memset(&fp, 0, sizeof(fp));
            // k rotation of the big-batch GEMMs (every workgroup starting its walk over k at another chunk): NOT done (round 5 measured it and
            // the code is gone).  A bare streaming loop of this access shape gains 20 % from it (tools/ubench_xring.hip: 5.0 -> 6.2 TB/s), the kernels themselves 0-3 % at N = 65 536 and LOSE 4 % at 32 768 (their waves are
            // not in lockstep across CUs the way the microbenchmark's are; profiles/r05_logs/ab_krot{1,2}.log) -- and it makes a node's encoder
            // output depend on WHICH row block of the batch it sits in (the summation starts elsewhere), which the un-rotated kernels do not
            // (tests/test_gpu_fuzz.py: 512 copies of one graph, bitwise).
            if (fused_tail) {
                fp.b1 = blob + hdr.enc_node_b[0];
                fp.W2 = blob + hdr.enc_node_w[1];
                fp.b2 = blob + hdr.enc_node_b[1];
                fp.projwT = blob + hdr.proj_wT;
                fp.projb = blob + hdr.proj_b;
                fp.h0 = h0;
                fp.trace_h = trace ? trace->h_enc : nullptr;
                fp.pd_out = pd[0];
                fp.psq_out = psq[0];
                fp.relu_prev = l.relu;
                // the plan goes FIRST here, so that one extra workgroup of the GEMM launch can fold its findings (and repair
                // an unsorted graph): no tail launch is left in this regime
                fp.ei = reinterpret_cast<const long long*>(edge_index);
                fp.seg_ptr = seg_ptr;
                fp.col32 = col32;
                fp.perm = perm;
                fp.cursor = cursor;
                fp.flags = flags;
                fp.blockflags = blockflags;
                fp.E = E;
                if (plan_blocks > 0) {
                    ep.plan_span = plan_span(edge_index, E);
                    if (ep.plan_span > 1) plan_blocks = (plan_blocks + ep.plan_span - 1) / ep.plan_span;
                    GNNCCA_LAUNCH(plan_only_kernel, dim3(plan_blocks), dim3(256), 0, st, ep);
                    HIP_TRY(hipGetLastError());
                    PROF_MARK(GNNCCA_K_PLAN_ROWS);
                }
                plan_launched = true;
            }
            // The fp16-split form (enc_f16.cuh) is the default of the 256-row regime; the bf16 form stays for GNNCCA_OPT_ENC_UNSPLIT (whose
            // bitwise batch independence is stated on the bf16 arithmetic of all three un-split kernels), for GNNCCA_OPT_ENC_SPLIT3 (an option
            // of that form) and as the A/B reference (GNNCCA_GEMM_BF16).  K / ks_split is a multiple of 32 on this path.
            // x stream of the fp16-split GEMMs: NON-TEMPORAL from 128 MB of x on (N >= 16 384 at K = 2048).  Inside a real forward the caches are full
            // of what the previous forward's step kernels left (dirty edge state), and a default-policy x stream fights it for every line: BASELINE
            // config 4 in situ 174 -> 137 us for this launch (0.516 -> 0.485 ms per forward), while an encoder timed alone on clean caches hides
            // the difference (121 us either way); at the 8 192-node share the policy costs 1 us, so small batches keep the default
            // (profiles/r05_logs/ab_config4_nt.log).  GNNCCA_GEMM_F16_XNT = 0 / 1 forces it off / on.
            static const int f16_x_nt_force = diag_env_int("GNNCCA_GEMM_F16_XNT", -1, -1, 1);
            const int f16_x_nt = f16_x_nt_force >= 0 ? f16_x_nt_force : ((double)N * K * 4.0 >= 128.0 * 1024 * 1024 ? 1 : 0);
            const bool use_f16 = use_lds && !use_r32 && !use_r32f && hdr.enc_w2h != 0 && !split3 && !unsplit && !gemm_bf16 &&
                                 K % 32 == 0 && (K / ks_split) % 32 == 0;
            static thread_local int attr_dev = -1;  // once per device and thread: the attribute is per device
            int dev = 0;
            HIP_TRY(hipGetDevice(&dev));
            if (attr_dev != dev) {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_gemm_f16_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF16LdsBytes));
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_gemm_f16_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF16LdsBytes));
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_gemm_f16_rows32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kF16R32LdsBytes));
                const void* fns[4] = {reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<false, false>),
                                      reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<true, false>),
                                      reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<false, true>),
                                      reinterpret_cast<const void*>(enc_gemm_split_lds_kernel<true, true>)};
                for (const void* fn : fns)
                    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsGemmBytes));
                attr_dev = dev;
            }
            // (Round 4 measured a 64-ROW split-K tiling for the mid-size batches -- 128 row blocks at 8192 nodes, split-K 4, two 64-KB-LDS
            // workgroups per CU, half the slabs: correct, and slower at every size: 32.1 vs 27.8 us at N = 8192 with a 7.0 instead of 9.3 us
            // tail, 59 vs 46 at 16 384, 129 vs 96 at 32 768 -- 4x the W traffic from L2 and one accumulation chain per wave; the kernel and
            // the log are kept under profiles/r04_logs/: enc_rows64.cuh.txt, ab_enc64_1.log.)
            if (use_r32f) {
                EncF16Params q;
                std::memset(&q, 0, sizeof(q));
                q.x = cur_in;
                q.w2h = reinterpret_cast<const unsigned short*>(blob + hdr.enc_w2h);
                q.w_bad = reinterpret_cast<const unsigned*>(blob + hdr.enc_w2h_bad);
                q.w3 = w3;
                q.M = N, q.K = K, q.kslice = K;
                q.force_arm = f16_force_arm;   // (here and in the 256-row form below: every tile on the bf16 arm)
                q.x_nt = f16_x_nt;
                GNNCCA_LAUNCH(enc_gemm_f16_rows32_kernel, dim3((unsigned)((N + 31) / 32) + 1), dim3(kF16R32Threads), kF16R32LdsBytes, st, q, fp);
            } else if (use_r32) {
                const dim3 rgrid((unsigned)((N + 31) / 32) + 1);
                const int nst = (N + 31) / 32 <= 256 ? 8 : 4;
                if (nst == 8 && split3)
                    GNNCCA_LAUNCH((enc_gemm_rows32_fused_kernel<true, 8>), rgrid, dim3(256), 0, st, cur_in, w3, N, K, fp);
                else if (nst == 8)
                    GNNCCA_LAUNCH((enc_gemm_rows32_fused_kernel<false, 8>), rgrid, dim3(256), 0, st, cur_in, w3, N, K, fp);
                else if (split3)
                    GNNCCA_LAUNCH((enc_gemm_rows32_fused_kernel<true, 4>), rgrid, dim3(256), 0, st, cur_in, w3, N, K, fp);
                else
                    GNNCCA_LAUNCH((enc_gemm_rows32_fused_kernel<false, 4>), rgrid, dim3(256), 0, st, cur_in, w3, N, K, fp);
            } else if (use_lds && use_f16) {
                // round 5: the fp16-split GEMM (enc_f16.cuh) -- three piece products, x and W by LDS-DMA rings; same grids, same epilogues
                EncF16Params q;
                std::memset(&q, 0, sizeof(q));
                q.x = cur_in;
                q.w2h = reinterpret_cast<const unsigned short*>(blob + hdr.enc_w2h);
                q.w_bad = reinterpret_cast<const unsigned*>(blob + hdr.enc_w2h_bad);
                q.w3 = w3;
                q.out = part;
                q.M = N, q.K = K, q.kslice = K / ks_split;
                q.force_arm = f16_force_arm;
                q.x_nt = f16_x_nt;
                const dim3 fgrid((N + 255) / 256 + 1, 1), sgrid((N + 255) / 256, ks_split);
                if (fused_tail)
                    GNNCCA_LAUNCH(enc_gemm_f16_fused_kernel, fgrid, dim3(512), kF16LdsBytes, st, q, fp);
                else
                    GNNCCA_LAUNCH(enc_gemm_f16_split_kernel, sgrid, dim3(512), kF16LdsBytes, st, q, fp);
            } else if (use_lds) {
                // 256-row workgroups, both operands through LDS (144 KB: one workgroup per CU, 8 waves); split-K by whole
                // rounds of 256 workgroups (internal.h: enc_lds_ksplit)
                // (The plan does not ride in this launch.  As extra workgroups: every workgroup reserves the 144 KB of dynamic LDS, so the
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
                const dim3 fgrid((N + 255) / 256 + 1, 1), sgrid((N + 255) / 256, ks_split);
                if (fused_tail && split3)
                    GNNCCA_LAUNCH((enc_gemm_split_lds_kernel<true, true>), fgrid, dim3(512), kLdsGemmBytes, st, cur_in, w3, part, N, K, O, K, fp);
                else if (fused_tail)
                    GNNCCA_LAUNCH((enc_gemm_split_lds_kernel<true, false>), fgrid, dim3(512), kLdsGemmBytes, st, cur_in, w3, part, N, K, O, K, fp);
                else if (split3)
                    GNNCCA_LAUNCH((enc_gemm_split_lds_kernel<false, true>), sgrid, dim3(512), kLdsGemmBytes, st, cur_in, w3, part, N, K, O,
                                  K / ks_split, fp);
                else
                    GNNCCA_LAUNCH((enc_gemm_split_lds_kernel<false, false>), sgrid, dim3(512), kLdsGemmBytes, st, cur_in, w3, part, N, K, O,
                                  K / ks_split, fp);
            } else {
                // 128-row workgroups (a wave = 32 rows x 128 columns); split-K until >= 512 workgroups are in flight
                while (ks_split < ws.ksplit && ((N + 127) / 128) * ks_split < 512 && (K / (ks_split * 2)) % 32 == 0) ks_split *= 2;
                const int rb = (N + 127) / 128;
                // the plan rides in this launch (extra workgroups beyond the GEMM tiles)
                EncPlanParams pl = ep;
                int ride = 0;
                if (plan_blocks > 0) {
                    pl.plan_span = plan_span(edge_index, E);   // narrow (0) or pair form by the edge count and alignment
                    ride = pl.plan_span > 1 ? (plan_blocks + pl.plan_span - 1) / pl.plan_span : plan_blocks;
                    plan_launched = true;
                } else {
                    pl.E = 0;
                }
                const dim3 dgrid((unsigned)(rb * ks_split + ride));
                if (split3)
                    GNNCCA_LAUNCH(enc_gemm_split_direct_kernel<true>, dgrid, dim3(256), 0, st, cur_in, w3, part, N, K, O, K / ks_split, rb, ks_split, pl);
                else
                    GNNCCA_LAUNCH(enc_gemm_split_direct_kernel<false>, dgrid, dim3(256), 0, st, cur_in, w3, part, N, K, O, K / ks_split, rb, ks_split, pl);
            }
            HIP_TRY(hipGetLastError());
            PROF_MARK(GNNCCA_K_ENC_GEMM);
        }
        if (ep.gemm_blocks + plan_blocks > 0 && !plan_launched) {
            if (ep.gemm_blocks == 0 && plan_blocks > 0) {   // a plan-only launch (big batches): several blocks per workgroup
                ep.plan_span = plan_span(edge_index, E);
                if (ep.plan_span > 1) plan_blocks = (plan_blocks + ep.plan_span - 1) / ep.plan_span;
            }
            if (ep.gemm_blocks == 0)
                GNNCCA_LAUNCH(plan_only_kernel, dim3(plan_blocks), dim3(256), 0, st, ep);
            else
                GNNCCA_LAUNCH(enc_gemm_plan_kernel, dim3(ep.gemm_blocks + plan_blocks), dim3(256), 0, st, ep);
            HIP_TRY(hipGetLastError());
            PROF_MARK(split ? GNNCCA_K_PLAN_ROWS : GNNCCA_K_ENC_GEMM);
        }
        // the slabs the GEMM that ran actually wrote: the slices and split forms pick their own count (<= ws.ksplit), the plan
        // GEMM writes ks; the rest of the workspace's slab region holds whatever an earlier forward left there
        ks_last = (split || use_slices) ? ks_split : ks;
        if (g < n_gemm - 1) {
            float* dst = act + (size_t)(g & 1) * N * O;
            GNNCCA_LAUNCH(reduce_bias_act_kernel, grid1((size_t)N * O, 256), dim3(256), 0, st, (const float*)part,
                               blob + hdr.enc_node_b[g], dst, N, O, ks_last, l.relu);
            HIP_TRY(hipGetLastError());
            PROF_MARK(GNNCCA_K_ENC_REDUCE);
            cur_in = dst;
        }
    }
    const int nf = d->reattach_nodes ? 2 : 1;
    const int hin = nf * kH;
    {
        const gnncca_layer& lprev = d->enc_node.layers[n_gemm - 1];
        TailParams tp;
        std::memset(&tp, 0, sizeof(tp));
        tp.blob = blob;
        tp.part = part;
        tp.h0 = h0;
        tp.trace_h = trace ? trace->h_enc : nullptr;
        tp.pd_out = pd[0];
        tp.psq_out = psq[0];
        tp.off_prev_b = hdr.enc_node_b[n_gemm - 1];
        tp.off_lastWT = hdr.enc_last_wT;
        tp.off_last_b = hdr.enc_node_b[nl - 1];
        tp.off_projwT = hdr.proj_wT;
        tp.off_projb = hdr.proj_b;
        tp.ks = ks_last;
        tp.F = lprev.out_dim;
        tp.N = N;
        tp.has_last = nl >= 2;
        tp.relu_prev = lprev.relu;
        tp.reatt_n = d->reattach_nodes;
        tp.hin = hin;
        tp.vec_reduce = (tp.F % 4 == 0) && (tp.F / 4 <= 64) && (64 % (tp.F / 4) == 0);
        const size_t lds = ((size_t)hin * kProjOut + (tp.has_last ? (size_t)tp.F * kH : 0) + 4 * (size_t)tp.F + 4 * 256) * sizeof(float);
        if (lds > 160 * 1024) return GNNCCA_ERR_UNSUPPORTED;
        if (lds > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_tail_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        tp.ei = reinterpret_cast<const long long*>(edge_index);
        tp.seg_ptr = seg_ptr;
        tp.col32 = col32;
        tp.perm = perm;
        tp.cursor = cursor;
        tp.flags = flags;
        tp.blockflags = blockflags;
        tp.E = E;
        tp.drop = drop;
        const unsigned blocks = (unsigned)std::min<size_t>(((size_t)N + 3) / 4, 2048) + 1;  // + plan-repair workgroup
        // register-resident tail in the latency-bound regime only: on big batches it is VALU-bound (readlane traffic) and
        // measured 15 % slower than the LDS form (72 vs 62 us at N = 65 536)
        const bool tail_mfma = tail_mfma_ok && !fused_tail;
        const bool tail_fast = !tail_mfma && !dropping && N < 4096 && tp.F == 128 && tp.has_last && !tp.reatt_n && tp.trace_h == nullptr && tp.vec_reduce &&
                               (reinterpret_cast<uintptr_t>(part) & 15) == 0;
        if (fused_tail) {
            // nothing: h0, the projections and the plan's flag word all came out of the GEMM launch
        } else if (tail_fast) {
            // nodes per workgroup: one up to 320 nodes, two up to 640, four beyond (a block of 200 forwards in one HIP graph: dense256 28.07 ->
            // 27.4 us per forward with one, dense64 24.7 -> 24.1; dense512 39.97 -> 39.5-39.8 with two; dense1024 best with four;
            // profiles/r03_logs/r3_tailnpw1.log)
            tp.npw = N <= 320 ? 1 : (N <= 640 ? 2 : 4);
            const unsigned fblocks = (unsigned)std::min<size_t>(((size_t)N + tp.npw - 1) / tp.npw, 2048) + 1;
            GNNCCA_LAUNCH(enc_tail_fast_kernel, dim3(fblocks), dim3(256), 0, st, tp);
        }
        else if (tail_mfma)
            GNNCCA_LAUNCH(enc_tail_mfma_kernel, dim3((unsigned)((N + 31) / 32) + 1), dim3(256), 0, st, tp,
                          blob + hdr.enc_node_w[nl - 1]);
        else
            GNNCCA_LAUNCH(enc_tail_kernel, dim3(blocks), dim3(256), std::max<size_t>(lds, 4096), st, tp);
        HIP_TRY(hipGetLastError());
        if (!fused_tail) PROF_MARK(GNNCCA_K_ENC_TAIL);
    }
    if (E == 0) return GNNCCA_OK;

    // ---- message passing steps ----------------------------------------------------------------------------
    const int L = d->num_enc_steps;
    const int first_cls = L - d->num_class_steps + 1;  // models/mpn.py:277
    const long long avg_deg = (E + (long long)N - 1) / N;
    const int chunks = (int)((avg_deg + 63) / 64);
    StepParams sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.blob = blob;
    sp.seg_ptr = seg_ptr;
    sp.col32 = col32;
    sp.perm = perm;
    sp.flags = flags;
    sp.edge_attr = edge_attr;
    sp.e = ebuf;
    sp.e0 = e0buf;
    sp.h0 = h0;
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
    int npw_first = 1, npw_later = 1;   // nodes per wave of step 1 / of the later message steps (step_pipe.cuh: NPW)
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
        if (unsplit && N >= 4096) wps = 1;
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
        npw_later = (wps == 1 && chunks <= 2 && (force_npw == 2 || (force_npw == 0 && N >= npw_min_n))) ? 2 : 1;
        npw_first = (npw_later == 2 && (force_npw == 2 || N >= npw_min_n_first)) ? 2 : 1;
        sp.npw = npw_later;
    }
    sp.hin = hin;
    // column ranges instead of the col32 stream on steps 2 ... L of the specialised kernels (StepParams::rng)
    sp.rng = (L >= 2 && (options & GNNCCA_OPT_COLUMN_RANGES) != 0) ? reinterpret_cast<int*>(base + ws.rng) : nullptr;
    sp.ws_base = base;
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
        sp.pd_in = pd[(step - 1) & 1];
        sp.so_pd = (unsigned)ws.pd[(step - 1) & 1];
        sp.psq_in = psq[(step - 1) & 1];
        sp.pd_out = step < L ? pd[step & 1] : nullptr;
        sp.psq_out = step < L ? psq[step & 1] : nullptr;
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
