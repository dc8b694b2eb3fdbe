// mpn_train.hip -- training on the device: the train-mode classifier and the fused backward of the MFMA family
// (backward.cuh, input_grads.cuh), the layer-by-layer engine for every other legal configuration (train_generic.cuh) with its stand-alone
// ops (gnncca_mlp_eval, gnncca_aggregate, gnncca_gather_cat), and the device packer that refreshes the inference blob from the parameters
// after an optimiser step (pack_device.cuh).  The plan, encoder-GEMM and generic op kernels it shares with the forward are compiled in
// mpn_forward.hip and reached through their launchers (internal.h).
#include "common.cuh"
#include "wave_reduce.cuh"
#include "plan.cuh"
#include "backward.cuh"
#include "input_grads.cuh"
#include "pack_device.cuh"
#include "train_generic.cuh"

using namespace gnncca;

extern "C" {

size_t gnncca_mlp_eval_workspace_bytes(const gnncca_mlp* mlp, int64_t rows) {
    if (!mlp_shape_ok(mlp) || rows < 0) return 0;
    return mlp_eval_ws(mlp, rows, nullptr, nullptr, nullptr, nullptr);
}

int gnncca_mlp_eval(const gnncca_mlp* mlp, const float* const* params_dev, int n_params, const float* in, int64_t rows, float* out,
                    void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    return mlp_eval_impl(mlp, params_dev, n_params, in, rows, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int gnncca_gather_cat(const float* a, const int64_t* ia, int wa, int64_t rows_a, const float* b, const int64_t* ib, int wb, int64_t rows_b,
                      const float* c, const int64_t* ic, int wc, int64_t rows_c, int64_t rows, float* out, gnncca_stream_t stream) {
    if (rows < 0 || wa < 0 || wb < 0 || wc < 0 || wa + wb + wc <= 0 || !out) return GNNCCA_ERR_INVALID_ARG;
    if ((wa > 0 && (!a || rows_a <= 0)) || (wb > 0 && (!b || rows_b <= 0)) || (wc > 0 && (!c || rows_c <= 0))) return rows == 0 ? GNNCCA_OK : GNNCCA_ERR_INVALID_ARG;
    if (rows == 0) return GNNCCA_OK;
    hipLaunchKernelGGL(tr_cat64_kernel, grid1((size_t)rows * (wa + wb + wc), 256), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                       reinterpret_cast<const long long*>(ia), wa, (long long)rows_a, b, reinterpret_cast<const long long*>(ib), wb,
                       (long long)rows_b, c, reinterpret_cast<const long long*>(ic), wc, (long long)rows_c, out, (long long)rows);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

size_t gnncca_aggregate_workspace_bytes(int64_t n_nodes, int64_t n_edges) { return agg_ws(n_nodes, n_edges).total; }

int gnncca_aggregate(const float* messages, const int64_t* edge_index, int64_t n_nodes, int64_t n_edges, int width, int agg, float* out,
                     void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    return aggregate_impl(messages, edge_index, n_nodes, n_edges, width, agg, out, workspace, workspace_bytes,
                          static_cast<hipStream_t>(stream));
}

size_t gnncca_train_tape_bytes(const gnncca_mpn_dims* d, int64_t n_nodes, int64_t n_edges) {
    TrPlan P;
    if (!d || n_nodes < 0 || n_edges < 0 || !tr_plan(d, n_nodes, n_edges, &P)) return 0;
    return P.total;
}

int gnncca_train_tape_latents(const gnncca_mpn_dims* d, int64_t n_nodes, int64_t n_edges, int64_t* offsets_out, int n_offsets) {
    TrPlan P;
    if (!d || !offsets_out || n_nodes < 0 || n_edges < 0 || !tr_plan(d, n_nodes, n_edges, &P)) return GNNCCA_ERR_INVALID_ARG;
    const int L = d->num_enc_steps;
    if (n_offsets != 2 + 2 * L) return GNNCCA_ERR_INVALID_ARG;
    auto last = [](const TrCall& c, const gnncca_mlp& m) -> int64_t { return m.n_layers > 0 ? (int64_t)c.lay[m.n_layers - 1].a : -1; };
    offsets_out[0] = last(P.enc_node, d->enc_node);
    offsets_out[1] = last(P.enc_edge, d->enc_edge);
    for (int s = 0; s < L; ++s) {
        offsets_out[2 + 2 * s] = (int64_t)P.h[s];
        offsets_out[3 + 2 * s] = last(P.edge[s], d->edge_mlp);
    }
    return GNNCCA_OK;
}

int gnncca_train_forward(const gnncca_mpn_dims* d, float* const* params_dev, int n_params, const float* x, const int64_t* edge_index,
                         const float* edge_attr, int64_t n_nodes, int64_t n_edges, void* tape, size_t tape_bytes, float* logits_out,
                         const gnncca_dropout* dropout, gnncca_stream_t stream) {
    if (!x || (n_edges > 0 && (!edge_index || !edge_attr || !logits_out))) return GNNCCA_ERR_INVALID_ARG;
    return train_forward_impl(d, params_dev, n_params, x, edge_index, edge_attr, n_nodes, n_edges, tape, tape_bytes, logits_out, dropout,
                              static_cast<hipStream_t>(stream));
}

int gnncca_train_backward(const gnncca_mpn_dims* d, float* const* params_dev, int n_params, const float* x, const int64_t* edge_index,
                          const float* edge_attr, int64_t n_nodes, int64_t n_edges, void* tape, size_t tape_bytes,
                          const float* grad_logits, float* const* grads_dev, const gnncca_dropout* dropout, gnncca_stream_t stream) {
    return gnncca_train_backward_inputs(d, params_dev, n_params, x, edge_index, edge_attr, n_nodes, n_edges, tape, tape_bytes, grad_logits,
                                        grads_dev, dropout, nullptr, stream);
}

int gnncca_train_backward_inputs(const gnncca_mpn_dims* d, float* const* params_dev, int n_params, const float* x,
                                 const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges, void* tape,
                                 size_t tape_bytes, const float* grad_logits, float* const* grads_dev, const gnncca_dropout* dropout,
                                 const gnncca_input_grads* input_grads, gnncca_stream_t stream) {
    if (!x || (n_edges > 0 && (!edge_index || !edge_attr))) return GNNCCA_ERR_INVALID_ARG;
    return train_backward_impl(d, params_dev, n_params, x, edge_index, edge_attr, n_nodes, n_edges, tape, tape_bytes, grad_logits,
                               grads_dev, dropout, input_grads ? input_grads->dx : nullptr,
                               input_grads ? input_grads->d_edge_attr : nullptr, static_cast<hipStream_t>(stream));
}

// ---- backward ---------------------------------------------------------------------------
// gnncca_dropout -> DropCfg; GNNCCA_OK with all p == 0 for a null / inactive one
static int drop_cfg(const gnncca_dropout* dropout, DropCfg* out) {
    std::memset(out, 0, sizeof(*out));
    if (!dropout) return GNNCCA_OK;
    const float ps[4] = {dropout->p_enc, dropout->p_edge, dropout->p_node, dropout->p_cls};
    bool any = false;
    for (float q : ps) {
        if (!(q >= 0.f && q < 1.f)) return GNNCCA_ERR_INVALID_ARG;
        any = any || q > 0.f;
    }
    if (!any) return GNNCCA_OK;
    if (!dropout->seed_dev) return GNNCCA_ERR_INVALID_ARG;
    out->p_enc = dropout->p_enc, out->p_edge = dropout->p_edge, out->p_node = dropout->p_node, out->p_cls = dropout->p_cls;
    out->seed = reinterpret_cast<const unsigned long long*>(dropout->seed_dev);
    return GNNCCA_OK;
}

static bool backward_ok(const gnncca_mpn_dims* d) {
    if (classify(d) != kFamilyMfma32x6) return false;
    if (d->num_enc_steps < 1) return false;
    if (d->enc_node.n_layers != 2) return false;
    const gnncca_mlp* all[5] = {&d->enc_node, &d->enc_edge, &d->edge_mlp, &d->node_mlp, &d->cls_edge};
    for (int mi = 0; mi < 5; ++mi)
        for (int l = 0; l < all[mi]->n_layers; ++l)
            if (all[mi]->layers[l].has_bn && !(mi == 4 && l == 0 && d->cls_edge.n_layers == 2)) return false;
    return true;  // BatchNorm is allowed only between the classifier's two layers (the shipped inference config)
}

// Train-mode classifier with BatchNorm1d between its two layers: batch statistics over the E edges for every
// classified step (models/mpn.py:290-293 with models/mlp.py:15 in train mode); running buffers updated in place.
int gnncca_classifier_train(const gnncca_mpn_dims* d, const float* const* params_dev, int n_params, const float* e_steps,
                            int64_t n_edges, void* scratch /* 2*C1 doubles */, float* bn_stat_out /* [n_out][C1][2] */,
                            float* logits_out, gnncca_stream_t stream) {
    return gnncca_classifier_train_dropout(d, params_dev, n_params, e_steps, n_edges, scratch, bn_stat_out, logits_out, nullptr, stream);
}

int gnncca_classifier_train_dropout(const gnncca_mpn_dims* d, const float* const* params_dev, int n_params, const float* e_steps,
                                    int64_t n_edges, void* scratch /* 2*C1 doubles */, float* bn_stat_out /* [n_out][C1][2] */,
                                    float* logits_out, const gnncca_dropout* dropout, gnncca_stream_t stream) {
    DropCfg drop;
    {
        const int ds = drop_cfg(dropout, &drop);
        if (ds != GNNCCA_OK) return ds;
    }
    if (!dims_valid(d) || !params_dev || n_params != gnncca_param_count(d) || n_edges < 0) return GNNCCA_ERR_INVALID_ARG;
    if (!backward_ok(d) || d->cls_edge.n_layers != 2 || !d->cls_edge.layers[0].has_bn) return GNNCCA_ERR_UNSUPPORTED;
    if (n_edges == 0) return GNNCCA_OK;
    if (!e_steps || !scratch || !bn_stat_out || !logits_out) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int C1 = d->cls_edge.layers[0].out_dim, L = d->num_enc_steps, first_cls = L - d->num_class_steps + 1;
    const ParamSlots c1s = param_slots(d, 4, 0), c2s = param_slots(d, 4, 1);
    const float *W1 = params_dev[c1s.w], *b1 = params_dev[c1s.b], *gamma = params_dev[c1s.bn], *beta = params_dev[c1s.bn + 1];
    float *rm = const_cast<float*>(params_dev[c1s.bn + 2]), *rv = const_cast<float*>(params_dev[c1s.bn + 3]);
    const float *W2 = params_dev[c2s.w], *b2 = params_dev[c2s.b];
    const long long E = n_edges;
    double* sums = static_cast<double*>(scratch);
    int li = 0;
    for (int s = 1; s <= L; ++s) {
        if (s < first_cls) continue;
        const float* e = e_steps + (size_t)(s - 1) * E * kEF;
        float* stat = bn_stat_out + (size_t)li * C1 * 2;
        HIP_TRY(hipMemsetAsync(sums, 0, sizeof(double) * 2 * C1, st));
        hipLaunchKernelGGL(cls_bn_stats_kernel, grid1((size_t)E, 256), dim3(256), 0, st, e, E, W1, b1, C1, sums);
        hipLaunchKernelGGL(cls_bn_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)sums, E, C1, stat, rm, rv);
        hipLaunchKernelGGL(cls_bn_apply_kernel, grid1((size_t)E, 256), dim3(256), 0, st, e, E, W1, b1, gamma, beta, (const float*)stat,
                           W2, b2, C1, logits_out + (size_t)li * E, drop, li);
        HIP_TRY(hipGetLastError());
        ++li;
    }
    return GNNCCA_OK;
}

int gnncca_backward_supported(const gnncca_mpn_dims* d) {
    if (!dims_valid(d)) return GNNCCA_ERR_INVALID_ARG;
    return backward_ok(d) ? GNNCCA_OK : GNNCCA_ERR_UNSUPPORTED;
}

size_t gnncca_backward_workspace_bytes(const gnncca_mpn_dims* d, int64_t n_nodes, int64_t n_edges) {
    if (!dims_valid(d) || !backward_ok(d) || n_nodes < 0 || n_edges < 0) return 0;
    return carve_backward(d, n_nodes, n_edges).total;
}

size_t gnncca_pack_program_bytes(void) { return sizeof(PackProgram); }

int gnncca_pack_program(const gnncca_mpn_dims* d, void* program_host, size_t program_bytes) {
    if (!dims_valid(d) || !program_host) return GNNCCA_ERR_INVALID_ARG;
    if (classify(d) != kFamilyMfma32x6) return GNNCCA_ERR_UNSUPPORTED;
    if (program_bytes < sizeof(PackProgram)) return GNNCCA_ERR_INVALID_ARG;
    return pack_program(d, static_cast<PackProgram*>(program_host)) ? GNNCCA_OK : GNNCCA_ERR_UNSUPPORTED;
}

int gnncca_pack_weights_device(const gnncca_mpn_dims* d, const float* const* params_dev, int n_params, const void* program_dev,
                               void* packed_dev, size_t packed_bytes, gnncca_stream_t stream) {
    if (!dims_valid(d) || !params_dev || !program_dev || !packed_dev) return GNNCCA_ERR_INVALID_ARG;
    if (classify(d) != kFamilyMfma32x6) return GNNCCA_ERR_UNSUPPORTED;
    if (n_params != gnncca_param_count(d) || n_params > kMaxPackParams) return GNNCCA_ERR_INVALID_ARG;
    if (packed_bytes < gnncca_packed_weights_bytes(d)) return GNNCCA_ERR_INVALID_ARG;
    PackProgram host;  // segment count only: the program itself is read on the device
    if (!pack_program(d, &host)) return GNNCCA_ERR_UNSUPPORTED;
    PackPtrs ptrs;
    std::memset(&ptrs, 0, sizeof(ptrs));
    for (int i = 0; i < n_params; ++i) {
        if (!params_dev[i]) return GNNCCA_ERR_INVALID_ARG;
        ptrs.p[i] = params_dev[i];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pack_device_kernel, dim3(64, (unsigned)host.n_segs + 1), dim3(256), 0, st,
                       static_cast<const PackProgram*>(program_dev), ptrs, static_cast<float*>(packed_dev));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_mpn_backward(const gnncca_mpn_dims* d, const float* const* params_dev, int n_params, const float* x,
                        const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                        const gnncca_trace* saved, const float* cls_bn_stat, const float* grad_logits,
                        float* const* grads_dev, void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    return gnncca_mpn_backward_ex(d, params_dev, n_params, x, edge_index, edge_attr, n_nodes, n_edges, saved, cls_bn_stat,
                                  grad_logits, grads_dev, workspace, workspace_bytes, 0u, stream);
}

int gnncca_mpn_backward_ex(const gnncca_mpn_dims* d, const float* const* params_dev, int n_params, const float* x,
                           const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                           const gnncca_trace* saved, const float* cls_bn_stat, const float* grad_logits,
                           float* const* grads_dev, void* workspace, size_t workspace_bytes, uint32_t options,
                           gnncca_stream_t stream) {
    return gnncca_mpn_backward_train(d, params_dev, n_params, x, edge_index, edge_attr, n_nodes, n_edges, saved, cls_bn_stat,
                                     grad_logits, grads_dev, workspace, workspace_bytes, options, nullptr, stream);
}

int gnncca_mpn_backward_train(const gnncca_mpn_dims* d, const float* const* params_dev, int n_params, const float* x,
                              const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                              const gnncca_trace* saved, const float* cls_bn_stat, const float* grad_logits,
                              float* const* grads_dev, void* workspace, size_t workspace_bytes, uint32_t options,
                              const gnncca_dropout* dropout, gnncca_stream_t stream) {
    return gnncca_mpn_backward_inputs(d, params_dev, n_params, x, edge_index, edge_attr, n_nodes, n_edges, saved, cls_bn_stat,
                                      grad_logits, grads_dev, workspace, workspace_bytes, options, dropout, nullptr, stream);
}

int gnncca_mpn_backward_inputs(const gnncca_mpn_dims* d, const float* const* params_dev, int n_params, const float* x,
                               const int64_t* edge_index, const float* edge_attr, int64_t n_nodes, int64_t n_edges,
                               const gnncca_trace* saved, const float* cls_bn_stat, const float* grad_logits,
                               float* const* grads_dev, void* workspace, size_t workspace_bytes, uint32_t options,
                               const gnncca_dropout* dropout, const gnncca_input_grads* input_grads, gnncca_stream_t stream) {
    float* const dx_out = input_grads ? input_grads->dx : nullptr;
    float* const dattr_out = input_grads ? input_grads->d_edge_attr : nullptr;
    DropCfg drop;
    {
        const int ds = drop_cfg(dropout, &drop);
        if (ds != GNNCCA_OK) return ds;
    }
    if (!dims_valid(d) || n_nodes < 0 || n_edges < 0) return GNNCCA_ERR_INVALID_ARG;
    if (!backward_ok(d)) return GNNCCA_ERR_UNSUPPORTED;
    if (n_params != gnncca_param_count(d) || !params_dev || !grads_dev) return GNNCCA_ERR_INVALID_ARG;
    for (int i = 0; i < n_params; ++i)
        if (!params_dev[i] || !grads_dev[i]) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_nodes, E = (int)n_edges;
    const int D = d->node_in, F1 = d->enc_node.layers[0].out_dim, A = d->edge_in;
    const int L = d->num_enc_steps, first_cls = L - d->num_class_steps + 1;
    const int c1 = d->cls_edge.n_layers == 2 ? d->cls_edge.layers[0].out_dim : 0;
    // zero every gradient
    if (!(options & GNNCCA_BWD_GRADS_ZEROED)) {
        for (int mi = 0; mi < 5; ++mi)
            for (int l = 0; l < mlp_by_index(d, mi).n_layers; ++l) {
                const gnncca_layer& ly = mlp_by_index(d, mi).layers[l];
                const ParamSlots ps = param_slots(d, mi, l);
                HIP_TRY(hipMemsetAsync(grads_dev[ps.w], 0, (size_t)ly.in_dim * ly.out_dim * 4, st));
                HIP_TRY(hipMemsetAsync(grads_dev[ps.b], 0, (size_t)ly.out_dim * 4, st));
                if (ps.bn >= 0)  // gamma, beta, and the two buffers (no gradient: left at zero)
                    for (int k = 0; k < 4; ++k) HIP_TRY(hipMemsetAsync(grads_dev[ps.bn + k], 0, (size_t)ly.out_dim * 4, st));
            }
    }
    if (N == 0 || E == 0) {   // no edge, no logit: nothing reaches either input
        if (dx_out && N > 0) HIP_TRY(hipMemsetAsync(dx_out, 0, (size_t)N * D * 4, st));
        return GNNCCA_OK;
    }
    if (!x || !edge_index || !edge_attr || !saved || !saved->h_enc || !saved->e_enc || !saved->h_steps || !saved->e_steps ||
        !grad_logits || !workspace)
        return GNNCCA_ERR_INVALID_ARG;
    const BwdWorkspace ws = carve_backward(d, n_nodes, n_edges);
    if (workspace_bytes < ws.total) return GNNCCA_ERR_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    float* gh0_acc = reinterpret_cast<float*>(base + ws.gh0_acc);
    float* ge0_acc = reinterpret_cast<float*>(base + ws.ge0_acc);
    int* deg = reinterpret_cast<int*>(base + ws.deg);
    float* Q = reinterpret_cast<float*>(base + ws.Q);
    int* hmax = reinterpret_cast<int*>(base + ws.hmax);
    int* hcnt = hmax + (size_t)N * kH;
    float* dP_all = reinterpret_cast<float*>(base + ws.dP_all);
    float* Hb[2] = {reinterpret_cast<float*>(base + ws.Hb[0]), reinterpret_cast<float*>(base + ws.Hb[1])};
    float* Gb[2] = {reinterpret_cast<float*>(base + ws.Gb[0]), reinterpret_cast<float*>(base + ws.Gb[1])};
    float* a1 = reinterpret_cast<float*>(base + ws.a1);
    float* gz1 = reinterpret_cast<float*>(base + ws.gz1);
    float* part = reinterpret_cast<float*>(base + ws.part);
    // the tensors' places in the parameter list (backward_ok: a two-layer node encoder; the second classifier layer only where c1)
    const ParamSlots sx1 = param_slots(d, 0, 0), sx2 = param_slots(d, 0, 1), se0 = param_slots(d, 1, 0), se = param_slots(d, 2, 0);
    const ParamSlots sn = param_slots(d, 3, 0), sc1 = param_slots(d, 4, 0), sc2 = param_slots(d, 4, 1);
    const float *W1 = params_dev[sx1.w], *b1 = params_dev[sx1.b], *W2 = params_dev[sx2.w];
    const float *We = params_dev[se.w], *Wn = params_dev[sn.w], *bn = params_dev[sn.b];
    const bool cls_bn = sc1.bn >= 0;
    if (cls_bn && !cls_bn_stat) return GNNCCA_ERR_INVALID_ARG;
    const float *Wc1 = params_dev[sc1.w], *bc1 = params_dev[sc1.b], *Wc2 = c1 ? params_dev[sc2.w] : nullptr;
    const float *cls_gamma = cls_bn ? params_dev[sc1.bn] : nullptr, *cls_beta = cls_bn ? params_dev[sc1.bn + 1] : nullptr;
    float *gW1 = grads_dev[sx1.w], *gb1 = grads_dev[sx1.b], *gW2 = grads_dev[sx2.w], *gb2 = grads_dev[sx2.b];
    float *gWe0 = grads_dev[se0.w], *gbe0 = grads_dev[se0.b], *gWe = grads_dev[se.w], *gbe = grads_dev[se.b];
    float *gWn = grads_dev[sn.w], *gbn = grads_dev[sn.b], *gWc1 = grads_dev[sc1.w], *gbc1 = grads_dev[sc1.b];
    float *gWc2 = c1 ? grads_dev[sc2.w] : nullptr, *gbc2 = c1 ? grads_dev[sc2.b] : nullptr;
    double* bn_sums = reinterpret_cast<double*>(base + ws.bn_sums);
    float* bn_red = reinterpret_cast<float*>(base + ws.bn_red);
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    if (d->agg == GNNCCA_AGG_MEAN) {
        HIP_TRY(hipMemsetAsync(deg, 0, (size_t)N * 4, st));
        hipLaunchKernelGGL(bwd_degree_kernel, grid1((size_t)E, 256), dim3(256), 0, st, ei, (long long)E, N, deg);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(dP_all, 0, (size_t)std::max(L, 1) * N * 44 * 4, st));
    const bool re_n = d->reattach_nodes != 0, re_e = d->reattach_edges != 0;
    const int HI = re_n ? 2 * kH : kH, WeLd = 2 * HI + (re_e ? 2 * kEF : kEF), WnLd = HI + kEF;
    if (re_n) HIP_TRY(hipMemsetAsync(gh0_acc, 0, (size_t)N * kH * 4, st));
    if (re_e) HIP_TRY(hipMemsetAsync(ge0_acc, 0, (size_t)E * kEF * 4, st));
    const float* g_h = nullptr;   // d loss / d h_s of the step being processed (null for s = L: its node update is dead)
    const float* ge_in = nullptr; // d loss / d e_s arriving from step s+1
    int out_idx = gnncca_num_outputs(d) - 1;
    for (int s = L; s >= 1; --s) {
        const float* h_prev = s == 1 ? saved->h_enc : saved->h_steps + (size_t)(s - 2) * N * kH;
        const float* e_cur = saved->e_steps + (size_t)(s - 1) * E * kEF;
        const float* e_prev = s == 1 ? saved->e_enc : saved->e_steps + (size_t)(s - 2) * E * kEF;
        if (g_h) {
            hipLaunchKernelGGL(bwd_q_kernel, grid1((size_t)N * kH, 256), dim3(256), 0, st, saved->h_enc, h_prev, Wn, bn, Q, N, HI);
            HIP_TRY(hipGetLastError());
        }
        float* dP = dP_all + (size_t)(s - 1) * N * 44;
        BwdEdgeParams bp;
        std::memset(&bp, 0, sizeof(bp));
        bp.ei = ei;
        bp.e_cur = e_cur;
        bp.e_prev = e_prev;
        bp.e0 = re_e ? saved->e_enc : nullptr;
        bp.ge0_acc = re_e ? ge0_acc : nullptr;
        bp.HI = HI;
        bp.Q = Q;
        bp.g_h = g_h;
        bp.deg = d->agg == GNNCCA_AGG_MEAN ? deg : nullptr;
        if (g_h && d->agg == GNNCCA_AGG_MAX) {  // which edge attained each node's maximum
            HIP_TRY(hipMemsetAsync(hmax, 0, (size_t)2 * N * kH * 4, st));
            hipLaunchKernelGGL(bwd_max_kernel<false>, grid1((size_t)E, 256), dim3(256), 0, st, ei, e_cur, (const float*)Q, Wn,
                               (long long)E, N, HI, hmax, hcnt, drop, s);
            hipLaunchKernelGGL(bwd_max_kernel<true>, grid1((size_t)E, 256), dim3(256), 0, st, ei, e_cur, (const float*)Q, Wn,
                               (long long)E, N, HI, hmax, hcnt, drop, s);
            HIP_TRY(hipGetLastError());
            bp.hmax = hmax;
            bp.hcnt = hcnt;
        }
        bp.g_logit = s >= first_cls ? grad_logits + (size_t)out_idx * E : nullptr;
        if (bp.g_logit && cls_bn) {  // reductions the BatchNorm backward needs before any per-edge gradient
            const float* stat = cls_bn_stat + (size_t)out_idx * c1 * 2;
            HIP_TRY(hipMemsetAsync(bn_sums, 0, sizeof(double) * 2 * c1, st));
            hipLaunchKernelGGL(bwd_cls_bn_reduce_kernel, grid1((size_t)E, 256), dim3(256), 0, st, e_cur, bp.g_logit, (long long)E, Wc1,
                               bc1, cls_gamma, cls_beta, stat, Wc2, c1, bn_sums, gWc2, gbc2, drop, out_idx);
            hipLaunchKernelGGL(bwd_cls_bn_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)bn_sums, (long long)E, c1, bn_red,
                               grads_dev[sc1.bn], grads_dev[sc1.bn + 1]);
            HIP_TRY(hipGetLastError());
            bp.bn_gamma = cls_gamma;
            bp.bn_beta = cls_beta;
            bp.bn_stat = stat;
            bp.bn_red = bn_red;
        }
        if (bp.g_logit) --out_idx;
        bp.drop = drop;
        bp.step_no = s;
        bp.cls_no = bp.g_logit ? out_idx + 1 : 0;   // out_idx was already stepped down past this classified step
        bp.ge_in = ge_in;
        bp.ge_out = Gb[s & 1];
        bp.dP = dP;
        bp.We = We;
        bp.Wn = Wn;
        bp.Wc1 = Wc1;
        bp.bc1 = bc1;
        bp.Wc2 = Wc2;
        bp.gWe = gWe;
        bp.gbe = gbe;
        bp.gWn = gWn;
        bp.gbn = gbn;
        bp.gWc1 = gWc1;
        bp.gbc1 = gbc1;
        bp.gWc2 = gWc2;
        bp.gbc2 = gbc2;
        bp.E = E;
        bp.N = N;
        bp.cls_hidden = c1;
        {   // persistent grid: enough workgroups to fill the chip, few enough that the final flush of the LDS-resident
            // parameter-gradient sums stays a few thousand atomics
            const unsigned chunks = (unsigned)(((size_t)E + 255) / 256);
            hipLaunchKernelGGL(bwd_edge_kernel, dim3(std::min(chunks, 512u)), dim3(256), 0, st, bp);
        }
        HIP_TRY(hipGetLastError());
        float* g_h_prev = Hb[s & 1];
        hipLaunchKernelGGL(bwd_node_kernel, grid1((size_t)N * HI, 256), dim3(256), 0, st, (const float*)dP, We, Wn, g_h_prev, gh0_acc, N,
                           HI, WeLd);
        HIP_TRY(hipGetLastError());
        // d W_src, d W_dst (columns 0..31, 32..63 of the edge-MLP weight), d W_nx (columns 0..31 of the node-MLP weight)
        // d W_src, d W_dst (columns [0, HI) and [HI, 2 HI) of the edge-MLP weight), d W_nx (columns [0, HI) of the node-MLP
        // weight): one product dP^T hin [44][HI], rows routed to the three weight blocks; hin = cat(h0, h_prev) with
        // reattach_initial_nodes, i.e. two 32-column products
        for (int part = 0; part < (re_n ? 2 : 1); ++part) {
            const float* hsrc = (re_n && part == 0) ? saved->h_enc : h_prev;
            const int coff = part * kH;
            OuterOut oo;
            oo.ptr[0] = gWe + coff, oo.ptr[1] = gWe + HI + coff, oo.ptr[2] = g_h ? gWn + coff : nullptr;
            oo.ld[0] = oo.ld[1] = WeLd, oo.ld[2] = WnLd;
            oo.row_begin[0] = 0, oo.row_begin[1] = 6, oo.row_begin[2] = 12, oo.row_begin[3] = 44;
            HIP_TRY(launch_outer_multi(dP, 44, hsrc, kH, oo, nullptr, N, g_h ? 44 : 12, kH, st));
        }
        g_h = g_h_prev;
        ge_in = Gb[s & 1];
    }
    // gradients that reached the encoder outputs through the reattached copies
    if (re_n) hipLaunchKernelGGL(bwd_add_kernel, grid1((size_t)N * kH, 256), dim3(256), 0, st, const_cast<float*>(g_h),
                                 (const float*)gh0_acc, (long long)N * kH);
    if (re_e) hipLaunchKernelGGL(bwd_add_kernel, grid1((size_t)E * kEF, 256), dim3(256), 0, st, const_cast<float*>(ge_in),
                                 (const float*)ge0_acc, (long long)E * kEF);
    // ---- encoders ---------------------------------------------------------------------------------------------------
    hipLaunchKernelGGL(bwd_edge_enc_kernel, dim3(std::min((unsigned)(((size_t)E + 255) / 256), 512u)), dim3(256), 0, st, ge_in,
                       saved->e_enc, edge_attr, A, (long long)E,
                       gWe0, gbe0, 1.f / (1.f - drop.p_enc));
    HIP_TRY(hipGetLastError());
    {   // a1 = ReLU(x W1^T + b1) is recomputed instead of stored: the forward's split-K MFMA GEMM + its reduce kernel
        const int ks = plan_gemm_ksplit(N, D);
        int kslice = (D + ks - 1) / ks;
        kslice = (kslice + 63) / 64 * 64;
        EncPlanParams ep;
        std::memset(&ep, 0, sizeof(ep));
        ep.in = x;
        ep.W = W1;
        ep.part = part;
        ep.M = N;
        ep.K = D;
        ep.O = F1;
        ep.kslice = kslice;
        ep.vec_ok = (D % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
        ep.nrt = (N + 31) / 32;
        ep.nks = ks;
        ep.gemm_blocks = ep.nrt * ks * ((F1 + 127) / 128);
        launch_enc_gemm_plan(ep, ep.gemm_blocks, st);
        HIP_TRY(hipGetLastError());
        launch_reduce_bias_act(part, b1, a1, N, F1, ks, 1, st);
        HIP_TRY(hipGetLastError());
        if (drop.p_enc > 0.f) {   // the forward's layer-2 input was a1 AFTER Dropout: re-derive the same mask
            hipLaunchKernelGGL(apply_dropout_kernel, grid1((size_t)N * F1, 256), dim3(256), 0, st, a1, (long long)N * F1, drop,
                               (unsigned)kDropEncNode1, drop.p_enc);
            HIP_TRY(hipGetLastError());
        }
    }
    float* gz2 = const_cast<float*>(g_h);  // [N][32] d loss / d h_enc, masked in place
    const float enc_scale = 1.f / (1.f - drop.p_enc);
    hipLaunchKernelGGL(bwd_relu_mask_kernel, grid1((size_t)N * kH, 256), dim3(256), 0, st, gz2, saved->h_enc, (long long)N * kH, enc_scale);
    HIP_TRY(launch_outer(gz2, kH, a1, F1, gW2, F1, gb2, N, kH, F1, st));
    hipLaunchKernelGGL(bwd_matmul_mask_kernel, grid1((size_t)N * F1, 256), dim3(256), 0, st, (const float*)gz2, W2, (const float*)a1,
                       gz1, N, kH, F1, enc_scale);
    HIP_TRY(launch_outer(gz1, F1, x, D, gW1, D, gb1, N, F1, D, st));
    HIP_TRY(hipGetLastError());
    // ---- inputs (only what the caller asked for) ----------------------------------------------------------------------
    if (dattr_out) {
        hipLaunchKernelGGL(bwd_edge_attr_kernel, grid1((size_t)E * A, 256), dim3(256), 0, st, ge_in, saved->e_enc, params_dev[se0.w],
                           dattr_out, A, (long long)E, enc_scale);
        HIP_TRY(hipGetLastError());
    }
    if (dx_out) HIP_TRY(launch_dx(gz1, W1, dx_out, N, F1, D, st));
    return GNNCCA_OK;
}

}  // extern "C"
