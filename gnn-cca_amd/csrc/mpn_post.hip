// mpn_post.hip -- post-processing on the device (threshold, pruning, flow counters, connected components; kernels in
// postprocess.cuh), the camera-exclusive clusters (exclusive.cuh), the strongly connected components of the unpruned edges (strong.cuh) and
// the one-call frame pipeline gnncca_frames_forward, which chains graph build, forward and post stage on one stream.
// The graph-plan kernels it needs are compiled in mpn_forward.hip and reached through their launchers (internal.h).
#include "common.cuh"
#include "plan.cuh"
#include "postprocess.cuh"
#include "exclusive.cuh"
#include "strong.cuh"

namespace gnncca {

int launch_post_plan(const long long* ei, int E, int N, const PostPlanPtrs& p, EmptyPlan when_empty, gnncca_stream_t stream) {
    if (E > 0) {
        EncPlanParams ep;
        std::memset(&ep, 0, sizeof(ep));
        ep.ei = ei, ep.seg_ptr = p.seg_ptr, ep.col32 = p.col32, ep.blockflags = p.blockflags, ep.E = E, ep.N = N;
        launch_plan_only(ep, plan_num_blocks(E), stream);
        HIP_TRY(hipGetLastError());
    }
    if (E > 0 || when_empty == EmptyPlan::kFinish) {
        launch_gen_plan_finish(ei, E, N, p.seg_ptr, p.col32, p.perm, p.cursor, p.flags, p.blockflags, stream);
        HIP_TRY(hipGetLastError());
    }
    return GNNCCA_OK;
}

}  // namespace gnncca

using namespace gnncca;

extern "C" {

int gnncca_pad_frame(const float* x, int64_t n_nodes, const int64_t* edge_index, const float* edge_attr, int64_t n_edges, float* x_pad,
                     int64_t n_real_max, int n_dummy, int64_t* edge_index_pad, float* edge_attr_pad, int64_t e_pad, int node_in, int edge_in,
                     gnncca_stream_t stream) {
    if (n_nodes < 0 || n_edges < 0 || n_real_max < n_nodes || e_pad < n_edges || n_dummy < 1 || node_in < 1 || edge_in < 1) return GNNCCA_ERR_INVALID_ARG;
    if (!x_pad || !edge_index_pad || !edge_attr_pad || (n_nodes > 0 && !x) || (n_edges > 0 && (!edge_index || !edge_attr))) return GNNCCA_ERR_INVALID_ARG;
    const long long total = (n_real_max + n_dummy) * (long long)node_in + e_pad * (2ll + edge_in);
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(pad_frame_kernel, dim3(std::max(blocks, 1u)), dim3(256), 0, static_cast<hipStream_t>(stream), x, (long long)n_nodes,
                       reinterpret_cast<const long long*>(edge_index), edge_attr, (long long)n_edges, x_pad, (long long)n_real_max, n_dummy,
                       reinterpret_cast<long long*>(edge_index_pad), edge_attr_pad, (long long)e_pad, node_in, edge_in);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

// ---- SURVEY.md 8f row N2 ------------------------------------------------------------------------------------
size_t gnncca_post_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
    if (n_nodes < 0 || n_edges < 0) return 0;
    return carve_post(n_nodes, n_edges).total;
}

int gnncca_post_threshold(const float* logits, int64_t n_edges, float* probs_out, int64_t* predictions_out,
                          gnncca_stream_t stream) {
    if (n_edges < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges == 0) return GNNCCA_OK;
    if (!logits || !probs_out || !predictions_out) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(post_threshold_kernel, grid1((size_t)n_edges, 256), dim3(256), 0, st, logits, (long long)n_edges, probs_out,
                       reinterpret_cast<long long*>(predictions_out));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_post_threshold_at(const float* logits, int64_t n_edges, double at, float* probs_out, int64_t* predictions_out,
                             gnncca_stream_t stream) {
    if (n_edges < 0 || at != at) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges == 0) return GNNCCA_OK;
    if (!logits || !probs_out || !predictions_out) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(post_threshold_at_kernel, grid1((size_t)n_edges, 256), dim3(256), 0, st, logits, (long long)n_edges, at, probs_out,
                       reinterpret_cast<long long*>(predictions_out));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

// `plan` (internal; null from the public entry points): the graph plan the MPN forward of the same batch left in ITS workspace (seg_ptr,
// col32, perm, flags) -- gnncca_frames_forward hands it over, so the pruning needs no plan launches of its own
struct PostPlan {
    const int* seg_ptr;
    const int* col32;
    const int* perm;
    const unsigned* flags;
    // gnncca_frames_forward's two other savings: the counters were zeroed by an earlier kernel of the batch (no memset node here), and the
    // threshold rides in the prune kernel (logits in, probabilities and predictions out)
    bool counters_zeroed;
    const float* logits;
    float* probs_out;
    int64_t* preds_out;
};
// The plan the forward of (d, n, e) left in `workspace`, whichever family's carve applies (both name the four offsets alike); the rest unset.
static PostPlan forward_plan(const gnncca_mpn_dims* d, void* workspace, int64_t n, int64_t e) {
    const auto at = [&](const auto& ws) {
        const char* wb = static_cast<const char*>(workspace);
        return PostPlan{reinterpret_cast<const int*>(wb + ws.seg_ptr), reinterpret_cast<const int*>(wb + ws.col32),
                        reinterpret_cast<const int*>(wb + ws.perm), reinterpret_cast<const unsigned*>(wb + ws.flags), false, nullptr, nullptr, nullptr};
    };
    return classify(d) == kFamilyMfma32x6 ? at(carve(d, n, e)) : at(carve_generic(d, n, e));
}

// Zeroes the counters the cluster kernels add to: flow_out [N], flow_in [N], *n_clusters and -- where the caller has them (`triggers`
// not null) -- the cluster sizes [N] and the n_trig trigger words.  ONE memset when the caller laid them out back to back in that order
// (gnn_cca_amd.postprocess does), one per array otherwise, the flows and the count in one where only those three adjoin.  N == 0: there
// are no flows and no sizes; the count (where there is one) and the trigger words.
static int zero_post_counters(int32_t* flow_out, int32_t* flow_in, int32_t* n_clusters, size_t N, int32_t* sizes, int32_t* triggers,
                              size_t n_trig, hipStream_t st) {
    if (N == 0) {
        if (n_clusters) HIP_TRY(hipMemsetAsync(n_clusters, 0, sizeof(int32_t), st));
        if (triggers) HIP_TRY(hipMemsetAsync(triggers, 0, n_trig * 4, st));
        return GNNCCA_OK;
    }
    const bool one_block = flow_in == flow_out + N && n_clusters == flow_in + N;
    if (one_block && triggers && sizes == n_clusters + 1 && triggers == sizes + N) {
        HIP_TRY(hipMemsetAsync(flow_out, 0, (3 * N + 1 + n_trig) * 4, st));
        return GNNCCA_OK;
    }
    if (one_block) {
        HIP_TRY(hipMemsetAsync(flow_out, 0, (2 * N + 1) * 4, st));
    } else {
        HIP_TRY(hipMemsetAsync(flow_out, 0, N * 4, st));
        HIP_TRY(hipMemsetAsync(flow_in, 0, N * 4, st));
        HIP_TRY(hipMemsetAsync(n_clusters, 0, sizeof(int32_t), st));
    }
    if (triggers) {
        HIP_TRY(hipMemsetAsync(sizes, 0, N * 4, st));
        HIP_TRY(hipMemsetAsync(triggers, 0, n_trig * 4, st));
    }
    return GNNCCA_OK;
}

static int post_prune_cluster_impl(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes, int64_t n_edges,
                                   const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames, void* workspace,
                                   size_t workspace_bytes, int64_t* pruned_out, int32_t* flow_out, int32_t* flow_in, int32_t* labels_out,
                                   int32_t* n_clusters_out, int32_t* sizes_scratch, int32_t* triggers_out, const PostPlan* plan,
                                   gnncca_stream_t stream) {
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0) return GNNCCA_ERR_INVALID_ARG;
    if ((sizes_scratch == nullptr) != (triggers_out == nullptr)) return GNNCCA_ERR_INVALID_ARG;
    if ((node_ptr_dev == nullptr) != (edge_ptr_dev == nullptr) || (node_ptr_dev != nullptr && n_frames == 0))
        return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    const size_t n_trig = (size_t)(node_ptr_dev ? n_frames : 1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_nodes == 0) return zero_post_counters(nullptr, nullptr, n_clusters_out, 0, nullptr, triggers_out, n_trig, st);
    if (!workspace || !flow_out || !flow_in || !labels_out || !n_clusters_out) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!edge_index || !predictions || !pruned_out)) return GNNCCA_ERR_INVALID_ARG;
    const PostWorkspace ws = carve_post(n_nodes, n_edges);
    if (!plan && workspace_bytes < ws.total) return GNNCCA_ERR_WORKSPACE;
    const int N = (int)n_nodes, E = (int)n_edges;
    const PostPlanPtrs own = post_plan_ptrs(workspace, ws);
    // (with `plan`: the MPN forward's plan of the same edge_index, nothing to build here)
    const int* seg_ptr = plan ? plan->seg_ptr : own.seg_ptr;
    const int* col32 = plan ? plan->col32 : own.col32;
    const int* perm = plan ? plan->perm : own.perm;
    const unsigned* flags = plan ? plan->flags : own.flags;
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    const long long* pred = reinterpret_cast<const long long*>(predictions);
    long long* pruned = reinterpret_cast<long long*>(pruned_out);
    if (!(plan && plan->counters_zeroed))   // (else: done launches ago)
        if (const int rc = zero_post_counters(flow_out, flow_in, n_clusters_out, (size_t)N, sizes_scratch, triggers_out, n_trig, st)) return rc;
    if (!plan)   // (kFinish: this entry's finish runs without edges too, so the workspace always holds a finished plan afterwards)
        if (const int rc = launch_post_plan(ei, E, N, own, EmptyPlan::kFinish, st)) return rc;
    if (E > 0) {
        if (plan && plan->logits)
            hipLaunchKernelGGL(post_prune_kernel<true>, grid1((size_t)E, 256), dim3(256), 0, st, ei, pred, (long long)E, seg_ptr, col32, perm, flags,
                               pruned, flow_out, flow_in, plan->logits, plan->probs_out, reinterpret_cast<long long*>(plan->preds_out));
        else
            hipLaunchKernelGGL(post_prune_kernel<false>, grid1((size_t)E, 256), dim3(256), 0, st, ei, pred, (long long)E, seg_ptr, col32, perm, flags,
                               pruned, flow_out, flow_in, (const float*)nullptr, (float*)nullptr, (long long*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(post_cc_kernel, dim3(node_ptr_dev ? (unsigned)n_frames : 1u), dim3(1024), 0, st, ei,
                       (const long long*)pruned, (long long)E, N, node_ptr_dev, edge_ptr_dev, labels_out, n_clusters_out,
                       (const int*)flow_out, (const int*)flow_in, sizes_scratch, triggers_out);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_post_prune_cluster(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes, int64_t n_edges,
                              void* workspace, size_t workspace_bytes, int64_t* pruned_out, int32_t* flow_out,
                              int32_t* flow_in, int32_t* labels_out, int32_t* n_clusters_out, gnncca_stream_t stream) {
    return post_prune_cluster_impl(edge_index, predictions, n_nodes, n_edges, nullptr, nullptr, 0, workspace, workspace_bytes, pruned_out, flow_out,
                                   flow_in, labels_out, n_clusters_out, nullptr, nullptr, nullptr, stream);
}

int gnncca_post_prune_cluster_frames(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes, int64_t n_edges,
                                     const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames, void* workspace,
                                     size_t workspace_bytes, int64_t* pruned_out, int32_t* flow_out, int32_t* flow_in, int32_t* labels_out,
                                     int32_t* n_clusters_out, gnncca_stream_t stream) {
    return post_prune_cluster_impl(edge_index, predictions, n_nodes, n_edges, node_ptr_dev, edge_ptr_dev, n_frames, workspace, workspace_bytes,
                                   pruned_out, flow_out, flow_in, labels_out, n_clusters_out, nullptr, nullptr, nullptr, stream);
}

int gnncca_post_prune_cluster_frames_ex(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes, int64_t n_edges,
                                        const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames, void* workspace,
                                        size_t workspace_bytes, int64_t* pruned_out, int32_t* flow_out, int32_t* flow_in,
                                        int32_t* labels_out, int32_t* n_clusters_out, int32_t* sizes_scratch, int32_t* triggers_out,
                                        gnncca_stream_t stream) {
    return post_prune_cluster_impl(edge_index, predictions, n_nodes, n_edges, node_ptr_dev, edge_ptr_dev, n_frames, workspace, workspace_bytes,
                                   pruned_out, flow_out, flow_in, labels_out, n_clusters_out, sizes_scratch, triggers_out, nullptr, stream);
}

// The argument checks the exclusive and the strong entry share: GNNCCA_ERR_INVALID_ARG for a negative count or a max_frame_nodes outside
// [0, min(limit, n_nodes)], else GNNCCA_ERR_UNSUPPORTED for 2^31 - 64 nodes or edges and more, else GNNCCA_OK.  Seen from outside the
// second refusal comes after the entry's own null-pointer checks: an entry returns the first at once and the second after those.
static int check_frames_args(int64_t n_nodes, int64_t n_edges, int32_t n_frames, int32_t max_frame_nodes, int limit) {
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > limit || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    return GNNCCA_OK;
}

// ---- camera-exclusive identity clusters (exclusive.cuh) -----------------------------------------------------------------------------------
// workspace: [the graph plan, as gnncca_post_workspace_bytes lays it out | rev int32 [E] | candidate keys u64 [E]]
struct ExclWorkspace { PostWorkspace plan; size_t rev, cand, total; };
static ExclWorkspace carve_excl(int64_t n, int64_t e, int64_t g) {
    ExclWorkspace w;
    w.plan = carve_post(n, e);
    size_t off = w.plan.total;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t E = (size_t)(e > 0 ? e : 0);
    w.rev = take(E * 4), w.cand = take(E * 8), w.total = off;
    return w;
}

size_t gnncca_post_exclusive_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames) {
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0) return 0;
    return carve_excl(n_nodes, n_edges, n_frames).total;
}

int gnncca_post_exclusive_frames(const int64_t* edge_index, const float* scores, int64_t n_nodes, int64_t n_edges, const int32_t* cam,
                                 const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_nodes,
                                 double threshold, int64_t* predictions_out, int32_t* labels_out, int32_t* n_clusters_out, int32_t* cut_out,
                                 uint32_t* flags_out, void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    const int args = check_frames_args(n_nodes, n_edges, n_frames, max_frame_nodes, kExclMaxNodes);
    if (args == GNNCCA_ERR_INVALID_ARG) return args;
    if (!(threshold > 0.0 && threshold < 1.0)) return GNNCCA_ERR_INVALID_ARG;   // (a NaN included)
    if (!n_clusters_out) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0 && n_nodes > 0) return GNNCCA_ERR_INVALID_ARG;
    if (args) return args;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_frames == 0) {   // nothing to cluster: the zero alone
        hipLaunchKernelGGL(excl_prepare_kernel, dim3(1), dim3(256), 0, st, (const long long*)nullptr, 0ll, (const int*)nullptr, (const int*)nullptr,
                           (const int*)nullptr, (const unsigned*)nullptr, (int*)nullptr, n_clusters_out);
        HIP_TRY(hipGetLastError());
        return GNNCCA_OK;
    }
    if (!node_ptr_dev || !edge_ptr_dev || !cut_out || !flags_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!cam || !labels_out)) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!edge_index || !scores || !predictions_out)) return GNNCCA_ERR_INVALID_ARG;
    const ExclWorkspace ws = carve_excl(n_nodes, n_edges, n_frames);
    if (workspace_bytes < ws.total) return GNNCCA_ERR_WORKSPACE;
    const int N = (int)n_nodes, E = (int)n_edges;
    char* base = static_cast<char*>(workspace);
    const PostPlanPtrs plan = post_plan_ptrs(workspace, ws.plan);
    int* rev = reinterpret_cast<int*>(base + ws.rev);
    excl_u64* cand = reinterpret_cast<excl_u64*>(base + ws.cand);
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    const int P = frame_capacity(max_frame_nodes);
    const auto lds_at = [](size_t nodes) { return nodes * (2 * sizeof(excl_u64) + sizeof(int)) + 8 * sizeof(int); };
    const size_t lds = lds_at(P);
    if (lds > 64 * 1024) HIP_TRY(lds_opt_in<excl_cluster_kernel<256>>(lds_at(kExclMaxNodes)));
    if (const int rc = launch_post_plan(ei, E, N, plan, EmptyPlan::kSkip, st)) return rc;
    // the reverse edges, and *n_clusters_out = 0 (kernels only on the stream: no memset)
    hipLaunchKernelGGL(excl_prepare_kernel, grid1((size_t)std::max(E, 1), 256), dim3(256), 0, st, ei, (long long)E, (const int*)plan.seg_ptr,
                       (const int*)plan.col32, (const int*)plan.perm, (const unsigned*)plan.flags, rev, n_clusters_out);
    HIP_TRY(hipGetLastError());
    long long* preds = reinterpret_cast<long long*>(predictions_out);
    launch_frame_block(P, [&](auto block) {
        constexpr int B = decltype(block)::value;
        hipLaunchKernelGGL((excl_cluster_kernel<B>), dim3((unsigned)n_frames), dim3(B), lds, st, ei, (long long)E, scores, threshold, cam,
                           (const int*)rev, cand, N, node_ptr_dev, edge_ptr_dev, P, preds, labels_out, n_clusters_out, cut_out, flags_out);
    });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

// ---- identity clusters without pruning: strongly connected components (strong.cuh) ---------------------------------------------------------
int gnncca_post_strong_frames(const int64_t* edge_index, const int64_t* predictions, int64_t n_nodes, int64_t n_edges,
                              const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_nodes,
                              int32_t* flow_out, int32_t* flow_in, int32_t* labels_out, int32_t* n_clusters_out, int32_t* triggers_out,
                              uint32_t* flags_out, gnncca_stream_t stream) {
    const int args = check_frames_args(n_nodes, n_edges, n_frames, max_frame_nodes, kStrongMaxNodes);
    if (args == GNNCCA_ERR_INVALID_ARG) return args;
    if ((node_ptr_dev == nullptr) != (edge_ptr_dev == nullptr) || (node_ptr_dev == nullptr) != (n_frames == 0)) return GNNCCA_ERR_INVALID_ARG;
    if (!n_clusters_out || !triggers_out || !flags_out) return GNNCCA_ERR_INVALID_ARG;   // (one trigger / flag word at least: the whole graph)
    if (n_nodes > 0 && (!flow_out || !flow_in || !labels_out)) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!edge_index || !predictions)) return GNNCCA_ERR_INVALID_ARG;
    if (args) return args;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (the kernel writes every trigger word itself and keeps its sizes in LDS: the flows and the count alone)
    if (const int rc = zero_post_counters(flow_out, flow_in, n_clusters_out, (size_t)n_nodes, nullptr, nullptr, 0, st)) return rc;
    const int P = strong_capacity(max_frame_nodes);            // the LDS capacity in nodes: rows of P / 32 words
    const size_t lds = (size_t)P * (size_t)(P / 32) * 4;       // 128 B at 32, 2 KiB at 128, 128 KiB at 1024
    if (lds > 64 * 1024) HIP_TRY(lds_opt_in<strong_cluster_kernel<1024>>((size_t)kStrongMaxNodes * (kStrongMaxNodes / 32) * 4));
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    const long long* pred = reinterpret_cast<const long long*>(predictions);
    // the block covers the largest frame with one node per thread: one wave for Terrace-sized frames (~20 detections), 1024 threads only
    // where a frame needs them
    launch_frame_block<1024>(P, [&](auto block) {
        constexpr int B = decltype(block)::value;
        hipLaunchKernelGGL((strong_cluster_kernel<B>), dim3(node_ptr_dev ? (unsigned)n_frames : 1u), dim3(B), lds, st, ei, pred, (long long)n_edges,
                           (int)n_nodes, node_ptr_dev, edge_ptr_dev, P, flow_out, flow_in, labels_out, n_clusters_out, triggers_out, flags_out);
    });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

// The one-call chain of gnncca_frames_forward (the complete graph), gnncca_frames_forward_topk (the staging image and n_edges are
// gnncca_plan_frames_ex(top_k)'s, the build is the capped kernel) and gnncca_frames_forward_radius (the image and n_edges are
// gnncca_plan_frames_radius', the build is the gated kernel), by `sel`.  Everything after the build sees an ordinary edge list.
static int frames_forward_impl(const gnncca_mpn_dims* d, const void* packed_dev, const gnncca_frames_io* io, void* mpn_workspace,
                               size_t mpn_workspace_bytes, void* post_workspace, size_t post_workspace_bytes, uint32_t options,
                               const EdgeSelect& sel, gnncca_stream_t stream) {
    if (const int bad = edge_select_refusal(sel)) return bad;
    if (!d || !io || !io->staged_dev) return GNNCCA_ERR_INVALID_ARG;
    const int64_t n = io->n_nodes, g = io->n_frames, e = io->n_edges;
    if (n < 1 || g < 1 || e < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n > 4096) return GNNCCA_ERR_UNSUPPORTED;   // (the one-launch normalisation's limit; bigger batches take the separate entry points)
    if (!io->node_embeds || !io->reid_embeds || !io->edge_index || !io->edge_attr || !io->edge_labels || !io->logits || !io->probs ||
        !io->predictions || !io->pruned || !io->counters || !io->labels || (io->normalize && (!io->node_norm || !io->reid_norm)))
        return GNNCCA_ERR_INVALID_ARG;
    if (io->counters_len < 3 * n + 1 + g) return GNNCCA_ERR_INVALID_ARG;   // flow_out | flow_in | n_clusters | sizes | triggers (ABI 2: stated, not assumed)
    // (what gnncca_build_edges_topk / _radius would refuse, refused here: before the normalisation's launch)
    if (sel.kind != EdgeSelect::kDense && (io->mode < GNNCCA_EDGE_ATTR_FULL || io->mode > GNNCCA_EDGE_ATTR_ONLY_DIST)) return GNNCCA_ERR_INVALID_ARG;
    if (sel.kind == EdgeSelect::kCapped && sel.rank_by == GNNCCA_RANK_BY_REID && io->reid_dim <= 0)
        return GNNCCA_ERR_INVALID_ARG;   // the ranking reads the table in every mode
    const StagingImage img = staging_image(io->staged_dev, n, g);
    const gnncca_frames fr = img.frames();
    const float* x = io->node_embeds;
    const float* reid = io->reid_embeds;
    int st = GNNCCA_OK;
    if (io->normalize) {
        st = gnncca_normalize_columns2(io->reid_embeds, io->reid_dim, io->reid_norm, io->node_embeds, d->node_in, io->node_norm, n, stream);
        if (st != GNNCCA_OK) return st;
        x = io->node_norm, reid = io->reid_norm;
    }
    // (the post stage's counters -- flow_out | flow_in | n_clusters | sizes | triggers -- are zeroed by this launch: no memset node later)
    const bool zero_here = e > 0 && mpn_workspace != nullptr;
    int32_t* zero_ptr = zero_here ? io->counters : nullptr;
    const int64_t zero_n = zero_here ? 3 * n + 1 + g : 0;
    st = build_edges_zeroing(&fr, reid, io->reid_dim, n, e, io->mode, sel, io->edge_index, io->edge_attr, io->edge_labels, zero_ptr, zero_n, stream);
    if (st != GNNCCA_OK) return st;
    const int n_out = gnncca_num_outputs(d);
    if (n_out < 1) return GNNCCA_ERR_UNSUPPORTED;
    if (e > 0) {
        st = gnncca_mpn_forward_ex(d, packed_dev, x, io->edge_index, io->edge_attr, n, e, mpn_workspace, mpn_workspace_bytes, io->logits, nullptr,
                                   options, stream);
        if (st != GNNCCA_OK) return st;
        if (!zero_here) {   // (no shared plan: the threshold keeps its own launch)
            st = gnncca_post_threshold(io->logits + (size_t)(n_out - 1) * e, e, io->probs, io->predictions, stream);
            if (st != GNNCCA_OK) return st;
        }
    }
    // the pruning searches reverse edges in the CSR plan of edge_index -- the one the forward above left in ITS workspace (seg_ptr / col32 /
    // perm / flag word: same plan_block + plan_finish, same stream): handed over instead of being built a second time (two launches less)
    PostPlan plan;
    const PostPlan* have_plan = nullptr;
    if (e > 0 && mpn_workspace) {
        plan = forward_plan(d, mpn_workspace, n, e);
        plan.counters_zeroed = zero_here;
        plan.logits = io->logits + (size_t)(n_out - 1) * e, plan.probs_out = io->probs, plan.preds_out = io->predictions;
        have_plan = &plan;
    }
    int32_t* c = io->counters;   // flow_out | flow_in | n_clusters | sizes (scratch) | triggers [G]
    return post_prune_cluster_impl(io->edge_index, io->predictions, n, e, fr.graph_ptr, img.edge_ptr_g, (int32_t)g, post_workspace, post_workspace_bytes,
                                   io->pruned, c, c + n, io->labels, c + 2 * n, c + 2 * n + 1, c + 3 * n + 1, have_plan, stream);
}

int gnncca_frames_forward(const gnncca_mpn_dims* d, const void* packed_dev, const gnncca_frames_io* io, void* mpn_workspace,
                          size_t mpn_workspace_bytes, void* post_workspace, size_t post_workspace_bytes, uint32_t options,
                          gnncca_stream_t stream) {
    return frames_forward_impl(d, packed_dev, io, mpn_workspace, mpn_workspace_bytes, post_workspace, post_workspace_bytes, options, EdgeSelect::dense(),
                               stream);
}

int gnncca_frames_forward_topk(const gnncca_mpn_dims* d, const void* packed_dev, const gnncca_frames_io* io, void* mpn_workspace,
                               size_t mpn_workspace_bytes, void* post_workspace, size_t post_workspace_bytes, uint32_t options,
                               int32_t top_k, int32_t rank_by, int32_t max_deg, gnncca_stream_t stream) {
    return frames_forward_impl(d, packed_dev, io, mpn_workspace, mpn_workspace_bytes, post_workspace, post_workspace_bytes, options,
                               EdgeSelect::capped(top_k, rank_by, max_deg), stream);
}

int gnncca_frames_forward_radius(const gnncca_mpn_dims* d, const void* packed_dev, const gnncca_frames_io* io, void* mpn_workspace,
                                 size_t mpn_workspace_bytes, void* post_workspace, size_t post_workspace_bytes, uint32_t options,
                                 double radius, int32_t unit, gnncca_stream_t stream) {
    return frames_forward_impl(d, packed_dev, io, mpn_workspace, mpn_workspace_bytes, post_workspace, post_workspace_bytes, options,
                               EdgeSelect::gated(radius, unit), stream);
}

}  // extern "C"
