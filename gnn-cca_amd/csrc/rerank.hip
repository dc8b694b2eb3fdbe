// rerank.hip -- the C entries of the rank-R ReID baseline (rerank.cuh has the kernels and what they compute): gnncca_frame_distances,
// gnncca_rerank_frames, gnncca_rank_predictions.  One launch each on the caller's stream, no host synchronisation, no allocation:
// capturable.  The whole unit is compiled without fp contraction: the re-ranking's fp32 expressions are the reference's, operation for
// operation, and tests/rerank_oracle.py writes the same ones in numpy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hip_try.h"

#pragma clang fp contract(off)

#include "rerank.cuh"

using namespace gnncca;

static bool frames_ok(int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, int64_t total) {
    return n_nodes >= 0 && n_frames >= 0 && max_frame_nodes >= 0 && max_frame_nodes <= n_nodes && total >= 0 &&
           n_nodes < (1ll << 31) - 64;
}

extern "C" {

int gnncca_frame_distances(const float* embeds, int32_t dim, int64_t n_nodes, const int32_t* node_ptr_dev, int32_t n_frames,
                           int32_t max_frame_nodes, int64_t total, float* out, gnncca_stream_t stream) {
    if (!frames_ok(n_nodes, n_frames, max_frame_nodes, total) || dim < 1) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0 || max_frame_nodes == 0 || total == 0) return GNNCCA_OK;
    if (!embeds || !node_ptr_dev || !out) return GNNCCA_ERR_INVALID_ARG;
    const int64_t tiles = ((int64_t)max_frame_nodes + kDistTile - 1) / kDistTile;
    if (tiles > 65535) return GNNCCA_ERR_UNSUPPORTED;   // (a frame of more than a million detections)
    hipLaunchKernelGGL(frame_distances_kernel, dim3((unsigned)n_frames, (unsigned)tiles, (unsigned)tiles), dim3(256), 0,
                       static_cast<hipStream_t>(stream), embeds, (int)dim, (int)n_nodes, node_ptr_dev, (long long)total, out);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

size_t gnncca_rerank_lds_bytes(int32_t max_frame_nodes, int32_t k1, int32_t k2) {
    if (max_frame_nodes < 0 || max_frame_nodes > kRerankMaxNodes || k1 < 1 || k1 > kRerankMaxK1 || k2 < 1 || k2 > k1) return 0;
    return rerank_lds(max_frame_nodes, k1, k2).total;
}

int gnncca_rerank_frames(const float* dist, int64_t total, int64_t n_nodes, const int32_t* node_ptr_dev, int32_t n_frames,
                         int32_t max_frame_nodes, int32_t k1, int32_t k2, double lam, float* out, int32_t* rank_out, int32_t rank_cols,
                         uint64_t* mask_out, gnncca_stream_t stream) {
    if (!frames_ok(n_nodes, n_frames, max_frame_nodes, total)) return GNNCCA_ERR_INVALID_ARG;
    if (k1 < 1 || k1 > kRerankMaxK1 || k2 < 1 || k2 > k1 || !(lam >= 0.0 && lam <= 1.0)) return GNNCCA_ERR_INVALID_ARG;
    if (rank_out && rank_cols < 1) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes > kRerankMaxNodes) return GNNCCA_ERR_UNSUPPORTED;
    if (n_frames == 0 || max_frame_nodes == 0 || total == 0) return GNNCCA_OK;
    if (!dist || !node_ptr_dev || !out) return GNNCCA_ERR_INVALID_ARG;
    const int P = max_frame_nodes;
    const size_t lds = rerank_lds(P, k1, k2).total;
    const bool big = P > 64;   // 16 waves share the one workgroup a CU holds at that size; small frames take 4 and several fit
    if (lds > 64 * 1024) {     // (both forms: either may be the one launched below)
        const size_t most = rerank_lds(kRerankMaxNodes, kRerankMaxK1, kRerankMaxK1).total;
        HIP_TRY((lds_opt_in<rerank_frames_kernel<1024, false>>(most)));
        HIP_TRY((lds_opt_in<rerank_frames_kernel<1024, true>>(most)));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float lam32 = (float)lam, one_minus = (float)(1.0 - lam);   // the reference's python floats, rounded once as numpy rounds them
    unsigned long long* mo = reinterpret_cast<unsigned long long*>(mask_out);
#define GNNCCA_RERANK(B, G)                                                                                                            \
    hipLaunchKernelGGL((rerank_frames_kernel<B, G>), dim3((unsigned)n_frames), dim3(B), lds, st, dist, (long long)total, (int)n_nodes,     \
                       node_ptr_dev, P, (int)k1, (int)k2, lam32, one_minus, out, rank_out, (int)rank_cols, mo)
    const bool debug = rank_out || mask_out;
    if (big) {
        if (debug) GNNCCA_RERANK(1024, true); else GNNCCA_RERANK(1024, false);
    } else {
        if (debug) GNNCCA_RERANK(256, true); else GNNCCA_RERANK(256, false);
    }
#undef GNNCCA_RERANK
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_rank_predictions(const float* dist, int64_t total, const int32_t* cam, int64_t n_nodes, const int64_t* edge_index,
                            int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                            int32_t max_frame_nodes, int32_t rank, int64_t* predictions, gnncca_stream_t stream) {
    if (!frames_ok(n_nodes, n_frames, max_frame_nodes, total) || n_edges < 0 || rank < 1) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes > kRerankMaxNodes) return GNNCCA_ERR_UNSUPPORTED;
    if (n_frames == 0 || n_edges == 0) return GNNCCA_OK;
    if (!node_ptr_dev || !edge_ptr_dev || !edge_index || !predictions) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!dist || !cam)) return GNNCCA_ERR_INVALID_ARG;
    hipLaunchKernelGGL((rank_predictions_kernel<256>), dim3((unsigned)n_frames), dim3(256), 0, static_cast<hipStream_t>(stream), dist,
                       (long long)total, cam, (int)n_nodes, reinterpret_cast<const long long*>(edge_index), (long long)n_edges, node_ptr_dev,
                       edge_ptr_dev, (int)rank, reinterpret_cast<long long*>(predictions));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
