// evaluate.hip -- the per-frame scoring of the reference's evaluation loop on gfx950 (inference.py:349-371): the edge confusion counts and
// P / R / F / per-class precisions of `compute_P_R_F` (inference.py:23-68), and ARI, AMI, homogeneity, completeness and V-measure between
// ID_GT (the components of the ground-truth-active edges, inference.py:296-299) and the predicted partition -- the numbers main.py:335-348
// averages.  The formulas and special cases are scikit-learn 1.7.2's (metrics/cluster/_supervised.py, _expected_mutual_info_fast.pyx).
//
// One workgroup per frame (frames are independent), everything frame-local in LDS:
//   1. edge counts (integers) and the GT partition in ONE pass over the edges: union-find over the edges with label 1 (the larger root
//      hooked under the smaller by compare-and-swap, then pointer jumping; the root of a component is its smallest node);
//   2. cluster sizes a_i (GT) and b_j (predicted) as one LDS histogram of packed 16-bit counts, and the contingency cells n_ij as runs of
//      the sorted 24-bit keys (gt_root << 12 | pred_root) (bitonic sort in LDS);
//   3. entropies, MI and the pair counts of ARI from the sizes and the cells;
//   4. the expected mutual information over DISTINCT cluster sizes with their multiplicities (a term depends on the two sizes only; a
//      frame of n nodes has at most ~sqrt(2 n) distinct sizes per side), each term table lookups into lf[k] = lgamma(k + 1) plus one
//      log and one exp.  The table lives in the caller's workspace ((n_g + 1) doubles per frame).
// LDS: 3 x P int32 (P = the batch's largest frame rounded up to a power of two: 48 KiB at 4096 nodes) + ~2 KiB.
// Deterministic: integer sums through LDS atomics, fp64 sums per lane in a fixed order, then a butterfly per wave and the waves in order.
// No fp64 atomics.  The whole file is compiled without fp contraction: the counts, P, R, F, the precisions and ARI are the reference's
// expressions operation for operation (bit-identical), and no multiply-add may fuse them.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "hip_try.h"
#include "plan.cuh"   // plan_num_blocks: the sweep builds the graph plan through internal.h's launchers

#pragma clang fp contract(off)

namespace gnncca {

constexpr int kEvalMaxNodes = GNNCCA_EVAL_MAX_FRAME_NODES;   // 12-bit frame-local ids in the contingency keys
constexpr int kEvalMaxSizes = 96;   // distinct cluster sizes of one side: k (k + 1) / 2 <= 4096  ->  k <= 90
constexpr double kEps = 2.220446049250313e-16;   // np.finfo(np.float64).eps

// integer accumulators of a frame (LDS atomics: order-independent)
enum { I_TP, I_FP, I_TN, I_FN, I_C1, I_C0, I_SSQ, I_SA2, I_SB2, I_KA, I_KB, I_NGT, I_NPRED, I_D1, I_D0, I_COUNT };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);   // every lane ends with the same bits (a + b == b + a)
    return v;
}

// sum over the block in a fixed order: butterfly per wave, then the waves in order (every thread gets the result)
template <int BLOCK>
__device__ __forceinline__ double block_sum(double v, double* scratch) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = scratch[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) s += scratch[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// A frame's lgamma table, lf[k] = lgamma(k + 1) for k <= n: the one loop of every writer (eval_frame_body<.., FILL_LF = true> and the
// sweeps' prepare kernels), so the table has the same bits whoever wrote it.  `stride`: the workgroup's threads.
__device__ __forceinline__ void fill_lgamma_table(double* lf, int n, int tid, int stride) {
    for (int k = tid; k <= n; k += stride) lf[k] = lgamma((double)k + 1.0);
}

// out[g][16] = P, R, F, TP, FP, FN, TN, ARI, AMI, homogeneity, completeness, V, precision0, precision1, n_clusters_gt, n_clusters_pred.
// P_lds: ints per LDS region (a power of two >= every frame's node count, <= kEvalMaxNodes).  lf_ws: the lgamma tables, frame g's at
// lf_ws + node_ptr[g] + g.  A frame whose ranges do not fit (node count above P_lds, ranges outside the arrays) gets a NaN row.
// DENSE (gnncca_eval_frames_dense): the batch is a capped graph, scored as the dense graph with every dropped edge predicted 0.  The GT
// partition then comes from the person ids and cameras, not from the kept edges: thread v walks the frame (person / cam staged in the LDS
// regions steps 2-3 use later) for the smallest detection with v's identity, whether that identity is on another camera too (then the
// dense graph's label-1 edges join all its detections: any two on one camera meet through one on another), and v's dense out-degree per
// class, whose sums minus the kept edges of the class are the dropped pairs: FN += D1 - C1, TN += D0 - C0.  n^2 / BLOCK LDS reads per
// thread (64 k at 4096 nodes).  person / cam are null otherwise and nothing of this runs: the instantiation is the kernel as it was.
// The body is written once for every caller (eval_frame_body): it asks "is edge k predicted" (`pred(k)`: 1 / 0, as the int64 prediction)
// and "the label of the frame's node v" (`label(v0, v)`: a batch-global node id) through two small functors, so that the kernels below read
// them from two global arrays and the threshold sweep (eval_sweep.cuh) from scores and LDS -- the arithmetic is the same text.
// FILL_LF: the workgroup writes its frame's lgamma table itself (false: an earlier launch did, with the same expression).
struct GlobalPred {
    const long long* __restrict__ pred;
    __device__ __forceinline__ long long operator()(long long k) const { return pred[k]; }
};
struct GlobalLabel {
    const int* __restrict__ labels;
    __device__ __forceinline__ int operator()(int v0, int v) const { return labels[v0 + v]; }
};

template <int BLOCK, bool DENSE, bool FILL_LF, class PredF, class LabelF>
__device__ __forceinline__ void eval_frame_body(const int g, double* __restrict__ row, const long long* __restrict__ ei, long long E,
                                                const float* __restrict__ elab, const PredF pred, const LabelF label, int N_all,
                                                const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int P_lds,
                                                int* __restrict__ gt_out, double* __restrict__ lf_ws, const int* __restrict__ person,
                                                const int* __restrict__ cam) {
    extern __shared__ int s_dyn[];
    __shared__ unsigned long long s_int[I_COUNT];
    __shared__ double s_red[BLOCK / 64];
    __shared__ int s_sa[kEvalMaxSizes], s_ma[kEvalMaxSizes], s_sb[kEvalMaxSizes], s_mb[kEvalMaxSizes];
    __shared__ int s_na, s_nb;
    int* parent = s_dyn;                                             // union-find, later the histogram of cluster sizes
    unsigned* cnt = reinterpret_cast<unsigned*>(s_dyn + P_lds);       // per local root: a (bits 0-15) | b (bits 16-31)
    unsigned* keys = reinterpret_cast<unsigned*>(s_dyn + 2 * P_lds);  // contingency keys, sorted

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v0 = node_ptr[g], v1 = node_ptr[g + 1];
    const long long k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
    const int n = v1 - v0;
    if (v0 < 0 || n < 0 || n > P_lds || v1 > N_all || k0 < 0 || k1 < k0 || k1 > E) {
        if (tid < 16) row[tid] = __builtin_nan("");
        return;
    }
    double* lf = lf_ws + v0 + g;
    for (int v = tid; v < n; v += BLOCK) {
        parent[v] = v;
        cnt[v] = DENSE ? (unsigned)cam[v0 + v] : 0u;
        if (DENSE) keys[v] = (unsigned)person[v0 + v];
    }
    if (FILL_LF) fill_lgamma_table(lf, n, tid, BLOCK);   // read only after the barriers below
    if (tid < I_COUNT) s_int[tid] = 0;
    __syncthreads();
    if (DENSE) {
        unsigned long long d1 = 0, d0 = 0;
        for (int v = tid; v < n; v += BLOCK) {
            const unsigned pv = keys[v], cv = cnt[v];
            int first = v;
            unsigned same_other = 0, diff_other = 0;
            for (int u = 0; u < n; ++u) {
                const bool same = keys[u] == pv, other = cnt[u] != cv;
                first = same && u < first ? u : first;
                same_other += same && other;
                diff_other += !same && other;
            }
            parent[v] = same_other ? first : v;   // (roots point at themselves: `first` has the same identity and sees the same cameras)
            d1 += same_other;
            d0 += diff_other;
        }
        if (d1) atomicAdd(&s_int[I_D1], d1);
        if (d0) atomicAdd(&s_int[I_D0], d0);
        __syncthreads();
        for (int v = tid; v < n; v += BLOCK) cnt[v] = 0;
        __syncthreads();
    }

    // ---- 1. edge counts (compute_P_R_F) and the GT partition, one pass over the frame's edges ----------------------------------------
    // Union-find over the edges with label 1: a root is hooked under the smaller root by compare-and-swap (it fails when another thread
    // hooked that root first: find the new roots and retry), so one pass joins every GT edge's endpoints; pointer jumping then leaves
    // parent[v] = the smallest node of v's component.
    {
        unsigned tp = 0, fp = 0, tn = 0, fn = 0, c1 = 0, c0 = 0;
        for (long long k = k0 + tid; k < k1; k += BLOCK) {
            const long long a = ei[k] - v0, b = ei[E + k] - v0;
            if (a < 0 || a >= n || b < 0 || b >= n) continue;   // an edge that leaves its frame: ignored
            const float l = elab[k];
            const long long p = pred(k);
            if (l == 1.f) {
                ++c1;
                tp += p == 1;
                fn += p == 0;
                int ra = (int)a, rb = (int)b;
                while (!DENSE) {   // (DENSE: the partition is the dense graph's, made above)
                    for (int q = lds_load(&parent[ra]); q != ra; q = lds_load(&parent[ra])) ra = q;
                    for (int q = lds_load(&parent[rb]); q != rb; q = lds_load(&parent[rb])) rb = q;
                    if (ra == rb) break;
                    const int hi = max(ra, rb), lo = min(ra, rb);
                    if (atomicCAS(&parent[hi], hi, lo) == hi) break;
                }
            } else if (l == 0.f) {
                ++c0;
                fp += p == 1;
                tn += p == 0;
            }
        }
        if (c1) {
            atomicAdd(&s_int[I_C1], (unsigned long long)c1);
            atomicAdd(&s_int[I_TP], (unsigned long long)tp);
            atomicAdd(&s_int[I_FN], (unsigned long long)fn);
        }
        if (c0) {
            atomicAdd(&s_int[I_C0], (unsigned long long)c0);
            atomicAdd(&s_int[I_FP], (unsigned long long)fp);
            atomicAdd(&s_int[I_TN], (unsigned long long)tn);
        }
    }
    __syncthreads();
    for (int v = tid; v < n; v += BLOCK) {   // pointer jumping (the forest no longer grows: every write points at an ancestor)
        int r = v;
        for (int q = lds_load(&parent[r]); q != r; q = lds_load(&parent[r])) r = q;
        __hip_atomic_store(&parent[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();

    // ---- 2. sizes and contingency keys ---------------------------------------------------------------------------------------------
    int sort_n = 1;
    while (sort_n < n) sort_n <<= 1;
    {
        unsigned ngt = 0, npred = 0;
        for (int v = tid; v < n; v += BLOCK) {
            const int r = parent[v];
            const int lab = label(v0, v);
            int lp = lab - v0;
            if (lp < 0 || lp >= n) lp = v;   // outside the frame: the node's own cluster
            atomicAdd(&cnt[r], 1u);
            atomicAdd(&cnt[lp], 1u << 16);
            keys[v] = ((unsigned)r << 12) | (unsigned)lp;
            ngt += r == v;
            npred += lab == v0 + v;
            if (gt_out) gt_out[v0 + v] = v0 + r;
        }
        for (int v = n + tid; v < sort_n; v += BLOCK) keys[v] = 0xFFFFFFFFu;
        if (ngt) atomicAdd(&s_int[I_NGT], (unsigned long long)ngt);
        if (npred) atomicAdd(&s_int[I_NPRED], (unsigned long long)npred);
    }
    __syncthreads();
    for (int v = tid; v < n; v += BLOCK) parent[v] = 0;   // from here on: histogram of cluster sizes (a - 1: bits 0-15, b - 1: bits 16-31)
    for (int k = 2; k <= sort_n; k <<= 1) {               // bitonic sort of the keys
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < sort_n; i += BLOCK) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned x = keys[i], y = keys[l];
                    if ((x > y) == ((i & k) == 0)) {
                        keys[i] = y;
                        keys[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();

    // ---- 3. entropies, MI, pair counts ---------------------------------------------------------------------------------------------
    const double dn = (double)n, logn = log(dn);
    double hc = 0.0, hk = 0.0, mi = 0.0;
    {
        unsigned long long sa2 = 0, sb2 = 0, ssq = 0;
        unsigned ka = 0, kb = 0;
        for (int v = tid; v < n; v += BLOCK) {
            const unsigned c = cnt[v], a = c & 0xFFFFu, b = c >> 16;
            if (a) {   // entropy(labels_true): -sum((pi / pi_sum) * (log(pi) - log(pi_sum)))
                sa2 += (unsigned long long)a * a;
                hc += ((double)a / dn) * (log((double)a) - logn);
                ++ka;
                atomicAdd((unsigned*)&parent[a - 1], 1u);
            }
            if (b) {
                sb2 += (unsigned long long)b * b;
                hk += ((double)b / dn) * (log((double)b) - logn);
                ++kb;
                atomicAdd((unsigned*)&parent[b - 1], 1u << 16);
            }
        }
        for (int p = tid; p < n; p += BLOCK) {   // one thread per contingency cell: the first position of its run of keys
            const unsigned key = keys[p];
            if (p > 0 && keys[p - 1] == key) continue;
            int lo = p + 1, hi = n;   // end of the run
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (keys[mid] == key) lo = mid + 1;
                else hi = mid;
            }
            const int nij = lo - p;
            ssq += (unsigned long long)nij * nij;
            const unsigned a = cnt[key >> 12] & 0xFFFFu, b = cnt[key & 0xFFFu] >> 16;
            // mutual_info_score: cnm * (log(nij) - log(N)) + cnm * (-log(a b) + log(N) + log(N)), |term| < eps -> 0
            const double cnm = (double)nij / dn;
            const double log_outer = -log((double)((unsigned long long)a * b)) + logn + logn;
            double t = cnm * (log((double)nij) - logn) + cnm * log_outer;
            if (fabs(t) < kEps) t = 0.0;
            mi += t;
        }
        if (sa2) atomicAdd(&s_int[I_SA2], sa2);
        if (sb2) atomicAdd(&s_int[I_SB2], sb2);
        if (ssq) atomicAdd(&s_int[I_SSQ], ssq);
        if (ka) atomicAdd(&s_int[I_KA], (unsigned long long)ka);
        if (kb) atomicAdd(&s_int[I_KB], (unsigned long long)kb);
    }
    hc = block_sum<BLOCK>(hc, s_red);   // (its barriers also publish the histograms and counters)
    hk = block_sum<BLOCK>(hk, s_red);
    mi = block_sum<BLOCK>(mi, s_red);
    const unsigned ka = (unsigned)s_int[I_KA], kb = (unsigned)s_int[I_KB];

    // ---- 4. expected mutual information over distinct sizes ------------------------------------------------------------------------
    if (wave == 0) {   // compaction of the size histogram, in size order
        int na = 0, nb = 0;
        const unsigned long long below = (1ull << lane) - 1;
        for (int base = 0; base < n; base += 64) {
            const int s = base + lane;
            const unsigned h = s < n ? (unsigned)parent[s] : 0u, ha = h & 0xFFFFu, hb = h >> 16;
            const unsigned long long ma = __ballot(ha != 0), mb = __ballot(hb != 0);
            const int pa = na + __popcll(ma & below), pb = nb + __popcll(mb & below);
            if (ha && pa < kEvalMaxSizes) {
                s_sa[pa] = s + 1;
                s_ma[pa] = (int)ha;
            }
            if (hb && pb < kEvalMaxSizes) {
                s_sb[pb] = s + 1;
                s_mb[pb] = (int)hb;
            }
            na += __popcll(ma);
            nb += __popcll(mb);
        }
        if (lane == 0) {
            s_na = min(na, kEvalMaxSizes);
            s_nb = min(nb, kEvalMaxSizes);
        }
    }
    __threadfence_block();   // lf (global) and the lists (LDS) of every thread are visible after the barrier
    __syncthreads();
    double emi = 0.0;
    if (ka > 1 && kb > 1) {
        const int na = s_na, nb = s_nb;
        const double lfn = lf[n];
        double acc = 0.0;
        for (int q = wave; q < na * nb; q += BLOCK / 64) {
            const int i = q / nb, j = q - (q / nb) * nb;
            const int a = s_sa[i], b = s_sb[j];
            const double w = (double)s_ma[i] * (double)s_mb[j];
            const double la = log((double)a), lb = log((double)b);
            const double glnab = lf[a] + lf[b] + lf[n - a] + lf[n - b];
            const int start = max(1, a - n + b), end = min(a, b) + 1;
            for (int nij = start + lane; nij < end; nij += 64) {
                const double term1 = (double)nij / dn;
                const double term2 = (logn + log((double)nij)) - la - lb;
                const double gln = glnab - (lf[nij] + lfn) - lf[a - nij] - lf[b - nij] - lf[n - a - b + nij];
                acc += w * (term1 * term2 * exp(gln));
            }
        }
        emi = block_sum<BLOCK>(acc, s_red);
    }

    // ---- the row ------------------------------------------------------------------------------------------------------------------
    if (tid != 0) return;
    unsigned long long TP = s_int[I_TP], FP = s_int[I_FP], TN = s_int[I_TN], FN = s_int[I_FN], C1 = s_int[I_C1], C0 = s_int[I_C0];
    if (DENSE) {   // the dropped ordered pairs of each class: predicted 0
        const unsigned long long D1 = s_int[I_D1], D0 = s_int[I_D0];
        if (D1 > C1) FN += D1 - C1, C1 = D1;
        if (D0 > C0) TN += D0 - C0, C0 = D0;
    }
    // compute_P_R_F, expression for expression
    const double P = (TP + FP) != 0 ? (double)TP / (double)(TP + FP) : 0.0;
    const double R = (TP + FN) != 0 ? (double)TP / (double)(TP + FN) : 0.0;
    const double PR = P * R;
    const double F = (P + R) != 0.0 ? 2.0 * PR / (P + R) : 0.0;
    const double prec1 = TP != 0 ? ((double)TP / (double)C1) * 100.0 : 0.0;
    const double prec0 = TN != 0 ? ((double)TN / (double)C0) * 100.0 : 0.0;
    // adjusted_rand_score from pair_confusion_matrix (all integers below 2^53 at 4096 nodes: exact)
    const long long nn = n, ssq = (long long)s_int[I_SSQ];
    const long long c11 = ssq - nn, c01 = (long long)s_int[I_SB2] - ssq, c10 = (long long)s_int[I_SA2] - ssq;
    const long long c00 = nn * nn - c01 - c10 - ssq;
    double ari = 1.0;
    if (!(c10 == 0 && c01 == 0)) {
        const long long num = c11 * c00 - c10 * c01;
        const long long den = (c11 + c10) * (c10 + c00) + (c11 + c01) * (c01 + c00);
        ari = 2.0 * (double)num / (double)den;
    }
    // homogeneity_completeness_v_measure (beta = 1) and adjusted_mutual_info_score (arithmetic)
    double h = 1.0, c = 1.0, vm = 1.0, ami = 1.0;
    if (n > 0) {
        const double HC = ka == 1 ? 0.0 : -hc, HK = kb == 1 ? 0.0 : -hk;
        const double MI = (ka == 1 || kb == 1) ? 0.0 : (mi > 0.0 ? mi : 0.0);
        h = HC != 0.0 ? MI / HC : 1.0;
        c = HK != 0.0 ? MI / HK : 1.0;
        const double hc2 = 2.0 * h;
        vm = h + c == 0.0 ? 0.0 : hc2 * c / (h + c);
        if (ka == 1 && kb == 1) {
            ami = 1.0;
        } else if (ka == 1 || kb == 1) {
            ami = 0.0;
        } else {
            const double normalizer = (HC + HK) / 2.0;
            double den = normalizer - emi;
            den = den < 0.0 ? fmin(den, -kEps) : fmax(den, kEps);
            double num = MI - emi;
            num = num < 0.0 ? fmin(num, -kEps) : fmax(num, kEps);
            ami = num / den;
        }
    }
    const double vals[16] = {P, R, F, (double)TP, (double)FP, (double)FN, (double)TN, ari, ami, h, c, vm, prec0, prec1,
                             (double)s_int[I_NGT], (double)s_int[I_NPRED]};
#pragma unroll
    for (int q = 0; q < 16; ++q) row[q] = vals[q];
}

template <int BLOCK, bool DENSE>
__global__ __launch_bounds__(BLOCK) void eval_frames_kernel(const long long* __restrict__ ei, long long E, const float* __restrict__ elab,
                                                            const long long* __restrict__ pred, const int* __restrict__ labels, int N_all,
                                                            const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int P_lds,
                                                            int* __restrict__ gt_out, double* __restrict__ out, double* __restrict__ lf_ws,
                                                            const int* __restrict__ person, const int* __restrict__ cam) {
    const int g = blockIdx.x;
    eval_frame_body<BLOCK, DENSE, true>(g, out + (size_t)g * 16, ei, E, elab, GlobalPred{pred}, GlobalLabel{labels}, N_all, node_ptr, edge_ptr,
                                        P_lds, gt_out, lf_ws, person, cam);
}

}  // namespace gnncca

#include "excl_common.cuh"           // the camera-exclusive rule's shared pieces (also part of mpn_post.hip through exclusive.cuh)
#include "eval_sweep.cuh"            // the threshold sweep: its kernels call eval_frame_body
#include "eval_sweep_exclusive.cuh"  // the same sweep over the camera-exclusive partition
#include "eval_sweep_joint.cuh"      // the sweep of a conjunction of conditions: eval_sweep.cuh's workgroup body, another predicate
#include "eval_sweep_strong.cuh"     // the joint sweep over the strongly connected components of the unpruned edges: no plan, no rev
#include "rank_metrics.cuh"          // threshold-free ranking scores per frame (AUROC, AP, best F) and the pooled curve's histograms

using namespace gnncca;

extern "C" {

size_t gnncca_eval_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames) {
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0) return 0;
    const size_t bytes = ((size_t)n_nodes + (size_t)n_frames) * sizeof(double);   // lf tables: n_g + 1 entries per frame
    return bytes < 256 ? 256 : (bytes + 255) / 256 * 256;
}

static int eval_frames(const int64_t* edge_index, const float* edge_labels, const int64_t* predictions, const int32_t* labels,
                       const int32_t* person_id, const int32_t* cam, bool dense, int64_t n_nodes, int64_t n_edges, const int32_t* node_ptr_dev,
                       const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_nodes, int32_t* gt_labels_out, double* out,
                       void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kEvalMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;
    if (!node_ptr_dev || !edge_ptr_dev || !out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && !labels) return GNNCCA_ERR_INVALID_ARG;
    if (dense && n_nodes > 0 && (!person_id || !cam)) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!edge_index || !edge_labels || !predictions)) return GNNCCA_ERR_INVALID_ARG;
    if (workspace_bytes < gnncca_eval_workspace_bytes(n_nodes, n_edges, n_frames)) return GNNCCA_ERR_WORKSPACE;
    if (n_nodes >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    const int P = frame_capacity(max_frame_nodes);
    const size_t lds = (size_t)3 * P * sizeof(int);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    const long long* pr = reinterpret_cast<const long long*>(predictions);
    double* lf = static_cast<double*>(workspace);
#define GNNCCA_EVAL(B, D)                                                                                                            \
    hipLaunchKernelGGL((eval_frames_kernel<B, D>), dim3((unsigned)n_frames), dim3(B), lds, st, ei, (long long)n_edges, edge_labels, pr, \
                       labels, (int)n_nodes, node_ptr_dev, edge_ptr_dev, P, gt_labels_out, out, lf, person_id, cam)
    launch_frame_block(P, [&](auto block) {
        constexpr int B = decltype(block)::value;
        if (dense) GNNCCA_EVAL(B, true); else GNNCCA_EVAL(B, false);
    });
#undef GNNCCA_EVAL
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_eval_frames(const int64_t* edge_index, const float* edge_labels, const int64_t* predictions, const int32_t* labels,
                       int64_t n_nodes, int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                       int32_t max_frame_nodes, int32_t* gt_labels_out, double* out, void* workspace, size_t workspace_bytes,
                       gnncca_stream_t stream) {
    return eval_frames(edge_index, edge_labels, predictions, labels, nullptr, nullptr, false, n_nodes, n_edges, node_ptr_dev, edge_ptr_dev,
                       n_frames, max_frame_nodes, gt_labels_out, out, workspace, workspace_bytes, stream);
}

int gnncca_eval_frames_dense(const int64_t* edge_index, const float* edge_labels, const int64_t* predictions, const int32_t* labels,
                             const int32_t* person_id, const int32_t* cam, int64_t n_nodes, int64_t n_edges, const int32_t* node_ptr_dev,
                             const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_nodes, int32_t* gt_labels_out, double* out,
                             void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    return eval_frames(edge_index, edge_labels, predictions, labels, person_id, cam, true, n_nodes, n_edges, node_ptr_dev, edge_ptr_dev,
                       n_frames, max_frame_nodes, gt_labels_out, out, workspace, workspace_bytes, stream);
}

// ---- the threshold sweep (eval_sweep.cuh) ---------------------------------------------------------------------------------------------
// The four sweeps -- gnncca_eval_sweep, _exclusive (eval_sweep_exclusive.cuh), _joint (eval_sweep_joint.cuh) and _strong
// (eval_sweep_strong.cuh) -- share one host path: sweep_check, joint_scores, carve_sweep + sweep_prepare, and launch_frame_block for the
// grid (G, T) launch.  What differs between them is an argument of those, never a copy.
//
// workspace of the sweeps that prune: [the graph plan, as gnncca_post_workspace_bytes lays it out | rev int32 [E] | pair keys u64 [E], the
// exclusive sweep only | lgamma tables fp64 [N + G]] -- O(E + N) whatever T is; the only thing of size T x N is the caller's labels_out.
// The strong sweep has neither plan nor reverse edges: its workspace is the lgamma tables alone (gnncca_eval_workspace_bytes).
struct SweepWorkspace { PostWorkspace plan; size_t rev, keys, lf, total; };
static SweepWorkspace carve_sweep(int64_t n, int64_t e, int64_t g, bool with_keys) {
    SweepWorkspace w;
    w.plan = carve_post(n, e);
    size_t off = w.plan.total;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t N = (size_t)(n > 0 ? n : 0), E = (size_t)(e > 0 ? e : 0), G = (size_t)(g > 0 ? g : 0);   // (carve_post's clamp: an entry carves first and checks then)
    w.rev = take(E * 4), w.keys = take(with_keys ? E * 8 : 0), w.lf = take((N + G) * sizeof(double)), w.total = off;
    return w;
}

size_t gnncca_eval_sweep_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames, int64_t n_thresholds) {
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0 || n_thresholds < 0) return 0;
    return carve_sweep(n_nodes, n_edges, n_frames, false).total;
}
size_t gnncca_eval_sweep_exclusive_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames, int64_t n_thresholds) {
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0 || n_thresholds < 0) return 0;
    return carve_sweep(n_nodes, n_edges, n_frames, true).total;
}
size_t gnncca_eval_sweep_joint_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_frames) {   // (whatever the numbers of points and scores)
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0) return 0;
    return carve_sweep(n_nodes, n_edges, n_frames, false).total;
}
size_t gnncca_eval_sweep_strong_workspace_bytes(int64_t n_nodes, int64_t n_edges, int32_t n_frames) {
    return gnncca_eval_workspace_bytes(n_nodes, n_edges, n_frames);
}

// The argument check of the four sweeps, in one order: the sizes, the points, "nothing to do" (OK with *work = false: the caller returns
// without a launch), the pointers the work reads (INVALID_ARG), the 32-bit index range (UNSUPPORTED), the workspace (WORKSPACE).
struct SweepLimits {
    int max_nodes;         // the widest frame: kEvalMaxNodes, kExclMaxNodes or kSweepStrongMaxNodes
    int max_points;        // GNNCCA_EVAL_SWEEP_MAX_THRESHOLDS or GNNCCA_EVAL_JOINT_MAX_POINTS
    bool zero_points_ok;   // the strong sweep: no points is nothing to do, as no frames is, and `points` is looked at only when there is work
    bool need_cam;         // the exclusive sweep
};
//                                            max_nodes             max_points                        zero_points_ok  need_cam
constexpr SweepLimits kLimitsComponents{kEvalMaxNodes,        GNNCCA_EVAL_SWEEP_MAX_THRESHOLDS, false,          false};
constexpr SweepLimits kLimitsExclusive {kExclMaxNodes,        GNNCCA_EVAL_SWEEP_MAX_THRESHOLDS, false,          true};
constexpr SweepLimits kLimitsJoint     {kEvalMaxNodes,        GNNCCA_EVAL_JOINT_MAX_POINTS,     false,          false};
constexpr SweepLimits kLimitsStrong    {kSweepStrongMaxNodes, GNNCCA_EVAL_JOINT_MAX_POINTS,     true,           false};
struct SweepPtrs {   // the arrays of a sweep as its entry got them (null: missing), set by name at the call sites
    const double* points;
    const int64_t* edge_index;   // these three are needed when there are edges; `scores` is the array, or the joint form's array of arrays
    const float* edge_labels;
    const void* scores;
    const int32_t* cam;          // (need_cam, when there are nodes)
    const int32_t* node_ptr;
    const int32_t* edge_ptr;
    const double* rows_out;
    const void* workspace;
};
static int sweep_check(const SweepLimits& lim, int64_t n_nodes, int64_t n_edges, int32_t n_frames, int32_t max_frame_nodes, int32_t n_points,
                       const SweepPtrs& p, size_t workspace_bytes, size_t workspace_need, bool* work) {
    *work = false;
    if (n_nodes < 0 || n_edges < 0 || n_frames < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n_points < (lim.zero_points_ok ? 0 : 1) || n_points > lim.max_points) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > lim.max_nodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    const bool nothing = n_frames == 0 || n_points == 0;
    if (!p.points && !(lim.zero_points_ok && nothing)) return GNNCCA_ERR_INVALID_ARG;
    if (nothing) return GNNCCA_OK;
    if (!p.node_ptr || !p.edge_ptr || !p.rows_out || !p.workspace) return GNNCCA_ERR_INVALID_ARG;
    if (lim.need_cam && n_nodes > 0 && !p.cam) return GNNCCA_ERR_INVALID_ARG;
    if (n_edges > 0 && (!p.edge_index || !p.edge_labels || !p.scores)) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes >= (1ll << 31) - 64 || n_edges >= (1ll << 31) - 64) return GNNCCA_ERR_UNSUPPORTED;
    if (workspace_bytes < workspace_need) return GNNCCA_ERR_WORKSPACE;
    *work = true;
    return GNNCCA_OK;
}

// The K score arrays of the joint and the strong sweep, checked and packed into the kernels' by-value argument.
static int joint_scores(const float* const* scores, const int64_t* score_strides, const int32_t* comparators, int32_t n_scores, int64_t n_edges,
                        JointScores* sc) {
    if (n_scores < 1 || n_scores > GNNCCA_EVAL_JOINT_MAX_SCORES) return GNNCCA_ERR_INVALID_ARG;
    if (!scores || !score_strides || !comparators) return GNNCCA_ERR_INVALID_ARG;
    std::memset(sc, 0, sizeof(*sc));
    sc->K = n_scores;
    for (int k = 0; k < n_scores; ++k) {
        if (comparators[k] < GNNCCA_CMP_GE || comparators[k] > GNNCCA_CMP_LT || score_strides[k] < 1) return GNNCCA_ERR_INVALID_ARG;
        if (n_edges > 0 && !scores[k]) return GNNCCA_ERR_INVALID_ARG;
        sc->p[k] = scores[k], sc->stride[k] = score_strides[k], sc->cmp[k] = comparators[k];
    }
    return GNNCCA_OK;
}

// The three launches every sweep that prunes starts with: the graph plan (launch_post_plan: plan_only + plan finish, nothing without
// edges) and one prepare kernel -- rev and the lgamma tables; with `keys` (the exclusive sweep) its own kernel, which writes the pair keys
// too.  The tables come back as pointers into the workspace.
struct SweepTables { int* rev; excl_u64* keys; double* lf; };
struct SweepExclKeys { const float* scores; const int32_t* edge_ptr_dev; int P; };   // what the pair keys are made of, besides the plan
static int sweep_prepare(const SweepWorkspace& ws, void* workspace, const long long* ei, int E, int N, const int32_t* node_ptr_dev,
                         int32_t n_frames, const SweepExclKeys* keys, hipStream_t st, SweepTables* out) {
    char* base = static_cast<char*>(workspace);
    const PostPlanPtrs plan = post_plan_ptrs(workspace, ws.plan);
    *out = SweepTables{reinterpret_cast<int*>(base + ws.rev), reinterpret_cast<excl_u64*>(base + ws.keys), reinterpret_cast<double*>(base + ws.lf)};
    if (const int rc = launch_post_plan(ei, E, N, plan, EmptyPlan::kSkip, st)) return rc;
    const int edge_blocks = (E + 255) / 256;
    const dim3 grid((unsigned)edge_blocks + (unsigned)n_frames);
    if (keys)
        hipLaunchKernelGGL(eval_sweep_excl_prepare_kernel, grid, dim3(256), 0, st, ei, (long long)E, (const int*)plan.seg_ptr, (const int*)plan.col32,
                           (const int*)plan.perm, (const unsigned*)plan.flags, keys->scores, out->rev, out->keys, edge_blocks, node_ptr_dev,
                           keys->edge_ptr_dev, (int)n_frames, N, keys->P, out->lf);
    else
        hipLaunchKernelGGL(eval_sweep_prepare_kernel, grid, dim3(256), 0, st, ei, (long long)E, (const int*)plan.seg_ptr, (const int*)plan.col32,
                           (const int*)plan.perm, (const unsigned*)plan.flags, out->rev, edge_blocks, node_ptr_dev, N, out->lf);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_eval_sweep(const int64_t* edge_index, const float* edge_labels, const float* scores, int64_t n_nodes, int64_t n_edges,
                      const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_nodes,
                      const double* thresholds_dev, int32_t n_thresholds, int32_t keep_le, double* rows_out, int32_t* labels_out,
                      void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    const SweepWorkspace ws = carve_sweep(n_nodes, n_edges, n_frames, false);
    SweepPtrs p{};
    p.points = thresholds_dev, p.edge_index = edge_index, p.edge_labels = edge_labels, p.scores = scores, p.cam = nullptr;
    p.node_ptr = node_ptr_dev, p.edge_ptr = edge_ptr_dev, p.rows_out = rows_out, p.workspace = workspace;
    bool work;
    if (const int rc = sweep_check(kLimitsComponents, n_nodes, n_edges, n_frames, max_frame_nodes, n_thresholds, p, workspace_bytes, ws.total, &work); rc || !work) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_nodes, E = (int)n_edges;
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    SweepTables tb;
    if (const int rc = sweep_prepare(ws, workspace, ei, E, N, node_ptr_dev, n_frames, nullptr, st, &tb)) return rc;
    const int P = frame_capacity(max_frame_nodes);
    const size_t lds = (size_t)3 * P * sizeof(int) + (size_t)P * sizeof(unsigned short);
    const dim3 grid((unsigned)n_frames, (unsigned)n_thresholds);
    launch_frame_block(P, [&](auto block) {
        constexpr int B = decltype(block)::value;
        hipLaunchKernelGGL((eval_sweep_kernel<B>), grid, dim3(B), lds, st, ei, (long long)E, edge_labels, scores, (const int*)tb.rev, thresholds_dev,
                           (int)keep_le, N, node_ptr_dev, edge_ptr_dev, P, rows_out, labels_out, tb.lf);
    });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_eval_sweep_exclusive(const int64_t* edge_index, const float* edge_labels, const float* scores, const int32_t* cam, int64_t n_nodes,
                                int64_t n_edges, const int32_t* node_ptr_dev, const int32_t* edge_ptr_dev, int32_t n_frames,
                                int32_t max_frame_nodes, const double* thresholds_dev, int32_t n_thresholds, double* rows_out,
                                int32_t* labels_out, void* workspace, size_t workspace_bytes, gnncca_stream_t stream) {
    const SweepWorkspace ws = carve_sweep(n_nodes, n_edges, n_frames, true);
    SweepPtrs p{};
    p.points = thresholds_dev, p.edge_index = edge_index, p.edge_labels = edge_labels, p.scores = scores, p.cam = cam;
    p.node_ptr = node_ptr_dev, p.edge_ptr = edge_ptr_dev, p.rows_out = rows_out, p.workspace = workspace;
    bool work;
    if (const int rc = sweep_check(kLimitsExclusive, n_nodes, n_edges, n_frames, max_frame_nodes, n_thresholds, p, workspace_bytes, ws.total, &work); rc || !work) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_nodes, E = (int)n_edges;
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    const int P = frame_capacity(max_frame_nodes);
    const size_t lds = (size_t)20 * P;   // best u64 | mask u64 | parent int; the scoring's 14 P lie inside (eval_sweep_exclusive.cuh)
    if (lds > 64 * 1024) HIP_TRY(lds_opt_in<eval_sweep_excl_kernel<256>>((size_t)20 * kExclMaxNodes));
    const SweepExclKeys keys{scores, edge_ptr_dev, P};
    SweepTables tb;
    if (const int rc = sweep_prepare(ws, workspace, ei, E, N, node_ptr_dev, n_frames, &keys, st, &tb)) return rc;
    const dim3 grid((unsigned)n_frames, (unsigned)n_thresholds);
    launch_frame_block(P, [&](auto block) {
        constexpr int B = decltype(block)::value;
        hipLaunchKernelGGL((eval_sweep_excl_kernel<B>), grid, dim3(B), lds, st, ei, (long long)E, edge_labels, scores, cam, (const int*)tb.rev,
                           (const excl_u64*)tb.keys, thresholds_dev, N, node_ptr_dev, edge_ptr_dev, P, rows_out, labels_out, tb.lf);
    });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_eval_sweep_joint(const int64_t* edge_index, const float* edge_labels, const float* const* scores, const int64_t* score_strides,
                            const int32_t* comparators, int32_t n_scores, int64_t n_nodes, int64_t n_edges, const int32_t* node_ptr_dev,
                            const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_nodes, const double* points_dev,
                            int32_t n_points, const double* frame_div_dev, double* rows_out, int32_t* labels_out, void* workspace,
                            size_t workspace_bytes, gnncca_stream_t stream) {
    JointScores sc;
    if (const int rc = joint_scores(scores, score_strides, comparators, n_scores, n_edges, &sc)) return rc;
    const SweepWorkspace ws = carve_sweep(n_nodes, n_edges, n_frames, false);
    SweepPtrs p{};
    p.points = points_dev, p.edge_index = edge_index, p.edge_labels = edge_labels, p.scores = scores, p.cam = nullptr;
    p.node_ptr = node_ptr_dev, p.edge_ptr = edge_ptr_dev, p.rows_out = rows_out, p.workspace = workspace;
    bool work;
    if (const int rc = sweep_check(kLimitsJoint, n_nodes, n_edges, n_frames, max_frame_nodes, n_points, p, workspace_bytes, ws.total, &work); rc || !work) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_nodes, E = (int)n_edges;
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    SweepTables tb;
    if (const int rc = sweep_prepare(ws, workspace, ei, E, N, node_ptr_dev, n_frames, nullptr, st, &tb)) return rc;
    const int P = frame_capacity(max_frame_nodes);
    const size_t lds = (size_t)3 * P * sizeof(int) + (size_t)P * sizeof(unsigned short);   // (eval_sweep_body's, as in gnncca_eval_sweep)
    const dim3 grid((unsigned)n_frames, (unsigned)n_points);
    launch_frame_block(P, [&](auto block) {
        constexpr int B = decltype(block)::value;
        hipLaunchKernelGGL((eval_sweep_joint_kernel<B>), grid, dim3(B), lds, st, ei, (long long)E, edge_labels, sc, (const int*)tb.rev, points_dev,
                           frame_div_dev, N, node_ptr_dev, edge_ptr_dev, P, rows_out, labels_out, tb.lf);
    });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_eval_sweep_strong(const int64_t* edge_index, const float* edge_labels, const float* const* scores, const int64_t* score_strides,
                             const int32_t* comparators, int32_t n_scores, int64_t n_nodes, int64_t n_edges, const int32_t* node_ptr_dev,
                             const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_nodes, const double* points_dev,
                             int32_t n_points, const double* frame_div_dev, double* rows_out, int32_t* labels_out, void* workspace,
                             size_t workspace_bytes, gnncca_stream_t stream) {
    JointScores sc;
    if (const int rc = joint_scores(scores, score_strides, comparators, n_scores, n_edges, &sc)) return rc;
    SweepPtrs p{};
    p.points = points_dev, p.edge_index = edge_index, p.edge_labels = edge_labels, p.scores = scores, p.cam = nullptr;
    p.node_ptr = node_ptr_dev, p.edge_ptr = edge_ptr_dev, p.rows_out = rows_out, p.workspace = workspace;
    bool work;
    if (const int rc = sweep_check(kLimitsStrong, n_nodes, n_edges, n_frames, max_frame_nodes, n_points, p, workspace_bytes, gnncca_eval_sweep_strong_workspace_bytes(n_nodes, n_edges, n_frames), &work); rc || !work) return rc;
    const int P = frame_capacity(max_frame_nodes);
    const auto lds_at = [](int nodes) { return sweep_strong_shared_bytes(nodes) + (size_t)nodes * sizeof(unsigned short); };
    const size_t lds = lds_at(P);
    if (lds > 64 * 1024) HIP_TRY(lds_opt_in<eval_sweep_strong_kernel<256>>(lds_at(kSweepStrongMaxNodes)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_nodes, E = (int)n_edges;
    const long long* ei = reinterpret_cast<const long long*>(edge_index);
    double* lf = static_cast<double*>(workspace);
    // the lgamma tables: eval_sweep_prepare_kernel's frame blocks alone (no edge blocks: nothing about edges is read)
    hipLaunchKernelGGL(eval_sweep_prepare_kernel, dim3((unsigned)n_frames), dim3(256), 0, st, ei, (long long)E, (const int*)nullptr,
                       (const int*)nullptr, (const int*)nullptr, (const unsigned*)nullptr, (int*)nullptr, 0, node_ptr_dev, N, lf);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)n_frames, (unsigned)n_points);
    launch_frame_block(P, [&](auto block) {
        constexpr int B = decltype(block)::value;
        hipLaunchKernelGGL((eval_sweep_strong_kernel<B>), grid, dim3(B), lds, st, ei, (long long)E, edge_labels, sc, points_dev, frame_div_dev, N,
                           node_ptr_dev, edge_ptr_dev, P, rows_out, labels_out, lf);
    });
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_eval_rows_accumulate(const double* rows, int32_t n_points, int32_t n_frames, double* sums, int64_t* frames,
                                gnncca_stream_t stream) {
    if (n_points < 1 || n_points > GNNCCA_EVAL_JOINT_MAX_POINTS || n_frames < 0 || !sums) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;
    if (!rows) return GNNCCA_ERR_INVALID_ARG;
    hipLaunchKernelGGL(eval_rows_accumulate_kernel, dim3((unsigned)(n_points * 16 + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       rows, (int)n_points, (int)n_frames, sums, reinterpret_cast<long long*>(frames));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

// ---- ranking scores without a threshold (rank_metrics.cuh) ------------------------------------------------------------------------------
// bytes of dynamic LDS for a batch whose largest frame has max_frame_edges edges: 8 per word of the next power of two (at least 64 words)
size_t gnncca_rank_metrics_lds_bytes(int32_t max_frame_edges) {
    if (max_frame_edges < 0 || max_frame_edges > kRankMaxEdges) return 0;
    size_t words = 64;
    while (words < (size_t)max_frame_edges) words <<= 1;
    return words * sizeof(rank_u64);
}

int gnncca_rank_metrics(const float* edge_labels, const float* const* scores, const int64_t* score_strides, const int32_t* positive_low,
                        int32_t n_scores, int64_t n_edges, const int32_t* edge_ptr_dev, int32_t n_frames, int32_t max_frame_edges,
                        double* rows_out, gnncca_stream_t stream) {
    if (n_edges < 0 || n_frames < 0) return GNNCCA_ERR_INVALID_ARG;
    if (n_scores < 1 || n_scores > kRankMaxScores || !scores || !score_strides || !positive_low) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_edges < 0 || max_frame_edges > kRankMaxEdges || max_frame_edges > n_edges) return GNNCCA_ERR_INVALID_ARG;
    RankScores sc;
    std::memset(&sc, 0, sizeof(sc));
    for (int k = 0; k < n_scores; ++k) {
        if (score_strides[k] < 1 || (positive_low[k] != 0 && positive_low[k] != 1)) return GNNCCA_ERR_INVALID_ARG;
        if (n_edges > 0 && !scores[k]) return GNNCCA_ERR_INVALID_ARG;
        sc.p[k] = scores[k], sc.stride[k] = score_strides[k], sc.low[k] = positive_low[k];
    }
    if (n_frames == 0) return GNNCCA_OK;
    if (!edge_ptr_dev || !rows_out || (n_edges > 0 && !edge_labels)) return GNNCCA_ERR_INVALID_ARG;
    const size_t lds = gnncca_rank_metrics_lds_bytes(max_frame_edges);
    const int cap = (int)(lds / sizeof(rank_u64));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_frames, (unsigned)n_scores);
    if (cap > 4096) HIP_TRY(lds_opt_in<rank_metrics_kernel<1024>>(kRankMaxEdges * sizeof(rank_u64)));   // (above 64 KiB of dynamic LDS)
#define GNNCCA_RANK(B)                                                                                                             \
    hipLaunchKernelGGL((rank_metrics_kernel<B>), grid, dim3(B), lds, st, edge_labels, (long long)n_edges, sc, edge_ptr_dev, cap, rows_out)
    if (cap <= 1024) GNNCCA_RANK(256);   // threads by capacity: at most 16 words of the image per thread
    else if (cap <= 4096) GNNCCA_RANK(512);
    else GNNCCA_RANK(1024);
#undef GNNCCA_RANK
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_rank_rows_accumulate(const double* rows, int32_t n_scores, int32_t n_frames, double* sums, int64_t* counts, gnncca_stream_t stream) {
    if (n_scores < 1 || n_scores > kRankMaxScores || n_frames < 0 || !sums || !counts) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;
    if (!rows) return GNNCCA_ERR_INVALID_ARG;
    hipLaunchKernelGGL(rank_rows_accumulate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), rows, (int)n_scores, (int)n_frames,
                       sums, reinterpret_cast<long long*>(counts));
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_rank_pool_add(const float* scores, int64_t score_stride, const float* labels, int64_t n_samples, const double* thresholds_dev,
                         int32_t n_thresholds, int32_t keep_le, int64_t* hist, int64_t* nan_count, gnncca_stream_t stream) {
    if (n_samples < 0 || score_stride < 1) return GNNCCA_ERR_INVALID_ARG;
    if (n_thresholds < 1 || n_thresholds > GNNCCA_RANK_POOL_MAX_THRESHOLDS || !thresholds_dev || !hist || !nan_count) return GNNCCA_ERR_INVALID_ARG;
    if (n_samples == 0) return GNNCCA_OK;
    if (!scores || !labels) return GNNCCA_ERR_INVALID_ARG;
    const long long per_block = 256 * kPoolPerThread;
    const long long blocks = (n_samples + per_block - 1) / per_block;
    if (blocks >= (1ll << 31)) return GNNCCA_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define GNNCCA_POOL(L)                                                                                                                   \
    hipLaunchKernelGGL((rank_pool_add_kernel<L>), dim3((unsigned)blocks), dim3(256), 0, st, scores, (long long)score_stride, labels,     \
                       (long long)n_samples, thresholds_dev, (int)n_thresholds, (int)keep_le, reinterpret_cast<rank_u64*>(hist),         \
                       reinterpret_cast<rank_u64*>(nan_count))
    if (n_thresholds + 1 <= kPoolLdsBuckets) GNNCCA_POOL(true); else GNNCCA_POOL(false);
#undef GNNCCA_POOL
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
