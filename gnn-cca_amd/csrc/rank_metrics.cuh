#pragma once
// rank_metrics.cuh -- how well a per-edge score ORDERS the edges, without a threshold: AUROC, average precision and the best F over all
// cuts, per frame (gnncca_rank_metrics); the fold of such rows over a data set (gnncca_rank_rows_accumulate); and the reference's pooled
// sweep (main.py:124-319, MODE REID: `preds = dist <= t` over every raw edge distance of the data set, compute_P_R_F on the pooled vector,
// no pruning, no clustering) as two histograms that any split of the data set into calls fills alike (gnncca_rank_pool_add).  Part of the
// translation unit evaluate.hip (fp contract(off): no multiply and add below may fuse); include/gnncca_mpn.h has the rule in full.
//
// One workgroup per (frame, score).  The frame's samples -- its edges with a label of exactly 1 or 0 and a score that is no NaN -- are
// packed as 64-bit words (~key << 32 | label) into LDS, every other slot up to the next power of two holds the sentinel ~0, and a bitonic
// network sorts the words ascending: the most positive key first, the sentinels last.  Equal words are equal bits, so the sorted image does
// not depend on where a sample started.  Then, on the sorted image:
//   scan    the low half of word i becomes the number of positives at positions <= i (tiles of BLOCK positions: ballot + popcount per
//           wave, the waves' totals through LDS); negatives follow from the position, a word's own label from its left neighbour;
//   groups  position i ends a tie group iff the key at i + 1 differs (a flag the scan leaves in bit 31 of the low half); the group's start
//           is a binary search for its key, and the counts at the end of the previous group are read there.  Integer sums (the AUROC
//           numerator, the number of groups) go through LDS atomics, which no order can change;
//   AP      the group's term lands on its end position, every other position holds +0; the image is overwritten with the terms, tile by
//           tile from the top (a group's end reads nothing above itself), and summed in the header's order: 256 lanes, lane q the
//           positions q, q + 256, ... ascending, a butterfly over each 64 lanes (xor 32 ... 1), the four results left to right.  The order
//           names neither the block size nor the LDS capacity: a frame's bits do not depend on the batch it travels in;
//   best F  every thread keeps its best cut, then an LDS maximum over the bits of F (non-negative doubles order as integers) and an LDS
//           minimum over (position << 32 | ~key) of the threads that reach it: the first cut in visiting order, with its score.
// Three instantiations, threads by LDS capacity (up to 1024 words: 256, up to 4096: 512, up to 16384: 1024; at most 16 words per thread).
// The launch reserves 8 bytes per word of the batch's largest frame rounded up to a power of two, so a Terrace frame (768 edges) takes
// 8 KiB of a CU's 160, not 128; above 64 KiB the largest form needs the dynamic-LDS attribute.
namespace gnncca {

constexpr int kRankMaxScores = GNNCCA_RANK_MAX_SCORES;
constexpr int kRankMaxEdges = GNNCCA_RANK_MAX_FRAME_EDGES;
constexpr int kRankLanes = 256;   // of AP's summation order

typedef unsigned long long rank_u64;
constexpr rank_u64 kRankEnd = 1ull << 31, kRankCount = (1ull << 31) - 1;   // a scanned word: ~key << 32 | the last of its group | positives so far

// the K scores of one call, by value in the kernel's arguments: element e of score k is p[k][e * stride[k]]
struct RankScores {
    const float* p[kRankMaxScores];
    long long stride[kRankMaxScores];
    int low[kRankMaxScores];   // 1: the ranking key is that of the negated score (distances)
};

// fp32 -> 32 bits, monotone: a larger score has a larger key; -0 is +0.  (NaNs never get here.)
__device__ __forceinline__ unsigned rank_key(float s) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rank_unkey(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

enum { R_NPOS, R_NNEG, R_NNAN, R_GROUPS, R_NUM, R_BESTF, R_BESTAT, R_COUNT };

// rows_out: fp64 [K][G][8] = n_pos, n_neg, n_distinct, n_nan, AUROC, AP, best_F, best_cut.  cap: words of dynamic LDS (a power of two
// <= CAP).  A frame whose edge range does not fit (outside [0, E], more than cap edges) gets eight NaNs.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void rank_metrics_kernel(const float* __restrict__ elab, long long E, const RankScores sc,
                                                             const int* __restrict__ edge_ptr, int cap, double* __restrict__ rows_out) {
    static_assert(BLOCK >= kRankLanes && BLOCK % 64 == 0, "AP's 256 lanes are threads of the block");
    extern __shared__ rank_u64 s_rank[];
    __shared__ rank_u64 s_acc[R_COUNT];
    __shared__ unsigned s_tile[BLOCK / 64];
    __shared__ double s_ap[kRankLanes / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, q = blockIdx.y;
    double* row = rows_out + ((size_t)q * gridDim.x + g) * 8;
    const long long k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
    if (k0 < 0 || k1 < k0 || k1 > E || k1 - k0 > cap) {
        if (tid < 8) row[tid] = __builtin_nan("");
        return;
    }
    const int ne = (int)(k1 - k0);
    int sort_n = 1;
    while (sort_n < ne) sort_n <<= 1;
    const float* sp = nullptr;
    long long stride = 1;
    bool low = false;
#pragma unroll
    for (int j = 0; j < kRankMaxScores; ++j)   // (constant indices: the argument struct stays in scalar registers)
        if (j == q) sp = sc.p[j], stride = sc.stride[j], low = sc.low[j] != 0;
    if (tid < R_COUNT) s_acc[tid] = tid == R_BESTAT ? ~0ull : 0ull;
    __syncthreads();

    // ---- the image -------------------------------------------------------------------------------------------------------------------
    {
        unsigned npos = 0, nneg = 0, nnan = 0;
        for (int i = tid; i < sort_n; i += BLOCK) {
            rank_u64 w = ~0ull;
            if (i < ne) {
                const float l = elab[k0 + i];
                if (l == 1.f || l == 0.f) {   // gnncca_eval_frames' reading of a label: any other value is no sample
                    float s = sp[(k0 + i) * stride];
                    npos += l == 1.f;
                    nneg += l == 0.f;
                    if (s != s) {
                        ++nnan;
                    } else {
                        if (low) s = -s;
                        w = ((rank_u64)(~rank_key(s)) << 32) | (l == 1.f ? 1ull : 0ull);
                    }
                }
            }
            s_rank[i] = w;
        }
        if (npos) atomicAdd(&s_acc[R_NPOS], (rank_u64)npos);
        if (nneg) atomicAdd(&s_acc[R_NNEG], (rank_u64)nneg);
        if (nnan) atomicAdd(&s_acc[R_NNAN], (rank_u64)nnan);
    }
    __syncthreads();
    for (int k = 2; k <= sort_n; k <<= 1) {   // bitonic sort, one compare-exchange per thread and pass
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int h = tid; h < (sort_n >> 1); h += BLOCK) {
                const int i = ((h & ~(j - 1)) << 1) | (h & (j - 1)), l = i | j;
                const rank_u64 x = s_rank[i], y = s_rank[l];
                if ((x > y) == ((i & k) == 0)) {
                    s_rank[i] = y;
                    s_rank[l] = x;
                }
            }
            __syncthreads();
        }
    }
    const rank_u64 NPOS = s_acc[R_NPOS], NNEG = s_acc[R_NNEG], NNAN = s_acc[R_NNAN];
    const int m = (int)(NPOS + NNEG - NNAN);   // the samples: positions [0, m) of the image
    const bool real = NNAN == 0 && NPOS > 0;   // AP and best F exist (AUROC: and NNEG > 0)

    // ---- scan: positives at positions <= i ---------------------------------------------------------------------------------------------
    {
        unsigned running = 0;
        for (int base = 0; base < m; base += BLOCK) {
            const int i = base + tid;
            const rank_u64 w = i < m ? s_rank[i] : 0ull;
            const bool end = i < m && (i + 1 == m || (unsigned)(s_rank[i + 1] >> 32) != (unsigned)(w >> 32));   // (i + 1: not written before the barrier)
            const rank_u64 b = __ballot((int)(w & 1ull));
            const unsigned upto = (unsigned)__popcll(b & ((2ull << lane) - 1ull));
            if (lane == 0) s_tile[wave] = (unsigned)__popcll(b);
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int v = 0; v < BLOCK / 64; ++v) {
                const unsigned c = s_tile[v];
                before += v < wave ? c : 0u;
                total += c;
            }
            if (i < m) s_rank[i] = (w & 0xFFFFFFFF00000000ull) | (end ? kRankEnd : 0ull) | (rank_u64)(running + before + upto);
            running += total;
            __syncthreads();
        }
    }

    // ---- groups: one tile of BLOCK positions at a time, from the last tile to the first ---------------------------------------------------
    // A group's end reads its own word, the words below it (the binary search for the group's start, the counts in front of it) and
    // nothing above: when a tile has been read, its positions are free to take AP's terms.
    {
        rank_u64 num = 0, at = ~0ull;
        unsigned groups = 0;
        double fbest = -1.0;
        for (int base = m > 0 ? (m - 1) / BLOCK * BLOCK : -1; base >= 0; base -= BLOCK) {
            const int i = base + tid;
            const rank_u64 w = i < m ? s_rank[i] : 0ull;
            double term = 0.0;
            if (w & kRankEnd) {
                ++groups;
                if (real) {
                    const unsigned hi = (unsigned)(w >> 32);
                    int lo = 0, up = i;   // the group's first position
                    while (lo < up) {
                        const int mid = (lo + up) >> 1;
                        if ((unsigned)(s_rank[mid] >> 32) < hi) lo = mid + 1;
                        else up = mid;
                    }
                    const rank_u64 TPprev = lo ? (s_rank[lo - 1] & kRankCount) : 0ull, FPprev = (rank_u64)lo - TPprev;
                    const rank_u64 TP = w & kRankCount, FP = (rank_u64)(i + 1) - TP, p = TP - TPprev;
                    num += p * ((NNEG - FP) + (NNEG - FPprev));   // p (2 neg_ranked_below + n)
                    if (p) term = ((double)p / (double)NPOS) * ((double)TP / (double)(TP + FP));
                    // compute_P_R_F at this cut: TP + FP = i + 1 > 0, TP + FN = NPOS > 0
                    const double P = (double)TP / (double)(TP + FP);
                    const double R = (double)TP / (double)NPOS;
                    const double PR = P * R;
                    const double F = (P + R) != 0.0 ? 2.0 * PR / (P + R) : 0.0;
                    if (F >= fbest) fbest = F, at = ((rank_u64)i << 32) | hi;   // (descending positions: >= keeps the first cut)
                }
            }
            __syncthreads();
            if (i < m) s_rank[i] = (rank_u64)__double_as_longlong(term);
            __syncthreads();
        }
        if (num) atomicAdd(&s_acc[R_NUM], num);
        if (groups) atomicAdd(&s_acc[R_GROUPS], (rank_u64)groups);
        if (fbest >= 0.0) atomicMax(&s_acc[R_BESTF], (rank_u64)__double_as_longlong(fbest));
        __syncthreads();
        if (fbest >= 0.0 && (rank_u64)__double_as_longlong(fbest) == s_acc[R_BESTF]) atomicMin(&s_acc[R_BESTAT], at);
    }
    double ap = 0.0;
    if (tid < kRankLanes)
        for (int i = tid; i < m; i += kRankLanes) ap += __longlong_as_double((long long)s_rank[i]);
    ap = wave_sum(ap);
    if (lane == 0 && wave < kRankLanes / 64) s_ap[wave] = ap;
    __syncthreads();

    // ---- the row ---------------------------------------------------------------------------------------------------------------------
    if (tid != 0) return;
    const double nan = __builtin_nan("");
    double auroc = nan, AP = nan, bestF = nan, cut = nan;
    if (real) {
        if (NNEG > 0) auroc = (double)s_acc[R_NUM] / (double)(2ull * NPOS * NNEG);
        AP = ((s_ap[0] + s_ap[1]) + s_ap[2]) + s_ap[3];
        bestF = __longlong_as_double((long long)s_acc[R_BESTF]);
        float s = rank_unkey(~(unsigned)(s_acc[R_BESTAT] & 0xFFFFFFFFull));
        if (low) s = -s;
        cut = (double)s + 0.0;   // (a zero cut is +0 under either sign of `positive`)
    }
    const double vals[8] = {(double)NPOS, (double)NNEG, (double)s_acc[R_GROUPS], (double)NNAN, auroc, AP, bestF, cut};
#pragma unroll
    for (int c = 0; c < 8; ++c) row[c] = vals[c];
}

// state: fp64 sums [K][8] then int64 counts [K][8].  One thread per (k, column): the frames in ascending g, a NaN skipped, a plain fp64
// add and a count for every other value.  No atomics, no tree: the order is the contract.
__global__ __launch_bounds__(64) void rank_rows_accumulate_kernel(const double* __restrict__ rows, int K, int G, double* __restrict__ sums,
                                                                  long long* __restrict__ counts) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= K * 8) return;
    const double* r = rows + (size_t)(i >> 3) * G * 8 + (i & 7);
    double s = sums[i];
    long long c = counts[i];
    for (int g = 0; g < G; ++g) {
        const double v = r[(size_t)g * 8];
        if (v == v) s += v, ++c;
    }
    sums[i] = s, counts[i] = c;
}

// The pooled curve.  hist: int64 [2][T + 1], row 0 the negatives, row 1 the positives; nan_out: int64 [2] likewise.  A sample's bucket is
// the number of thresholds below its score (keep_le: strictly below; else: below or equal), found by binary search in fp64 against the
// widened fp32 score: with keep_le the sample is predicted at every t >= bucket, else at every t < bucket.  Up to 1024 thresholds a
// workgroup counts in LDS first and adds its non-zero counters to the global histograms; above that every sample adds there itself.
// Integer atomics only: the state after a data set does not depend on how it was cut into calls.
constexpr int kPoolLdsBuckets = 1025;
constexpr int kPoolPerThread = 16;

template <bool LDS_HIST>
__global__ __launch_bounds__(256) void rank_pool_add_kernel(const float* __restrict__ scores, long long stride, const float* __restrict__ labels,
                                                            long long n, const double* __restrict__ th, int T, int keep_le,
                                                            rank_u64* __restrict__ hist, rank_u64* __restrict__ nan_out) {
    __shared__ unsigned s_hist[LDS_HIST ? 2 * kPoolLdsBuckets : 1];
    const int tid = threadIdx.x;
    if (LDS_HIST) {
        for (int i = tid; i < 2 * (T + 1); i += 256) s_hist[i] = 0u;
        __syncthreads();
    }
    unsigned nan0 = 0, nan1 = 0;
    const long long first = (long long)blockIdx.x * (256 * kPoolPerThread);
    for (int r = 0; r < kPoolPerThread; ++r) {
        const long long e = first + (long long)r * 256 + tid;
        if (e >= n) break;
        const float l = labels[e];
        if (!(l == 1.f || l == 0.f)) continue;
        const int pos = l == 1.f;
        const float sf = scores[e * stride];
        if (sf != sf) {
            nan0 += !pos, nan1 += pos;
            continue;
        }
        const double s = (double)sf;
        int lo = 0, up = T;
        while (lo < up) {
            const int mid = (lo + up) >> 1;
            const double t = th[mid];
            if (keep_le ? t < s : t <= s) lo = mid + 1;
            else up = mid;
        }
        if (LDS_HIST) atomicAdd(&s_hist[pos * (T + 1) + lo], 1u);
        else atomicAdd(&hist[(size_t)pos * (T + 1) + lo], 1ull);
    }
    if (nan0) atomicAdd(&nan_out[0], (rank_u64)nan0);
    if (nan1) atomicAdd(&nan_out[1], (rank_u64)nan1);
    if (LDS_HIST) {
        __syncthreads();
        for (int i = tid; i < 2 * (T + 1); i += 256) {
            const unsigned c = s_hist[i];
            if (c) atomicAdd(&hist[i], (rank_u64)c);
        }
    }
}

}  // namespace gnncca
