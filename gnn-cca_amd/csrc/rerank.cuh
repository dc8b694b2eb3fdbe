#pragma once
// rerank.cuh -- the rank-R ReID baseline of the reference (MODE eval_RANK, inference.py:388-511) on gfx950: all-pairs L2 distances inside
// every frame (torch.cdist, inference.py:416), k-reciprocal re-ranking (libs/utils.py:578-644, Zhong et al.) and the rank-R selection onto
// the batch's own edge list (inference.py:454-481).  Part of the translation unit rerank.hip, compiled without fp contraction: every
// multiply-add below that may fuse is written as fmaf.
//
// A batch's matrices lie back to back: frame g's n_g x n_g row-major fp32 matrix at data + sum_{q<g} n_q^2.  No kernel is handed that
// offset: a workgroup sums the squares of the frames in front of it from node_ptr (integers through an LDS atomic: order-independent) and
// refuses its frame when the matrix would not fit into `total` elements -- the device offsets cannot lead a store out of the allocation.
namespace gnncca {

constexpr int kRerankMaxNodes = GNNCCA_RERANK_MAX_FRAME_NODES;
constexpr int kRerankMaxK1 = GNNCCA_RERANK_MAX_K1;

// -> the element offset of frame g's matrix, or -1 when node_ptr is not usable (a negative or decreasing entry, a frame in front of g or g
// itself that would end beyond `total`).  Every thread of the block gets the same value; two barriers.
template <int BLOCK>
__device__ __forceinline__ long long frame_matrix_offset(const int* __restrict__ node_ptr, int g, long long total) {
    __shared__ unsigned long long s_off;
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_off = 0, s_bad = 0;
    __syncthreads();
    unsigned long long part = 0;
    bool bad = false;
    for (int q = threadIdx.x; q < g; q += BLOCK) {
        const long long m = (long long)node_ptr[q + 1] - (long long)node_ptr[q];
        if (m < 0 || m > (1ll << 30)) bad = true;
        else part += (unsigned long long)(m * m);
    }
    if (part) atomicAdd(&s_off, part);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    const long long off = (long long)s_off;
    const long long n = (long long)node_ptr[g + 1] - (long long)node_ptr[g];
    if (s_bad || node_ptr[g] < 0 || n < 0 || n > (1ll << 30) || off < 0 || off > total || n * n > total - off) return -1;
    return off;
}

// ---- 1. all-pairs L2 distances per frame ---------------------------------------------------------------------------------------------
// Workgroup (g, ti, tj): the 16 x 16 tile (ti, tj) of frame g; thread (r, c) owns out[16 ti + r][16 tj + c] = sqrt(sum_k (a_k - b_k)^2),
// summed over k ascending with one fmaf per term.  (a - b)^2 == (b - a)^2 exactly and the order does not depend on the side, so the
// matrix is symmetric bit for bit; a row against itself sums zeros, so the diagonal is exactly 0.  The two 16-row slabs go through LDS
// in chunks of 32 columns (scalar loads: any width R >= 1, any alignment).
constexpr int kDistTile = 16, kDistChunk = 32;

__global__ __launch_bounds__(256) void frame_distances_kernel(const float* __restrict__ x, int R, int N_all, const int* __restrict__ node_ptr,
                                                              long long total, float* __restrict__ out) {
    __shared__ float s_a[kDistTile][kDistChunk + 1], s_b[kDistTile][kDistChunk + 1];
    const int g = blockIdx.x, tid = threadIdx.x;
    const long long off = frame_matrix_offset<256>(node_ptr, g, total);
    if (off < 0) return;
    const int v0 = node_ptr[g], n = node_ptr[g + 1] - v0;
    if (n > N_all - v0) return;
    const int i0 = (int)blockIdx.y * kDistTile, j0 = (int)blockIdx.z * kDistTile;
    if (i0 >= n || j0 >= n) return;   // (the grid is sized for the batch's largest frame)
    const int r = tid >> 4, c = tid & 15;
    float acc = 0.f;
    for (int k0 = 0; k0 < R; k0 += kDistChunk) {
        for (int t = tid; t < kDistTile * kDistChunk; t += 256) {
            const int row = t / kDistChunk, col = t % kDistChunk;
            const bool in_k = k0 + col < R;
            s_a[row][col] = (in_k && i0 + row < n) ? x[(size_t)(v0 + i0 + row) * R + k0 + col] : 0.f;
            s_b[row][col] = (in_k && j0 + row < n) ? x[(size_t)(v0 + j0 + row) * R + k0 + col] : 0.f;
        }
        __syncthreads();
        const int kc = min(kDistChunk, R - k0);
        for (int k = 0; k < kc; ++k) {
            const float d = s_a[r][k] - s_b[c][k];
            acc = fmaf(d, d, acc);
        }
        __syncthreads();
    }
    if (i0 + r < n && j0 + c < n) out[off + (long long)(i0 + r) * n + (j0 + c)] = sqrtf(acc);
}

// ---- 2. k-reciprocal re-ranking, one workgroup per frame, everything between the two passes over D on chip ------------------------------
// LDS (dynamic), P = the batch's largest frame, LD = P | 1 (an odd row stride: a column walk touches every bank once):
//   ta fp32 [P][LD]   V;           tb fp32 [P][LD]   O (steps 1-5), then V' (steps 6-7; O is recomputed from D for step 8)
//   cmax fp32 [P]     the column maxima of D^2;      rsum fp32 [P]   the row sums of step 5
//   masks u64 [6][P][2]   F_K, F_h, R_K, R_h, X and the support of V' (the last for the debug output only)
//   rank u8 [P][KP]   the first KP = min(max(k1 + 1, k2), P) entries of every row's ranking
// 153,728 bytes at P = 128 (one workgroup per CU), 13.9 KiB at P = 34.
struct RerankLds {
    int ld, kp;
    size_t ta, tb, cmax, rsum, masks, rank, total;
};
__host__ __device__ inline RerankLds rerank_lds(int P, int k1, int k2) {
    RerankLds l;
    l.ld = P | 1;
    const int want = (k1 + 1 > k2 ? k1 + 1 : k2);
    l.kp = want < P ? want : P;
    size_t off = 0;
    l.ta = off, off += (size_t)P * l.ld * 4;
    l.tb = off, off += (size_t)P * l.ld * 4;
    off = (off + 7) / 8 * 8;
    l.masks = off, off += (size_t)6 * P * 16;
    l.cmax = off, off += (size_t)P * 4;
    l.rsum = off, off += (size_t)P * 4;
    l.rank = off, off += (size_t)P * l.kp;
    l.total = (off + 15) / 16 * 16;
    return l;
}

enum { M_FK, M_FH, M_RK, M_RH, M_X, M_SUP };

__device__ __forceinline__ bool mask_has(const unsigned long long* m, int j) { return (m[j >> 6] >> (j & 63)) & 1ull; }
__device__ __forceinline__ void mask_set(unsigned long long* m, int j) { atomicOr(&m[j >> 6], 1ull << (j & 63)); }

// h = int(np.around(k1 / 2.)) + 1: numpy rounds a half to the even neighbour (k1 = 5 -> 3, k1 = 7 -> 5)
__host__ __device__ inline int rerank_half(int k1) {
    int m = k1 / 2;
    if ((k1 & 1) && (m & 1)) ++m;
    return m + 1;
}

// rank_out (nullable): int32 [N_all][rank_cols], row v = the first min(rank_cols, KP, n) entries of v's ranking (frame-local ids), -1 after.
// mask_out (nullable): u64 [N_all][4], row v = X(v) (two words) and the support of V'[v] (two words).
// DEBUG = false ignores both (the instantiation every ordinary call runs: three arguments fewer to keep in scalar registers).
template <int BLOCK, bool DEBUG>
__global__ __launch_bounds__(BLOCK) void rerank_frames_kernel(const float* __restrict__ dist, long long total, int N_all,
                                                              const int* __restrict__ node_ptr, int P, int k1, int k2, float lam,
                                                              float one_minus_lam, float* __restrict__ out, int* __restrict__ rank_out,
                                                              int rank_cols, unsigned long long* __restrict__ mask_out) {
    extern __shared__ unsigned char s_raw[];
    const int g = blockIdx.x, tid = threadIdx.x;
    const long long off = frame_matrix_offset<BLOCK>(node_ptr, g, total);
    if (off < 0) return;
    const int v0 = node_ptr[g], n = node_ptr[g + 1] - v0;
    if (n > P || n > N_all - v0 || n == 0) return;   // (the entry refused a larger frame from the host's node_ptr already)
    const RerankLds L = rerank_lds(P, k1, k2);
    const int LD = L.ld, KP = min(L.kp, n);
    float* ta = reinterpret_cast<float*>(s_raw + L.ta);
    float* tb = reinterpret_cast<float*>(s_raw + L.tb);
    float* cmax = reinterpret_cast<float*>(s_raw + L.cmax);
    float* rsum = reinterpret_cast<float*>(s_raw + L.rsum);
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(s_raw + L.masks);
    unsigned char* rank = s_raw + L.rank;
    auto mask = [&](int which, int i) { return masks + ((size_t)which * P + i) * 2; };
    const float* D = dist + off;
    float* outg = out + off;
    const int nn = n * n;
    const int K = k1 + 1, h = rerank_half(k1);

    // 1. normalise: cmax[i] = max_k fl(D[k][i]^2); O[i][j] = fl(D[j][i]^2) / cmax[i], a zero column gives a zero row
    for (int i = tid; i < n; i += BLOCK) {
        float m = 0.f;
        for (int k = 0; k < n; ++k) {
            const float d = D[k * n + i];
            m = fmaxf(m, d * d);
        }
        cmax[i] = m;
    }
    for (int t = tid; t < 6 * P * 2; t += BLOCK) masks[t] = 0ull;
    for (int t = tid; t < P * L.kp; t += BLOCK) rank[t] = 0;   // (a NaN distance leaves positions unclaimed: they must stay valid ids)
    __syncthreads();
    for (int t = tid; t < nn; t += BLOCK) {   // t = j * n + i: the loads are contiguous, the odd LD keeps the stores off one bank
        const int j = t / n, i = t - j * n;
        const float d = D[t], m = cmax[i];
        tb[i * LD + j] = m > 0.f ? (d * d) / m : 0.f;
    }
    __syncthreads();
    // 2. rank by counting: the position of j in row i is #{m : O[i][m] < O[i][j], or equal and m < j}
    for (int t = tid; t < nn; t += BLOCK) {
        const int i = t / n, j = t - i * n;
        const float* row = tb + i * LD;
        const float oj = row[j];
        int pos = 0;
        for (int m = 0; m < n; ++m) {
            const float om = row[m];
            pos += (om < oj || (om == oj && m < j)) ? 1 : 0;
        }
        if (pos < KP) rank[i * L.kp + pos] = (unsigned char)j;
        if (pos < K) mask_set(mask(M_FK, i), j);
        if (pos < h) mask_set(mask(M_FH, i), j);
    }
    __syncthreads();
    // 3. reciprocal sets: R_m(i) = {j in F_m(i) : i in F_m(j)}
    for (int t = tid; t < nn; t += BLOCK) {
        const int i = t / n, j = t - i * n;
        if (mask_has(mask(M_FK, i), j) && mask_has(mask(M_FK, j), i)) mask_set(mask(M_RK, i), j), mask_set(mask(M_X, i), j);
        if (mask_has(mask(M_FH, i), j) && mask_has(mask(M_FH, j), i)) mask_set(mask(M_RH, i), j);
    }
    __syncthreads();
    // 4. expansion: X(i) = R_K(i) | OR { R_h(c) : c in R_K(i), |R_h(c) & R_K(i)| > 2/3 |R_h(c)| }.  The reference compares a > 2./3*b in
    // float64; 3 a > 2 b decides the same for every 0 <= a <= b <= 65 (tests/test_rerank_args.py checks all of them on the CPU).
    for (int t = tid; t < nn; t += BLOCK) {
        const int i = t / n, c = t - i * n;
        const unsigned long long* rk = mask(M_RK, i);
        if (!mask_has(rk, c)) continue;
        const unsigned long long* rh = mask(M_RH, c);
        const unsigned long long h0 = rh[0], h1 = rh[1];
        const int a = __popcll(h0 & rk[0]) + __popcll(h1 & rk[1]), b = __popcll(h0) + __popcll(h1);
        if (3 * a > 2 * b) {
            unsigned long long* x = mask(M_X, i);
            if (h0) atomicOr(&x[0], h0);
            if (h1) atomicOr(&x[1], h1);
        }
    }
    __syncthreads();
    // 5. weights: V[i][j] = exp(-O[i][j]) / sum_{m in X(i), ascending} exp(-O[i][m]).  The row sum runs over every column in ascending
    // order: the columns outside X(i) hold +0, which changes no partial sum, so it is the sum over X(i) in ascending order.
    for (int t = tid; t < nn; t += BLOCK) {
        const int i = t / n, j = t - i * n;
        ta[i * LD + j] = mask_has(mask(M_X, i), j) ? expf(-tb[i * LD + j]) : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < n; i += BLOCK) {
        float s = 0.f;
        for (int m = 0; m < n; ++m) s += ta[i * LD + m];
        rsum[i] = s;
    }
    __syncthreads();
    for (int t = tid; t < nn; t += BLOCK) {
        const int i = t / n, j = t - i * n;
        const float w = ta[i * LD + j];
        if (w != 0.f) ta[i * LD + j] = w / rsum[i];
    }
    __syncthreads();
    // 6. query expansion: V'[i] = (V[rank[i][0]] + V[rank[i][1]] + ...) / count, summed in rank order, over the first min(k2, n) entries
    const float* tv = ta;
    if (k2 != 1) {
        const int kq = min(k2, n);
        const float cnt = (float)kq;
        for (int t = tid; t < nn; t += BLOCK) {
            const int i = t / n, c = t - i * n;
            const unsigned char* ri = rank + i * L.kp;
            float s = 0.f;
            for (int q = 0; q < kq; ++q) s += ta[(int)ri[q] * LD + c];
            tb[i * LD + c] = s / cnt;
        }
        tv = tb;
        __syncthreads();
    }
    if (DEBUG && mask_out) {
        for (int t = tid; t < nn; t += BLOCK) {
            const int i = t / n, c = t - i * n;
            if (tv[i * LD + c] != 0.f) mask_set(mask(M_SUP, i), c);
        }
        __syncthreads();
        for (int t = tid; t < n * 4; t += BLOCK) {
            const int i = t >> 2, w = t & 3;
            mask_out[(size_t)(v0 + i) * 4 + w] = mask(w < 2 ? M_X : M_SUP, i)[w & 1];
        }
    }
    if (DEBUG && rank_out) {
        for (int t = tid; t < n * rank_cols; t += BLOCK) {
            const int i = t / rank_cols, q = t - i * rank_cols;
            rank_out[(size_t)(v0 + i) * rank_cols + q] = q < KP ? (int)rank[i * L.kp + q] : -1;
        }
    }
    // 7. + 8.  S = sum_c min(V'[i][c], V'[j][c]) over c ascending; J = 1 - S / (2 - S); out = J (1 - lam) + O lam
    for (int t = tid; t < nn; t += BLOCK) {
        const int i = t / n, j = t - i * n;
        const float* a = tv + i * LD;
        const float* b = tv + j * LD;
        float s = 0.f;
        for (int c = 0; c < n; ++c) s += fminf(a[c], b[c]);
        const float jac = 1.f - s / (2.f - s);
        const float d = D[j * n + i], m = cmax[i];
        const float o = m > 0.f ? (d * d) / m : 0.f;
        outg[t] = jac * one_minus_lam + o * lam;
    }
}

// ---- 3. rank-R predictions on the batch's edge list ----------------------------------------------------------------------------------
// One workgroup per frame.  A wave takes a row i at a time: the row of `dist` and the cameras sit in LDS, lane j counts the cross-camera
// candidates of i in front of j (smaller distance, or equal and a smaller id) and j is selected iff fewer than `rank` are.  The selected
// sets are 128-bit masks; the workgroup then walks the frame's edges: (i, j) is predicted iff j is selected by i or i by j.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void rank_predictions_kernel(const float* __restrict__ dist, long long total, const int* __restrict__ cam,
                                                                 int N_all, const long long* __restrict__ ei, long long E,
                                                                 const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, int rank,
                                                                 long long* __restrict__ pred) {
    __shared__ float s_row[BLOCK / 64][kRerankMaxNodes];
    __shared__ int s_cam[kRerankMaxNodes];
    __shared__ unsigned long long s_sel[kRerankMaxNodes][2];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long k0 = edge_ptr[g], k1 = edge_ptr[g + 1];
    const bool edges_ok = k0 >= 0 && k1 >= k0 && k1 <= E;
    const long long off = frame_matrix_offset<BLOCK>(node_ptr, g, total);
    const int v0 = node_ptr[g], n = node_ptr[g + 1] - v0;
    if (off < 0 || n > kRerankMaxNodes || n > N_all - v0) {   // nothing can be ranked: nothing is predicted
        if (edges_ok)
            for (long long k = k0 + tid; k < k1; k += BLOCK) pred[k] = 0;
        return;
    }
    if (!edges_ok) return;
    const float* D = dist + off;
    for (int v = tid; v < n; v += BLOCK) s_cam[v] = cam[v0 + v], s_sel[v][0] = 0ull, s_sel[v][1] = 0ull;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += BLOCK / 64) {   // (the same trip count for every wave: the barriers are the workgroup's)
        const int i = i0 + wave;
        float* row = s_row[wave];
        if (i < n)
            for (int j = lane; j < n; j += 64) row[j] = D[i * n + j];
        __syncthreads();
        if (i < n) {
            const int ci = s_cam[i];
            for (int j = lane; j < n; j += 64) {
                if (s_cam[j] == ci) continue;
                const float dj = row[j];
                int pos = 0;
                for (int m = 0; m < n; ++m) {
                    const float dm = row[m];
                    pos += (s_cam[m] != ci && (dm < dj || (dm == dj && m < j))) ? 1 : 0;
                }
                if (pos < rank) atomicOr(&s_sel[i][j >> 6], 1ull << (j & 63));
            }
        }
        __syncthreads();
    }
    for (long long k = k0 + tid; k < k1; k += BLOCK) {
        const long long a = ei[k] - v0, b = ei[E + k] - v0;
        long long p = 0;
        if (a >= 0 && a < n && b >= 0 && b < n)   // an edge that leaves its frame is never predicted
            p = (mask_has(s_sel[a], (int)b) || mask_has(s_sel[b], (int)a)) ? 1 : 0;
        pred[k] = p;
    }
}

}  // namespace gnncca
