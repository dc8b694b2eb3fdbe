#pragma once
// SURVEY.md 8f row N1, backward: gradients of the graph build with respect to the RAW embeddings (the reference's statements are plain
// torch ops -- F.normalize(dim=0) at train.py:257-259 / inference.py:189-190, F.pairwise_distance and F.cosine_similarity of gathered reid
// rows at train.py:306-308 / inference.py:222-226 -- so with the no_grad around its CNN removed, autograd carries the association loss
// back to a ReID head through them).  Two pieces, both without atomics, fp32, bit for bit the same from run to run:
//
// (a) edges_bwd_*: d loss / d r [N][R] of the normalised reid table r from d loss / d edge_attr (its `emb` and `cos` columns).
//     For an edge e = (i -> j), a = r_i, b = r_j, n_x = max(||x||, 1e-8):
//        emb_e = ||a - b + 1e-6||          d emb / d a = (a - b + 1e-6) / emb_e = -d emb / d b      (0 where emb_e == 0)
//        cos_e = a.b / (n_a n_b)           d cos / d a = b / (n_a n_b) - cos_e a / n_a^2            (and the same with a, b swapped)
//     Every frame holds e = (i -> j) and e' = (j -> i), so with p = g_emb[e] / emb[e], q = g_cos[e] (primes: the reverse edge)
//        grad_r[i] = sum_j C[i][j] r_j + alpha_i r_i + 1e-6 beta_i
//        C[i][j]   = -(p + p') + (q + q') / (n_i n_j)               (zero inside a camera and across frames)
//        alpha_i   = sum_j (p + p') - (q cos_e + q' cos_e') / n_i^2
//        beta_i    = sum_j (p - p')
//     The slot of an edge follows from the plan: e(i -> j) = edge_ptr[pos_i] + (j - frame start) - (nodes of i's camera below j), where
//     pos_i, i's position in src_order, is a ballot rank over the frame's cameras (edges_bwd_prep_kernel) and the last term is a lower
//     bound in i's camera block of src_order (sorted by node id; log2(camera size) steps) -- the edge list itself is never searched.
//     A row whose norm is under the 1e-8 clamp is OUTSIDE the parity contract (torch differentiates through the clamp; here the clamped
//     norm simply takes the norm's place): the result is finite, not the reference's.
//     Because the emb term is evaluated as (sum_j w) r_i - sum_j w r_j rather than sum_j w (r_i - r_j), two nearly identical rows lose
//     about |r| / emb_e ulps of their emb gradient; the matrix form is what lets a frame's rows be read once per tile.
//
//     Shape: workgroup = 16 consecutive nodes x a column slice (128 threads, four columns each when R % 4 == 0 and the tables are
//     16-byte aligned, else one).  It walks the nodes of the frames its rows belong to in chunks of 64: the 16 x 64 block of C (and of
//     the alpha / beta terms) is built in LDS, one entry per thread and round, then every thread streams its columns of the chunk's
//     64 rows once and updates its 16 accumulators from LDS broadcasts, j ascending.  VALU, not the fp32 matrix pipe of
//     input_grads.cuh: the product is 2 n_g R flops per node (0.1 GFLOP for a 64-frame Terrace batch), three orders of magnitude under
//     what the vector ALUs deliver in the time the 10 MB table takes to stream -- the kernel is bound by the table traffic and the
//     latency of the C build, which an MFMA form would not change.  (Not A/B-measured against an MFMA form: none was written.)
//
// (b) colnorm_bwd_*: backward of y = x / nrm_c, nrm_c = max(||x[:, c]||, 1e-12):  gx = (gy - y s_c) / nrm_c,  s_c = sum_rows gy y.
//     The norm is recomputed from x with the forward's own ordered sums (64-row chunks, fma chain, four ordered quarters), s_c as
//     (sum_rows gy x) / nrm_c with the same ordering; the one-launch form (<= 4096 rows, up to two matrices) and the three-kernel
//     form perform the same operations in the same order.  The forward kernels are untouched.
// Part of the translation unit graph_build.hip.

namespace gnncca {

struct __attribute__((aligned(16))) NodeAux {
    float nrm;   // max(||r_i||, 1e-8)
    int pos;     // position of node i in src_order
    int cs, ce;  // [cs, ce): the positions of i's camera inside its frame
};

// One wave per node: the row norm (butterfly sum: the same value in every lane, the same bits every run) and the camera ballot ranks.
__global__ __launch_bounds__(256) void edges_bwd_prep_kernel(const gnncca_frames fr, const float* __restrict__ reid, int R, int N,
                                                             NodeAux* __restrict__ aux) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const int g = fr.graph_of[i];
    const int gs = fr.graph_ptr[g], ge = fr.graph_ptr[g + 1];
    const int ci = fr.cam[i];
    int below = 0, same = 0, same_before = 0;
    for (int j0 = gs; j0 < ge; j0 += 64) {
        const int j = j0 + lane;
        const bool inb = j < ge;
        const int cj = inb ? fr.cam[j] : 0;
        below += __popcll(__ballot(inb && cj < ci));   // cameras in ascending id: np.unique's order (gnncca_plan_frames)
        same += __popcll(__ballot(inb && cj == ci));
        same_before += __popcll(__ballot(inb && cj == ci && j < i));
    }
    const float* __restrict__ ri = reid + (size_t)i * R;
    float s = 0.f;
    if ((R & 3) == 0 && (reinterpret_cast<uintptr_t>(reid) & 15) == 0) {
        for (int d = lane * 4; d < R; d += 256) {
            const float4 a = *reinterpret_cast<const float4*>(ri + d);
            s = fmaf(a.x, a.x, s), s = fmaf(a.y, a.y, s), s = fmaf(a.z, a.z, s), s = fmaf(a.w, a.w, s);
        }
    } else {
        for (int d = lane; d < R; d += 64) s = fmaf(ri[d], ri[d], s);
    }
    s = wave_sum(s);
    if (lane == 0) {
        NodeAux a;
        a.nrm = fmaxf(sqrtf(s), 1e-8f);
        a.pos = gs + below + same_before;
        a.cs = gs + below;
        a.ce = gs + below + same;
        aux[i] = a;
    }
}

constexpr int kGgRows = 16, kGgChunk = 64, kGgThreads = 128;

// number of entries of the ascending run src_order[lo, hi) that are < v
__device__ __forceinline__ int count_below(const int32_t* __restrict__ src_order, int lo, int hi, int v) {
    const int lo0 = lo;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (src_order[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo - lo0;
}

// slot of the edge (source at position `pos` -> j) in a pruned edge list (gnncca_build_edges_topk): a search in the source's run of
// ascending destination ids dst[edge_ptr[pos], edge_ptr[pos + 1]); -1 when the source did not keep j
__device__ __forceinline__ long long find_edge(const int32_t* __restrict__ edge_ptr, const long long* __restrict__ dst, long long E, int pos,
                                               int j) {
    long long lo = edge_ptr[pos], hi = edge_ptr[pos + 1];
    if (lo < 0 || hi > E) return -1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (dst[mid] < j) lo = mid + 1; else hi = mid;
    }
    return lo < edge_ptr[pos + 1] && dst[lo] == j ? lo : -1;
}

// PRUNED (gnncca_build_edges_topk_backward): `dst` is the destination row of the forward's edge_index and fr.edge_ptr counts the kept
// edges; an edge the selection dropped has p = q = 0.  Every other statement, and with it the order of every sum, is the dense one.
template <int MODE, bool VEC, bool PRUNED>
__global__ __launch_bounds__(kGgThreads) void edges_bwd_kernel(const gnncca_frames fr, const float* __restrict__ reid, int R, int N,
                                                               long long E, const NodeAux* __restrict__ aux,
                                                               const float* __restrict__ attr, const float* __restrict__ gattr,
                                                               const long long* __restrict__ dst, float* __restrict__ grad_r) {
    constexpr int NA = MODE == GNNCCA_EDGE_ATTR_FULL ? 4 : 2, CE = NA - 2, CC = NA - 1;   // columns of emb and cos
    constexpr int W = VEC ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float s_c[kGgChunk][kGgRows];
    __shared__ float s_a[kGgChunk][kGgRows], s_b[kGgChunk][kGgRows];
    __shared__ float s_alpha[kGgRows], s_beta[kGgRows];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * kGgRows;
    const int rows = min(kGgRows, N - n0);
    const int jlo = fr.graph_ptr[fr.graph_of[n0]], jhi = fr.graph_ptr[fr.graph_of[n0 + rows - 1] + 1];
    const int col = (blockIdx.y * kGgThreads + tid) * W;
    const bool col_ok = col < R;
    float acc[kGgRows][W];
#pragma unroll
    for (int t = 0; t < kGgRows; ++t)
#pragma unroll
        for (int w = 0; w < W; ++w) acc[t][w] = 0.f;
    float run = 0.f;   // threads 0 .. 15: alpha of row tid; 16 .. 31: beta of row tid - 16
    for (int jc = jlo; jc < jhi; jc += kGgChunk) {
        if (jc > jlo) __syncthreads();   // the previous chunk's block has been read
        for (int idx = tid; idx < kGgRows * kGgChunk; idx += kGgThreads) {
            const int t = idx & (kGgRows - 1), jj = idx / kGgRows;
            const int i = n0 + t, j = jc + jj;
            float c = 0.f, a = 0.f, b = 0.f;
            if (t < rows && j < jhi) {
                const int gi = fr.graph_of[i];
                if (gi == fr.graph_of[j] && fr.cam[i] != fr.cam[j]) {
                    const int gs = fr.graph_ptr[gi];
                    const NodeAux ai = aux[i], aj = aux[j];
                    if (PRUNED) {
                        const long long e = find_edge(fr.edge_ptr, dst, E, ai.pos, j), er = find_edge(fr.edge_ptr, dst, E, aj.pos, i);
                        const float emb = e >= 0 ? attr[e * NA + CE] : 0.f, embr = er >= 0 ? attr[er * NA + CE] : 0.f;
                        const float p = emb != 0.f ? gattr[e * NA + CE] / emb : 0.f;
                        const float pr = embr != 0.f ? gattr[er * NA + CE] / embr : 0.f;
                        const float q = e >= 0 ? gattr[e * NA + CC] : 0.f, qr = er >= 0 ? gattr[er * NA + CC] : 0.f;
                        const float ps = p + pr;
                        c = (q + qr) / (ai.nrm * aj.nrm) - ps;
                        a = ps - fmaf(q, e >= 0 ? attr[e * NA + CC] : 0.f, qr * (er >= 0 ? attr[er * NA + CC] : 0.f)) / (ai.nrm * ai.nrm);
                        b = p - pr;
                    } else {
                        const long long e = (long long)fr.edge_ptr[ai.pos] + (j - gs) - count_below(fr.src_order, ai.cs, ai.ce, j);
                        const long long er = (long long)fr.edge_ptr[aj.pos] + (i - gs) - count_below(fr.src_order, aj.cs, aj.ce, i);
                        if ((unsigned long long)e < (unsigned long long)E && (unsigned long long)er < (unsigned long long)E) {
                            const float emb = attr[e * NA + CE], embr = attr[er * NA + CE];
                            const float p = emb != 0.f ? gattr[e * NA + CE] / emb : 0.f;
                            const float pr = embr != 0.f ? gattr[er * NA + CE] / embr : 0.f;
                            const float q = gattr[e * NA + CC], qr = gattr[er * NA + CC];
                            const float ps = p + pr;
                            c = (q + qr) / (ai.nrm * aj.nrm) - ps;
                            a = ps - fmaf(q, attr[e * NA + CC], qr * attr[er * NA + CC]) / (ai.nrm * ai.nrm);
                            b = p - pr;
                        }
                    }
                }
            }
            s_c[jj][t] = c, s_a[jj][t] = a, s_b[jj][t] = b;
        }
        __syncthreads();
        const int nj = min(kGgChunk, jhi - jc);
        if (tid < kGgRows) {
            for (int jj = 0; jj < nj; ++jj) run += s_a[jj][tid];
        } else if (tid < 2 * kGgRows) {
            for (int jj = 0; jj < nj; ++jj) run += s_b[jj][tid - kGgRows];
        }
        if (col_ok) {
            for (int jj = 0; jj < nj; jj += 4) {
                float v[4][W];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float* __restrict__ pr = reid + (size_t)(jc + min(jj + u, nj - 1)) * R + col;
                    if (VEC) {
                        const float4 x = *reinterpret_cast<const float4*>(pr);
                        v[u][0] = x.x, v[u][W > 1 ? 1 : 0] = x.y, v[u][W > 1 ? 2 : 0] = x.z, v[u][W > 1 ? 3 : 0] = x.w;
                    } else {
                        v[u][0] = *pr;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (jj + u < nj) {
                        const float4* __restrict__ pc = reinterpret_cast<const float4*>(&s_c[jj + u][0]);
#pragma unroll
                        for (int t4 = 0; t4 < kGgRows / 4; ++t4) {
                            const float4 cc = pc[t4];
#pragma unroll
                            for (int w = 0; w < W; ++w) {
                                acc[4 * t4 + 0][w] = fmaf(cc.x, v[u][w], acc[4 * t4 + 0][w]);
                                acc[4 * t4 + 1][w] = fmaf(cc.y, v[u][w], acc[4 * t4 + 1][w]);
                                acc[4 * t4 + 2][w] = fmaf(cc.z, v[u][w], acc[4 * t4 + 2][w]);
                                acc[4 * t4 + 3][w] = fmaf(cc.w, v[u][w], acc[4 * t4 + 3][w]);
                            }
                        }
                    }
            }
        }
    }
    if (tid < kGgRows) s_alpha[tid] = run;
    else if (tid < 2 * kGgRows) s_beta[tid - kGgRows] = run;
    __syncthreads();
    if (!col_ok) return;
#pragma unroll
    for (int t = 0; t < kGgRows; ++t) {
        if (t >= rows) break;
        const float al = s_alpha[t], be = 1e-6f * s_beta[t];
        const float* __restrict__ pr = reid + (size_t)(n0 + t) * R + col;
        float* __restrict__ po = grad_r + (size_t)(n0 + t) * R + col;
        if (VEC) {
            const float4 x = *reinterpret_cast<const float4*>(pr);
            *reinterpret_cast<float4*>(po) = make_float4(fmaf(al, x.x, acc[t][0]) + be, fmaf(al, x.y, acc[t][W > 1 ? 1 : 0]) + be,
                                                         fmaf(al, x.z, acc[t][W > 1 ? 2 : 0]) + be, fmaf(al, x.w, acc[t][W > 1 ? 3 : 0]) + be);
        } else {
            *po = fmaf(al, *pr, acc[t][0]) + be;
        }
    }
}

// ---- (b) backward of the column normalisation ----------------------------------------------------------------------------------
// Three-kernel form, any number of rows.  scratch: sq [chunks][n_cols], norm [n_cols], dot [chunks][n_cols], s [n_cols].
__global__ __launch_bounds__(256) void colnorm_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ gy, long long n_rows,
                                                                  long long n_cols, float* __restrict__ sq, float* __restrict__ dot) {
    const long long r0 = (long long)blockIdx.y * kColChunk, r1 = min(r0 + kColChunk, n_rows);
    for (int q = 0; q < 4; ++q) {
        const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) * 4 + q;
        if (c >= n_cols) return;
        float s = 0.f, d = 0.f;
        for (long long r = r0; r < r1; ++r) {
            const float v = x[r * n_cols + c];
            s = fmaf(v, v, s);
            d = fmaf(gy[r * n_cols + c], v, d);
        }
        sq[(long long)blockIdx.y * n_cols + c] = s;
        dot[(long long)blockIdx.y * n_cols + c] = d;
    }
}

// colnorm_finish_kernel's four ordered quarter sums for both tables: norm = max(sqrt(.), 1e-12), s = dot / norm.
__global__ __launch_bounds__(256) void colnorm_bwd_finish_kernel(float* __restrict__ sq, float* __restrict__ dot, long long n_chunks,
                                                                 long long n_cols) {
    __shared__ float s_q[2][4][64];
    const int q = threadIdx.x >> 6, cl = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * 64 + cl;
    const long long per = (n_chunks + 3) / 4, k0 = min((long long)q * per, n_chunks), k1 = min(k0 + per, n_chunks);
    float s = 0.f, d = 0.f;
    if (c < n_cols)
        for (long long k = k0; k < k1; ++k) s += sq[k * n_cols + c], d += dot[k * n_cols + c];
    s_q[0][q][cl] = s, s_q[1][q][cl] = d;
    __syncthreads();
    if (q == 0 && c < n_cols) {
        const float nrm = fmaxf(sqrtf(((s_q[0][0][cl] + s_q[0][1][cl]) + s_q[0][2][cl]) + s_q[0][3][cl]), 1e-12f);
        sq[n_chunks * n_cols + c] = nrm;
        dot[n_chunks * n_cols + c] = (((s_q[1][0][cl] + s_q[1][1][cl]) + s_q[1][2][cl]) + s_q[1][3][cl]) / nrm;
    }
}

__device__ __forceinline__ float colnorm_bwd_value(float x, float gy, float nrm, float s) { return (gy - (x / nrm) * s) / nrm; }

__global__ __launch_bounds__(256) void colnorm_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                const float* __restrict__ norm, const float* __restrict__ s, long long total,
                                                                long long n_cols, float* __restrict__ gx) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < total) {
        const long long c = t % n_cols;
        gx[t] = colnorm_bwd_value(x[t], gy[t], norm[c], s[c]);
    }
}

// One launch, up to two matrices of <= 4096 rows: colnorm_fused_kernel's shape (16 columns per workgroup; chunk sums -> LDS, ordered
// quarters, then the rows strided over the chunk lanes) with the second sum riding along.
struct ColnormBwdJob {
    const float* x;
    const float* gy;
    float* gx;
    long long n_cols;
    int first_block;
};
__global__ __launch_bounds__(256) void colnorm_bwd_fused_kernel(const ColnormBwdJob j0, const ColnormBwdJob j1, long long n_rows) {
    __shared__ float s_part[2][kFusedMaxChunks][kFusedCols];
    __shared__ float s_q[2][4][kFusedCols];
    __shared__ float s_norm[kFusedCols], s_s[kFusedCols];
    const bool second = j1.x != nullptr && (int)blockIdx.x >= j1.first_block;
    const ColnormBwdJob& j = second ? j1 : j0;
    const long long n_cols = j.n_cols;
    const float* __restrict__ x = j.x;
    const float* __restrict__ gy = j.gy;
    float* __restrict__ gx = j.gx;
    const int tid = threadIdx.x, cl = tid >> 2, cg = tid & 3;
    const long long c = (long long)((int)blockIdx.x - j.first_block) * kFusedCols + 4 * cg;
    const int n_chunks = (int)((n_rows + kColChunk - 1) / kColChunk);
    const bool vec = (n_cols & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(gx)) & 15) == 0;
    for (int ch = cl; ch < n_chunks; ch += 64) {
        const long long r0 = (long long)ch * kColChunk, r1 = min(r0 + kColChunk, n_rows);
        f32x4g s = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            if (c < n_cols)
                for (long long r = r0; r < r1; r += 8) {
                    f32x4g v[8], w[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        v[u] = *reinterpret_cast<const f32x4g*>(x + min(r + u, r1 - 1) * n_cols + c);
                        w[u] = *reinterpret_cast<const f32x4g*>(gy + min(r + u, r1 - 1) * n_cols + c);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (r + u < r1)
#pragma unroll
                            for (int q = 0; q < 4; ++q) s[q] = fmaf(v[u][q], v[u][q], s[q]), d[q] = fmaf(w[u][q], v[u][q], d[q]);
                }
        } else {
            for (int q = 0; q < 4; ++q)
                if (c + q < n_cols)
                    for (long long r = r0; r < r1; ++r) {
                        const float v = x[r * n_cols + c + q];
                        s[q] = fmaf(v, v, s[q]);
                        d[q] = fmaf(gy[r * n_cols + c + q], v, d[q]);
                    }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) s_part[0][ch][4 * cg + q] = s[q], s_part[1][ch][4 * cg + q] = d[q];
    }
    __syncthreads();
    if (tid < 8 * kFusedCols) {
        const int which = tid / (4 * kFusedCols), q = (tid / kFusedCols) & 3, cc = tid % kFusedCols;
        const int per = (n_chunks + 3) / 4, k0 = min(q * per, n_chunks), k1 = min(k0 + per, n_chunks);
        float t = 0.f;
        for (int k = k0; k < k1; ++k) t += s_part[which][k][cc];
        s_q[which][q][cc] = t;
    }
    __syncthreads();
    if (tid < kFusedCols) {
        const float nrm = fmaxf(sqrtf(((s_q[0][0][tid] + s_q[0][1][tid]) + s_q[0][2][tid]) + s_q[0][3][tid]), 1e-12f);
        s_norm[tid] = nrm;
        s_s[tid] = (((s_q[1][0][tid] + s_q[1][1][tid]) + s_q[1][2][tid]) + s_q[1][3][tid]) / nrm;
    }
    __syncthreads();
    if (vec) {
        if (c < n_cols) {
            for (long long r = cl; r < n_rows; r += 64 * 4) {
                f32x4g v[4], w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    v[u] = *reinterpret_cast<const f32x4g*>(x + min(r + 64 * u, n_rows - 1) * n_cols + c);
                    w[u] = *reinterpret_cast<const f32x4g*>(gy + min(r + 64 * u, n_rows - 1) * n_cols + c);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (r + 64 * u < n_rows) {
                        f32x4g o;
#pragma unroll
                        for (int q = 0; q < 4; ++q) o[q] = colnorm_bwd_value(v[u][q], w[u][q], s_norm[4 * cg + q], s_s[4 * cg + q]);
                        *reinterpret_cast<f32x4g*>(gx + (r + 64 * u) * n_cols + c) = o;
                    }
            }
        }
    } else {
        for (int q = 0; q < 4; ++q)
            if (c + q < n_cols)
                for (long long r = cl; r < n_rows; r += 64)
                    gx[r * n_cols + c + q] = colnorm_bwd_value(x[r * n_cols + c + q], gy[r * n_cols + c + q], s_norm[4 * cg + q], s_s[4 * cg + q]);
    }
}

}  // namespace gnncca
