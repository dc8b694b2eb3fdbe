// identities_reentry.cuh -- the re-entry gallery (gnncca_reentry_update), included at the end of identities.hip after the linkers: a track
// born after a long absence gets the IDENTITY of the ended track it looks like.  frame_range, usable_count, wave_number, wave_min_lex,
// wave_sum_f64 and the host-known frame offsets (GapFrames) are the linkers', shared through link_common.cuh.
//
// The rule (include/gnncca_mpn.h has it in full, tests/reentry_oracle.py as loops): ring slot j mod S holds track j's running appearance
// sum, the frame and place of its latest cluster, its identity and a `continued` flag; a birth b of frame f may take over an ended track j
// with b - W <= j < b that still owns its slot, is not continued, has been absent for at least M + 2 frames (and at most max_age, and no
// farther than max_speed times the absence), at cosine distance dcos <= max_cos; mutual best per frame, ties to the smaller id / rank.
// An eligible track can no longer be continued by the linker, so its sum / last / pos are final: they are accumulated for the whole call
// first and looked at afterwards.  Only `continued` and the identities are serial in time.  Launches, 6 of them:
//   1. reentry_prep_kernel (one workgroup per frame): per batch row its ring slot (-1: not a usable cluster), whether it is a birth, its frame.
//   2. reentry_mark_kernel (a thread per ring slot + one workgroup more): the thread walks the call's rows in frame order and keeps its
//      slot's owner: a birth takes the slot (rule step 4), a cluster whose track owns the slot moves last / pos (step 5); per row it leaves
//      what launch 3 has to do with the sum (nothing, add, clear and add).  The extra workgroup numbers the births by a ballot scan; the
//      births of a call carry consecutive track ids in row order (every linker numbers fresh ids so) -- if they do not, the count is taken
//      as 0 and nobody re-enters.
//   3. reentry_accumulate_kernel ((256 columns, 64 slot groups)): a thread owns a column of the slots of its group and applies the marked
//      rows in frame order: the fp32 additions come out in the oracle's order.
//   4. reentry_norm_kernel (a wave per slot and per birth): the fp64 sum of squares of every owned sum row and of every birth's row, once
//      per call (lane-strided partial sums, then a butterfly: a fixed order).
//   5. reentry_cosine_kernel, the hot path: births x window tracks x R.  A workgroup takes 32 births against 64 consecutive track ids;
//      chunks of 32 columns of both sides' rows are staged in LDS (16-byte loads when R is a multiple of 4), a thread holds 2 x 4 fp64
//      accumulators in registers, and a pair's products are added in ascending column order by fused multiply-adds, whatever the tile: the
//      table is bitwise reproducible and does not depend on how a sequence is cut.  Entries failing the arithmetic tests (window, owner,
//      absence, age, speed, max_cos, NaN) are +inf; a tile without a candidate is filled without reading a row.  The grid is sized from N
//      and W; workgroups beyond the device-side birth count exit at once.
//   6. reentry_walk_kernel, grid = 1: the frames in order -- per frame the mutual best over table rows (no R-length load), `continued`,
//      the births' identities, the continued clusters' identities (from the batch or the identity history, never through the ring),
//      node_identity; at the end the identity history of the last M + 1 frames.  A __syncthreads() stands between a frame's writes and the
//      next frame's reads; arrays written and later read are plain pointers.
// Every loop is bounded by G, N, W, S or 64; a count that does not fit is taken as 0; no workgroup waits for another.
#pragma once

namespace gnncca {

constexpr int kReentryMaxWindow = GNNCCA_REENTRY_MAX_WINDOW;
constexpr int kReTB = 32, kReTS = 64, kReKC = 32, kReLd = kReKC + 4;   // the cosine tile: births, track ids, columns per chunk, LDS row stride
constexpr int kReGroups = 64;                                          // slot groups of the accumulate launch

// the ring of S slots: owner, identity, last int64 [S]; pos fp64 [S][2]; continued int32 [S]; sum fp32 [S][R] from a 256-byte boundary
__host__ __device__ inline size_t ring_sum_off(long long S) { return ((size_t)S * 44 + 255) / 256 * 256; }
struct Ring {
    long long* owner;
    long long* identity;
    long long* last;
    double* pos;
    int* continued;
    float* sum;
    __host__ __device__ Ring(char* base, long long S)
        : owner(reinterpret_cast<long long*>(base)), identity(owner + S), last(owner + 2 * S), pos(reinterpret_cast<double*>(owner + 3 * S)),
          continued(reinterpret_cast<int*>(base + (size_t)S * 40)), sum(reinterpret_cast<float*>(base + ring_sum_off(S))) {}
};

// the workspace: table fp64 [N][W], norms of the sum rows fp64 [S] and of the births fp64 [N], the births' track ids int64 [N], then
// int32 [N] each: slot, flags, frame, apply, birth_row (birth -> row), birth_idx (row -> birth, -1), and the birth count
struct ReentryWs {
    double* table;
    double* norm_slot;
    double* norm_birth;
    long long* birth_track;
    int *slot, *flags, *frame, *apply, *birth_row, *birth_idx, *n_births;
    __host__ __device__ ReentryWs(char* base, long long N, long long W, long long S)
        : table(reinterpret_cast<double*>(base)), norm_slot(table + (size_t)N * W), norm_birth(norm_slot + S),
          birth_track(reinterpret_cast<long long*>(norm_birth + N)), slot(reinterpret_cast<int*>(birth_track + N)), flags(slot + N),
          frame(flags + N), apply(frame + N), birth_row(apply + N), birth_idx(birth_row + N), n_births(birth_idx + N) {}
};
static size_t reentry_ws_bytes(long long N, long long W, long long S) {
    return round256(((size_t)N * W + S + 2 * (size_t)N) * 8 + (6 * (size_t)N + 1) * 4);
}

struct ReentryRule {
    double max_cos, max_speed;
    long long max_age, seen;   // seen: frames before this call
    int max_gap, has_max_age, has_max_speed, W;
    long long S;
};

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reentry_prep_kernel(const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                                           const long long* __restrict__ cluster_track, const int* __restrict__ matched_prev,
                                                           long long S, int P_lds, ReentryWs ws, long long* __restrict__ cluster_identity,
                                                           long long* __restrict__ reentered_from) {
    const int g = blockIdx.x;
    int v0, n;
    if (!frame_range(node_ptr, g, N_all, v0, n)) return;
    const int ca = usable_count(count, g, n, P_lds);
    for (int a = threadIdx.x; a < n; a += 256) {
        const int row = v0 + a;
        int slot = -1, birth = 0;
        if (a < ca) {
            const long long t = cluster_track[row];
            if (t >= 0) slot = (int)(t % S), birth = matched_prev[row] < 0;
        }
        ws.slot[row] = slot;
        ws.flags[row] = birth;
        ws.frame[row] = g;
        ws.apply[row] = 0;
        ws.birth_idx[row] = -1;
        cluster_identity[row] = -1;
        reentered_from[row] = -1;
    }
}

// ---- launch 2 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reentry_mark_kernel(int N_all, int G, const long long* __restrict__ cluster_track,
                                                           const double* __restrict__ pos, ReentryRule rule, Ring ring, ReentryWs ws) {
    const int tid = threadIdx.x;
    const long long S = rule.S;
    if ((long long)blockIdx.x * 256 >= S) {   // the workgroup after the slots': the births in row order
        __shared__ int s_n, s_bad;
        if (tid == 0) s_bad = 0;
        if (tid < 64) {
            const int c = wave_number(N_all, [&](int i) { const int sl = ws.slot[i]; return sl >= 0 && sl < S && ws.flags[i] == 1; },
                                      [&](int i, int k) { ws.birth_row[k] = i, ws.birth_track[k] = cluster_track[i]; });
            if (tid == 0) s_n = c;
        }
        __syncthreads();   // (the list was written by this workgroup: visible after the barrier)
        const int nb = s_n;
        int bad = 0;
        for (int k = tid; k < nb; k += 256) {
            const int i = ws.birth_row[k];
            bad |= ws.birth_track[k] != ws.birth_track[0] + k;
            ws.birth_idx[i] = k;
        }
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
        if (tid == 0) *ws.n_births = s_bad ? 0 : nb;
        return;
    }
    const long long s = (long long)blockIdx.x * 256 + tid;   // (a thread beyond S stays for the wave's shuffles: no row has its slot)
    const bool real = s < S;
    long long own = real ? ring.owner[s] : -1, last = real ? ring.last[s] : 0;
    double px = real ? ring.pos[2 * s] : 0.0, py = real ? ring.pos[2 * s + 1] : 0.0;
    int cont = real ? ring.continued[s] : 0;
    bool touched = false;
    const int lane = tid & 63;
    for (int base = 0; base < N_all; base += 64) {   // a wave reads 64 rows' slots at once, then every thread looks for its own among them
        const int mine = base + lane < N_all ? ws.slot[base + lane] : -1;
        if (!__ballot(mine >= 0)) continue;
        for (int l = 0; l < 64; ++l) {   // ascending rows: frame order
            if (__shfl(mine, l) != (int)s) continue;
            const int i = base + l;
            const long long t = cluster_track[i];
            const int g = ws.frame[i];
            int ap = 0;
            if (ws.flags[i] == 1) own = t, cont = 0, ap = 2;
            if (own == t && g >= 0 && g < G) {
                ap |= 1;
                last = rule.seen + g;
                px = pos[2 * (size_t)i], py = pos[2 * (size_t)i + 1];
            }
            ws.apply[i] = ap;
            touched = true;
        }
    }
    if (touched && real) {
        ring.owner[s] = own, ring.last[s] = last, ring.continued[s] = cont;
        ring.pos[2 * s] = px, ring.pos[2 * s + 1] = py;
    }
}

// ---- launch 3 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reentry_accumulate_kernel(int N_all, const float* __restrict__ emb, int R, long long S, Ring ring,
                                                                 ReentryWs ws) {
    const int col = blockIdx.x * 256 + threadIdx.x, group = blockIdx.y, lane = threadIdx.x & 63;
    for (int base = 0; base < N_all; base += 64) {
        const int i = base + lane;
        int ap = 0, sl = -1;
        if (i < N_all) ap = ws.apply[i], sl = ws.slot[i];
        unsigned long long todo = __ballot(ap != 0 && sl >= 0 && sl < S && sl % kReGroups == group);
        while (todo) {   // ascending rows: frame order
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int a = __shfl(ap, l), s = __shfl(sl, l);
            if (col < R) {
                float* cell = ring.sum + (size_t)s * R + col;
                float v = (a & 2) ? 0.f : *cell;
                if (a & 1) v = v + emb[(size_t)(base + l) * R + col];
                *cell = v;
            }
        }
    }
}

// ---- launch 4 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reentry_norm_kernel(int N_all, const float* __restrict__ emb, int R, long long S, Ring ring, ReentryWs ws) {
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const float* row;
    double* out;
    if (w < S) {
        if (ring.owner[w] < 0) return;
        row = ring.sum + (size_t)w * R, out = ws.norm_slot + w;
    } else {
        const long long k = w - S;
        int nb = *ws.n_births;
        nb = nb >= 0 && nb <= N_all ? nb : 0;
        if (k >= nb) return;
        const int i = ws.birth_row[k];
        if (i < 0 || i >= N_all) return;
        row = emb + (size_t)i * R, out = ws.norm_birth + k;
    }
    double acc = 0.0;
    for (int c = lane; c < R; c += 64) {
        const double x = (double)row[c];
        acc += x * x;
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) *out = acc;
}

// ---- launch 5: the table ----------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void reentry_cosine_kernel(int N_all, int G, const double* __restrict__ pos, const float* __restrict__ emb,
                                                             int R, ReentryRule rule, Ring ring, ReentryWs ws) {
    __shared__ float sA[kReTB][kReLd], sB[kReTS][kReLd];
    __shared__ int s_row[kReTB], s_slot[kReTS];
    __shared__ long long s_f[kReTB], s_last[kReTS];
    __shared__ double s_ax[kReTB], s_ay[kReTB], s_na[kReTB], s_bx[kReTS], s_by[kReTS], s_nb[kReTS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int nb = *ws.n_births;
    nb = nb >= 0 && nb <= N_all ? nb : 0;
    const int k0 = blockIdx.y * kReTB;
    if (k0 >= nb) return;
    const int W = rule.W;
    const long long S = rule.S, b0 = ws.birth_track[k0];   // the births of a call are consecutive: birth k0 + y has track b0 + y
    const long long J0 = b0 - W + (long long)blockIdx.x * kReTS;
    if (tid < kReTB) {
        const int k = k0 + tid;
        int row = k < nb ? ws.birth_row[k] : -1;
        if (row < 0 || row >= N_all) row = -1;
        int g = row >= 0 ? ws.frame[row] : 0;
        if (g < 0 || g >= G) row = -1, g = 0;
        s_row[tid] = row;
        s_f[tid] = rule.seen + g;
        s_ax[tid] = row >= 0 ? pos[2 * (size_t)row] : 0.0;
        s_ay[tid] = row >= 0 ? pos[2 * (size_t)row + 1] : 0.0;
        s_na[tid] = row >= 0 ? ws.norm_birth[k] : 0.0;
    } else if (tid >= 64 && tid < 64 + kReTS) {
        const int x = tid - 64;
        const long long j = J0 + x;
        int slot = -1;
        if (j >= 0) {
            slot = (int)(j % S);
            if (ring.owner[slot] != j) slot = -1;
        }
        s_slot[x] = slot;
        s_last[x] = slot >= 0 ? ring.last[slot] : 0;
        s_bx[x] = slot >= 0 ? ring.pos[2 * (size_t)slot] : 0.0;
        s_by[x] = slot >= 0 ? ring.pos[2 * (size_t)slot + 1] : 0.0;
        s_nb[x] = slot >= 0 ? ws.norm_slot[slot] : 0.0;
    }
    __syncthreads();
    // the arithmetic part of the rule for this thread's 2 x 4 pairs: birth y = ty + 16 i, track x = tx + 16 j
    bool elig[2][4];
    int any = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int y = ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = tx + 16 * j;
            const int c = blockIdx.x * kReTS + x - y;   // the pair's column of the table: track b - W + c
            bool ok = s_row[y] >= 0 && s_slot[x] >= 0 && c >= 0 && c < W;
            const long long away = s_f[y] - s_last[x];
            ok = ok && away >= rule.max_gap + 2 && (!rule.has_max_age || away <= rule.max_age);
            if (ok && rule.has_max_speed) {
                const double dx = s_ax[y] - s_bx[x], dy = s_ay[y] - s_by[x];
                ok = sqrt(dx * dx + dy * dy) <= rule.max_speed * (double)away;
            }
            elig[i][j] = ok;
            any |= ok;
        }
    }
    double acc[2][4] = {};
    if (__syncthreads_or(any)) {   // (uniform) a tile without a candidate reads no row
        for (int kc = 0; kc < R; kc += kReKC) {
            if (VEC) {   // R % 4 == 0: every row starts on a 16-byte boundary
                for (int e = tid; e < (kReTB + kReTS) * (kReKC / 4); e += 256) {
                    const int r = e / (kReKC / 4), q = (e % (kReKC / 4)) * 4;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (r < kReTB) {
                        if (s_row[r] >= 0 && kc + q < R) v = *reinterpret_cast<const float4*>(emb + (size_t)s_row[r] * R + kc + q);
                        *reinterpret_cast<float4*>(&sA[r][q]) = v;
                    } else {
                        const int x = r - kReTB;
                        if (s_slot[x] >= 0 && kc + q < R) v = *reinterpret_cast<const float4*>(ring.sum + (size_t)s_slot[x] * R + kc + q);
                        *reinterpret_cast<float4*>(&sB[x][q]) = v;
                    }
                }
            } else {
                for (int e = tid; e < (kReTB + kReTS) * kReKC; e += 256) {
                    const int r = e / kReKC, q = e % kReKC;
                    float v = 0.f;
                    if (r < kReTB) {
                        if (s_row[r] >= 0 && kc + q < R) v = emb[(size_t)s_row[r] * R + kc + q];
                        sA[r][q] = v;
                    } else {
                        const int x = r - kReTB;
                        if (s_slot[x] >= 0 && kc + q < R) v = ring.sum[(size_t)s_slot[x] * R + kc + q];
                        sB[x][q] = v;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kReKC; q += 4) {   // columns beyond R are zero on both sides: they add +0
                float4 a[2], b[4];
#pragma unroll
                for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const float4*>(&sA[ty + 16 * i][q]);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(&sB[tx + 16 * j][q]);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        double v = acc[i][j];
                        v = __builtin_fma((double)a[i].x, (double)b[j].x, v);
                        v = __builtin_fma((double)a[i].y, (double)b[j].y, v);
                        v = __builtin_fma((double)a[i].z, (double)b[j].z, v);
                        v = __builtin_fma((double)a[i].w, (double)b[j].w, v);
                        acc[i][j] = v;
                    }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int y = ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = tx + 16 * j;
            const int c = blockIdx.x * kReTS + x - y;
            if (k0 + y >= nb || c < 0 || c >= W) continue;
            double v = __builtin_inf();
            if (elig[i][j]) {
                const double na = s_na[y], nbq = s_nb[x];
                const double dcos = (na == 0.0 || nbq == 0.0) ? 1.0 : 1.0 - acc[i][j] / (sqrt(na) * sqrt(nbq));
                if (dcos <= rule.max_cos) v = dcos;   // (a NaN is admissible with nobody)
            }
            ws.table[(size_t)(k0 + y) * W + c] = v;
        }
    }
}

// ---- launch 6: the walk -------------------------------------------------------------------------------------------------------------------
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void reentry_walk_kernel(const int* __restrict__ node_ptr, int N_all, int G, const int* __restrict__ count,
                                                             const int* __restrict__ rank, const long long* __restrict__ cluster_track,
                                                             const int* __restrict__ matched_prev, const int* __restrict__ matched_gap,
                                                             ReentryRule rule, Ring ring, ReentryWs ws, const long long* __restrict__ hist_in,
                                                             GapFrames in, long long* hist_out, GapFrames out, int P_lds,
                                                             long long* cluster_identity, long long* __restrict__ node_identity,
                                                             long long* __restrict__ reentered_from) {
    extern __shared__ int s_dyn[];
    __shared__ int s_nbf, s_kfirst;
    int* fwd = s_dyn;           // [birth of the frame] -> its best column of the table
    int* bwd = s_dyn + P_lds;   // [track - first candidate track] -> its best birth of the frame
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = rule.W;
    const long long S = rule.S;
    int nb = *ws.n_births;
    nb = nb >= 0 && nb <= N_all ? nb : 0;

    for (int t = 0; t < G; ++t) {
        int v0, n;
        const bool ok = frame_range(node_ptr, t, N_all, v0, n);
        const int ca = ok ? usable_count(count, t, n, P_lds) : 0;
        if (tid < 64) {   // the frame's births: consecutive entries of the call's list, in rank order
            const int c = wave_number(ca, [&](int a) { const int k = ws.birth_idx[v0 + a]; return k >= 0 && k < nb; },
                                      [&](int a, int i) { if (i == 0) s_kfirst = ws.birth_idx[v0 + a]; });
            if (tid == 0) s_nbf = c;
        }
        __syncthreads();
        int nbf = s_nbf;
        const int kf = nbf > 0 ? s_kfirst : 0;
        if (kf + nbf > nb) nbf = 0;
        const long long bfirst = nbf > 0 ? ws.birth_track[kf] : 0, jbase = bfirst - W;   // candidate c of the frame is track jbase + c
        const int ncand = nbf > 0 ? W + nbf - 1 : 0;
        for (int i = wave; i < nbf; i += BLOCK / 64) {   // a wave takes a birth, its lanes the columns
            const double* trow = ws.table + (size_t)(kf + i) * W;
            double best = __builtin_inf();
            int bi = INT_MAX;
            const long long j0 = jbase + i + lane;   // this lane's first track; its slot moves on by 64 (mod S) per pass
            unsigned slot = (unsigned)((j0 % S + S) % S);
            const unsigned step = (unsigned)(64 % S);
            for (int c0 = lane; c0 < W; c0 += 4 * 64) {   // four entries and their tracks' flags in flight; a lane's columns ascend
                double v[4];
                int taken[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    v[u] = c0 + 64 * u < W ? trow[c0 + 64 * u] : __builtin_inf();
                    taken[u] = ring.continued[slot];
                    slot = (slot + step) % (unsigned)S;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + 64 * u;
                    if (v[u] < best && j0 + (c - lane) >= 0 && !taken[u]) best = v[u], bi = c;
                }
            }
            const int b = wave_min_lex(best, bi).i;
            if (lane == 0) fwd[i] = b == INT_MAX ? -1 : b;
        }
        for (int c0 = tid; c0 < ncand; c0 += 2 * BLOCK) {   // a thread takes a track (two at a time): birth i sees it in column c - i
            double best[2] = {__builtin_inf(), __builtin_inf()};
            int bi[2] = {-1, -1};
            bool open[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = c0 + h * BLOCK;
                const long long j = jbase + c;
                open[h] = c < ncand && j >= 0 && !ring.continued[j >= 0 ? j % S : 0];
            }
            for (int i0 = 0; i0 < nbf; i0 += 8) {   // eight loads per track in flight
                double v[2][8];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + u, col = c0 + h * BLOCK - i;
                        v[h][u] = (open[h] && i < nbf && col >= 0 && col < W) ? ws.table[(size_t)(kf + i) * W + col] : __builtin_inf();
                    }
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (v[h][u] < best[h]) best[h] = v[h][u], bi[h] = i0 + u;   // (births ascend: the smaller rank stays on a tie)
            }
            bwd[c0] = bi[0];
            if (c0 + BLOCK < ncand) bwd[c0 + BLOCK] = bi[1];
        }
        __syncthreads();   // (every read of `continued` above comes before the writes below)
        for (int a = tid; a < ca; a += BLOCK) {
            const int row = v0 + a, k = ws.birth_idx[row];
            long long id = -1;
            if (matched_prev[row] < 0) {
                id = cluster_track[row];
                const int i = k - kf;
                if (k >= 0 && i >= 0 && i < nbf) {
                    const int col = fwd[i];
                    if (col >= 0 && bwd[col + i] == i) {
                        const long long j = jbase + i + col;
                        id = ring.identity[j % S];
                        ring.continued[j % S] = 1;
                        reentered_from[row] = j;
                    }
                }
                if (id >= 0 && ring.owner[cluster_track[row] % S] == cluster_track[row]) ring.identity[cluster_track[row] % S] = id;   // (step 4)
            } else {   // continued by the linker: the identity of its predecessor's row, from the batch or the history
                const int m = matched_prev[row], tp = t - 1 - matched_gap[row];
                if (tp >= 0 && tp < t) {
                    int u0, un;
                    if (frame_range(node_ptr, tp, N_all, u0, un) && m < un) id = cluster_identity[u0 + m];
                } else if (tp < 0 && in.n + tp >= 0) {
                    const int f = in.n + tp;
                    if (m < in.off[f + 1] - in.off[f]) id = hist_in[in.off[f] + m];
                }
            }
            cluster_identity[row] = id;
        }
        __syncthreads();   // (the next frame reads this frame's identities and flags)
        for (int v = tid; v < n; v += BLOCK) {
            const int r = rank[v0 + v];
            node_identity[v0 + v] = (r >= 0 && r < ca) ? cluster_identity[v0 + r] : -1;
        }
    }
    // the identity history of the last frames: slot j of the new one is a batch frame or a frame of the old one
    const int first_kept = G - out.n;
    for (int j = 0; j < out.n; ++j) {
        const int g = first_kept + j, orow = out.off[j], cap = out.off[j + 1] - orow;
        if (g >= 0) {
            int v0, n;
            const bool ok = frame_range(node_ptr, g, N_all, v0, n);
            const int ca = ok ? usable_count(count, g, n, P_lds) : 0;
            for (int a = tid; a < cap; a += BLOCK) hist_out[orow + a] = a < ca ? cluster_identity[v0 + a] : -1;
        } else {
            const int f = in.n + g;
            const int have = f >= 0 ? in.off[f + 1] - in.off[f] : 0;
            for (int a = tid; a < cap; a += BLOCK) hist_out[orow + a] = a < have ? hist_in[in.off[f] + a] : -1;
        }
    }
}

}  // namespace gnncca

extern "C" {

size_t gnncca_reentry_state_bytes(int64_t n_slots, int32_t reid_dim) {
    if (n_slots < 1 || reid_dim < 1) return 0;
    return gnncca::round256(gnncca::ring_sum_off(n_slots) + (size_t)n_slots * (size_t)reid_dim * sizeof(float));
}

size_t gnncca_reentry_workspace_bytes(int64_t n_nodes, int32_t window, int32_t max_batch) {
    if (n_nodes < 0 || window < 1 || window > gnncca::kReentryMaxWindow || max_batch < 1) return 0;
    return gnncca::reentry_ws_bytes(n_nodes, window, (long long)window + max_batch);
}

int gnncca_reentry_update(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* rank, const double* pos, const float* emb,
                          int32_t reid_dim, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, const int64_t* cluster_track,
                          const int32_t* matched_prev, const int32_t* matched_gap, int32_t max_gap, double max_cos, int32_t window,
                          int32_t max_batch, int32_t has_max_age, int64_t max_age, int32_t has_max_speed, double max_speed,
                          int64_t frames_seen, void* ring_state, const int64_t* hist_in, const int32_t* hist_in_frame_rows,
                          int32_t hist_in_frames, int64_t* hist_out, const int32_t* hist_out_frame_rows, int32_t hist_out_frames,
                          int64_t* cluster_identity, int64_t* node_identity, int64_t* reentered_from, void* workspace,
                          size_t workspace_bytes, gnncca_stream_t stream) {
    using namespace gnncca;
    if (n_nodes < 0 || n_frames < 0 || reid_dim < 1 || frames_seen < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_gap < 0 || max_gap > kTrackMaxGap) return GNNCCA_ERR_INVALID_ARG;
    if (!(max_cos >= 0.0 && max_cos <= 2.0)) return GNNCCA_ERR_INVALID_ARG;
    if (window < 1 || window > kReentryMaxWindow || max_batch < 1 || n_nodes > max_batch) return GNNCCA_ERR_INVALID_ARG;
    if (has_max_age && max_age < max_gap + 2) return GNNCCA_ERR_INVALID_ARG;
    if (has_max_speed && (!(max_speed > 0.0) || !(max_speed < __builtin_inf()))) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kTrackMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (hist_in_frames < 0 || hist_in_frames > max_gap + 1 || (hist_in_frames > 0 && (!hist_in || !hist_in_frame_rows))) return GNNCCA_ERR_INVALID_ARG;
    GapFrames in, out;
    if (!gap_frames(hist_in_frame_rows, hist_in_frames, in)) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;   // no time passes: the caller keeps its state
    const long long seen = (long long)in.n + n_frames;
    const int kept = (int)(seen < max_gap + 1 ? seen : max_gap + 1);
    if (hist_out_frames != kept || !hist_out_frame_rows || !gap_frames(hist_out_frame_rows, kept, out)) return GNNCCA_ERR_INVALID_ARG;
    if (!node_ptr_dev || !count || !ring_state || !hist_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!rank || !pos || !emb || !cluster_track || !matched_prev || !matched_gap || !cluster_identity || !node_identity || !reentered_from))
        return GNNCCA_ERR_INVALID_ARG;
    if (workspace_bytes < gnncca_reentry_workspace_bytes(n_nodes, window, max_batch)) return GNNCCA_ERR_WORKSPACE;
    const long long S = (long long)window + max_batch;
    if (S >= (1ll << 31) - 256) return GNNCCA_ERR_UNSUPPORTED;
    int P = 64;
    while (P < max_frame_nodes) P <<= 1;
    const ReentryRule rule{max_cos, max_speed, (long long)max_age, (long long)frames_seen, (int)max_gap, has_max_age != 0, has_max_speed != 0,
                           (int)window, S};
    const Ring ring(static_cast<char*>(ring_state), S);
    const ReentryWs ws(static_cast<char*>(workspace), n_nodes, window, S);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int N = (int)n_nodes, R = (int)reid_dim, G = (int)n_frames;
    const long long* track = reinterpret_cast<const long long*>(cluster_track);
    long long* ident = reinterpret_cast<long long*>(cluster_identity);
    long long* reent = reinterpret_cast<long long*>(reentered_from);
    hipLaunchKernelGGL(reentry_prep_kernel, dim3((unsigned)G), dim3(256), 0, st, node_ptr_dev, N, count, track, matched_prev, S, P, ws, ident, reent);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(reentry_mark_kernel, dim3((unsigned)((S + 255) / 256 + 1)), dim3(256), 0, st, N, G, track, pos, rule, ring, ws);
    HIP_TRY(hipGetLastError());
    if (N > 0) {
        hipLaunchKernelGGL(reentry_accumulate_kernel, dim3((unsigned)((R + 255) / 256), kReGroups), dim3(256), 0, st, N, emb, R, S, ring, ws);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(reentry_norm_kernel, dim3((unsigned)((S + N + 3) / 4)), dim3(256), 0, st, N, emb, R, S, ring, ws);
        HIP_TRY(hipGetLastError());
        const dim3 grid((unsigned)((window + kReTB + kReTS - 1) / kReTS), (unsigned)((N + kReTB - 1) / kReTB));
        if (R % 4 == 0) hipLaunchKernelGGL((reentry_cosine_kernel<true>), grid, dim3(256), 0, st, N, G, pos, emb, R, rule, ring, ws);
        else hipLaunchKernelGGL((reentry_cosine_kernel<false>), grid, dim3(256), 0, st, N, G, pos, emb, R, rule, ring, ws);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((reentry_walk_kernel<1024>), dim3(1), dim3(1024), (size_t)(2 * P + window) * sizeof(int), st, node_ptr_dev, N, G, count, rank,
                       track, matched_prev, matched_gap, rule, ring, ws, reinterpret_cast<const long long*>(hist_in), in,
                       reinterpret_cast<long long*>(hist_out), out, P, ident, reinterpret_cast<long long*>(node_identity), reent);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
