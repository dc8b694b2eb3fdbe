// link_common.cuh -- what every linker of identities.hip shares, written once; included by identities.hip after its `fp contract(off)`
// and before its kernels and the mode files (identities_gap.cuh, identities_assign.cuh, identities_motion.cuh):
//   the pair rule   pair_rule: d = sqrt(dx^2 + dy^2), the gate, the whole-wave fp64 cosine of the pairs inside it (wave_cosine_distance:
//                   lane-strided partial sums, then a butterfly), max_cos and cost = d / gate + lam * dcos.  best_partner (the mutual-best
//                   search of link_match_kernel, gap_level_kernel and motion_walk_kernel) and the table of gap_level_assign_kernel call it;
//   wave_min_lex    the lexicographic (value, index) minimum of a wave: ties to the smaller index;
//   wave_number     the ballot scan that numbers the entries where a predicate holds, in ascending order;
//   side_b          where a frame's partners of level k are: an earlier frame of the batch, or a frame of the carried history;
//   StateView       the arrays of a carried history state (without velocities, with them, or the Kalman linker's), write_slot one frame's
//                   rows into it;
//   cv_kalman_step  the constant-velocity Kalman filter's link rule (and cv_predicted_var, its predicted position variance): the
//                   smoother's walk and the Kalman linker's commit and variance gate (VarianceGate, pair_rule's extra predicate) run it;
//   level_dt        the time between the two frames of a (frame, level) table when the call has time stamps, and whether the table counts;
//   write_node_tracks, link_init_kernel, and on the host plan_history: the checks and the numbers both history entries need.
#pragma once

#include <type_traits>

namespace gnncca {

constexpr int kTrackMaxGap = GNNCCA_TRACK_MAX_GAP;
constexpr int kGapMaxFrames = kTrackMaxGap + 1;
constexpr int kTrackMaxOptimalNodes = GNNCCA_TRACK_MAX_OPTIMAL_FRAME_NODES;   // matching = 1: a frame pair's table lives in LDS

// `max_step` is the gate of the pairs at hand: the caller's max_step for adjacent frames, max_step * (k + 1) at level k.
struct LinkRule {
    double max_step, lam, max_cos;
    int need_emb, has_max_cos;
};

// a frame's cluster count if the summaries hold one that fits (0 otherwise: such a frame links to nothing)
__device__ __forceinline__ int usable_count(const int* __restrict__ count, int g, int n, int P_lds) {
    const int c = count[g];
    return (c >= 0 && c <= n && c <= P_lds) ? c : 0;
}

// ---- the pair rule ------------------------------------------------------------------------------------------------------------------------
// 1 - <er, ec> / (|er| |ec|) in fp64 by the whole wave (1 if a norm is 0): lane l sums the columns l, l + 64, ... in that order, then a
// butterfly, so every lane returns the same bits.  LOADS: the loads per side kept in flight; the order of a lane's additions is the same.
template <int LOADS>
__device__ __forceinline__ double wave_cosine_distance(const float* er, const float* ec, int R) {
    double dot = 0.0, na = 0.0, nb = 0.0;
    int k = threadIdx.x & 63;
    for (; LOADS > 1 && k + (LOADS - 1) * 64 < R; k += LOADS * 64) {
        float xs[LOADS], ys[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            xs[u] = er[k + 64 * u];
            ys[u] = ec[k + 64 * u];
        }
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const double x = (double)xs[u], y = (double)ys[u];
            dot += x * y;
            na += x * x;
            nb += y * y;
        }
    }
    for (; k < R; k += 64) {
        const double x = (double)er[k], y = (double)ec[k];
        dot += x * y;
        na += x * x;
        nb += y * y;
    }
    dot = wave_sum_f64(dot);
    na = wave_sum_f64(na);
    nb = wave_sum_f64(nb);
    return (na == 0.0 || nb == 0.0) ? 1.0 : 1.0 - dot / (sqrt(na) * sqrt(nb));
}

// An extra admissibility predicate of the pair rule, asked with d^2 = dx*dx + dy*dy inside the distance gate: none.  (pair_rule is called
// with d^2 alone, best_partner with the row and the column as well; an instantiation with AdmitAll compiles to the rule without one.)
struct AdmitAll {
    __device__ __forceinline__ bool operator()(double) const { return true; }
    __device__ __forceinline__ bool operator()(double, int, int) const { return true; }
};

// The variance gate of the Kalman linker: d^2 / s <= max_nis, s the predicted innovation variance of the pair's cluster of side B -- the
// search's row (BY_ROW) or its column -- which the caller has put into an LDS array, one per cluster of side B, before the search.  One fp64
// division; a NaN is admissible with nobody.  has == 0: no variance gate was asked for, the array is not read.
template <bool BY_ROW>
struct VarianceGate {
    const double* s;
    double max_nis;
    int has;
    __device__ __forceinline__ bool operator()(double d2, int r, int c) const { return !has || d2 / s[BY_ROW ? r : c] <= max_nis; }
};

// One pass of 64 columns against a row at (rx, ry) with appearance row er: this lane's column stands at (cx, cy) if `on`, and ec_of(j) is
// the appearance row of lane j's column.  use(cost) is called in the lanes whose pair is admissible (a NaN d is admissible with nobody):
// the division and the caller's use of the cost stay under one branch, which a pass without admissible pairs skips.  admit(d^2): one more
// predicate a pair inside the distance gate has to pass (AdmitAll: none).
template <int LOADS, class EmbOf, class Use, class Admit = AdmitAll>
__device__ __forceinline__ void pair_rule(bool on, double rx, double ry, double cx, double cy, const float* er, EmbOf ec_of, int R,
                                          const LinkRule& rule, Use use, Admit admit = Admit{}) {
    const int lane = threadIdx.x & 63;
    bool cand = false;
    double d = 0.0, dcos = 0.0;
    if (on) {
        const double dx = rx - cx, dy = ry - cy;
        const double d2 = dx * dx + dy * dy;
        d = sqrt(d2);
        cand = d <= rule.max_step;
        if constexpr (!std::is_same_v<Admit, AdmitAll>) cand = cand && admit(d2);
    }
    if (rule.need_emb) {
        unsigned long long todo = __ballot(cand);   // (uniform) the pairs inside the gate: the whole wave computes each cosine
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const double v = wave_cosine_distance<LOADS>(er, ec_of(j), R);
            if (lane == j) dcos = v;
        }
        if (rule.has_max_cos) cand = cand && dcos <= rule.max_cos;
    }
    if (cand) use(rule.need_emb ? d / rule.max_step + rule.lam * dcos : d / rule.max_step);
}

// the lexicographic minimum of (v, i) over the wave: the same in every lane.  (Values in, a value out: a search's running minimum stays
// a register that nobody holds a reference to.)
struct ValueIndex {
    double v;
    int i;
};
__device__ __forceinline__ ValueIndex wave_min_lex(double best, int bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ob < best || (ob == best && oi < bi)) best = ob, bi = oi;
    }
    return {best, bi};
}

// One side of a frame pair: n clusters at pos (+ steps * vel where vel is given), appearance rows emb; in a MASKED search entry i takes
// part iff mask[i] == free (otherwise every entry does).  Masks and velocities may have been written by this workgroup before a barrier.
struct LinkSide {
    const double* pos;
    const double* vel;
    const float* emb;
    const int* mask;
    int free, n;
};

// where an entry stands and whether it takes part: mask, position and velocity are loaded together and the mask is looked at
// afterwards (one round trip, not two)
struct Spot {
    double x, y;
    bool free;
};
template <bool MASKED>
__device__ __forceinline__ Spot side_at(const LinkSide& s, int i, double steps) {
    const int m = MASKED ? s.mask[i] : s.free;
    double x = s.pos[2 * (size_t)i], y = s.pos[2 * (size_t)i + 1];
    if (s.vel) {
        x = x + steps * s.vel[2 * (size_t)i];
        y = y + steps * s.vel[2 * (size_t)i + 1];
    }
    return {x, y, m == s.free};
}

// out[r] = the admissible free column of smallest cost for the free row r (ties: the smaller column), or -1.  A wave takes a row, its
// lanes the columns.  The minimum is over ORIGINAL ranks, never over compacted positions.  dx is squared, so which side is predicted
// does not change a bit of d.  admit(d^2, row, column): pair_rule's extra predicate for this search (AdmitAll: none).
template <int BLOCK, int LOADS, bool MASKED, class Admit = AdmitAll>
__device__ void best_partner(const LinkSide& rows, const LinkSide& cols, double steps, int R, const LinkRule& rule, int* out,
                             Admit admit = Admit{}) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < rows.n; r += BLOCK / 64) {
        const Spot row = side_at<MASKED>(rows, r, steps);
        if (!row.free) {   // (uniform in the wave)
            if (lane == 0) out[r] = -1;
            continue;
        }
        double best = __builtin_inf();
        int bi = INT_MAX;
        for (int base = 0; base < cols.n; base += 64) {
            const int c = base + lane;
            Spot col{0.0, 0.0, false};
            if (c < cols.n) col = side_at<MASKED>(cols, c, steps);
            const auto use = [&](double cost) {
                if (cost < best) best = cost, bi = c;   // (a lane's columns ascend: the smaller one stays on a tie)
            };
            const auto emb_of = [&](int j) { return cols.emb + (size_t)(base + j) * R; };
            if constexpr (std::is_same_v<Admit, AdmitAll>)
                pair_rule<LOADS>(col.free, row.x, row.y, col.x, col.y, rows.emb + (size_t)r * R, emb_of, R, rule, use);
            else
                pair_rule<LOADS>(col.free, row.x, row.y, col.x, col.y, rows.emb + (size_t)r * R, emb_of, R, rule, use,
                                 [&](double d2) { return admit(d2, r, c); });
        }
        const int b = wave_min_lex(best, bi).i;
        if (lane == 0) out[r] = b == INT_MAX ? -1 : b;
    }
}

// fwd[a] -> b and bwd[b] -> a for the two sides of a frame pair (the caller's barrier follows).  admit_ab / admit_ba: the extra predicate
// of the two searches, the same pairs seen from either side (AdmitAll: none).
template <int BLOCK, int LOADS, bool MASKED, class AdmitAB = AdmitAll, class AdmitBA = AdmitAll>
__device__ __forceinline__ void mutual_best(const LinkSide& a, const LinkSide& b, double steps, int R, const LinkRule& rule, int* fwd, int* bwd,
                                            AdmitAB admit_ab = AdmitAB{}, AdmitBA admit_ba = AdmitBA{}) {
    best_partner<BLOCK, LOADS, MASKED>(a, b, steps, R, rule, fwd, admit_ab);
    best_partner<BLOCK, LOADS, MASKED>(b, a, steps, R, rule, bwd, admit_ba);
}

// ---- numbering ----------------------------------------------------------------------------------------------------------------------------
// One wave: the entries i < c with on(i) get put(i, k), k = 0, 1, ... in ascending i; returns their number (the same in every lane).
template <class On, class Put>
__device__ __forceinline__ int wave_number(int c, On on, Put put) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    int k = 0;
    for (int base = 0; base < c; base += 64) {
        const int i = base + lane;
        const bool is = i < c && on(i);
        const unsigned long long mk = __ballot(is);
        if (is) put(i, k + __popcll(mk & below));
        k += __popcll(mk);
    }
    return k;
}

// ranks r < c with mask[r] == free, in ascending order -> list; returns their number (one wave, the same in every lane)
__device__ __forceinline__ int wave_compact(const int* mask, int free, int c, int* list) {
    return wave_number(c, [&](int r) { return mask[r] == free; }, [&](int r, int k) { list[k] = r; });
}

// a frame's clusters without a predecessor (gap[a] < 0, gap in LDS), numbered in rank order by wave 0: -> rank_out[a], their number -> *n_out
__device__ __forceinline__ void number_fresh(const int* gap, int ca, int* rank_out, int* n_out) {
    if (threadIdx.x < 64) {
        const int c = wave_number(ca, [&](int a) { return gap[a] < 0; }, [&](int a, int k) { rank_out[a] = k; });
        if (threadIdx.x == 0) *n_out = c;
    }
}

// node_track of a frame's detections from their cluster's rank and the frame's cluster tracks
template <int BLOCK>
__device__ __forceinline__ void write_node_tracks(const int* __restrict__ rank, int n, int ca, const long long* track, long long* __restrict__ node_track) {
    for (int v = threadIdx.x; v < n; v += BLOCK) {
        const int r = rank[v];
        node_track[v] = (r >= 0 && r < ca) ? track[r] : -1;
    }
}

// ---- the carried history state --------------------------------------------------------------------------------------------------------------
// GapHeader (64 bytes: next_id as an int64 at offset 0, the number of frames, reid_dim, the cluster count per frame), then for a total
// capacity of C rows: pos fp64 [C][2], with velocities vel fp64 [C][2], track int64 [C], emb fp32 [C][R], succ int32 [C] -- every 8-byte
// array before the 4-byte ones.  Frame f owns the rows off[f] .. off[f + 1], the running sum of the per-frame capacities the CALLER knows
// on the host (node counts bound cluster counts) and passes by value: nothing is read back to size anything.
struct GapHeader {
    long long next_id;
    int n_frames;
    int reid_dim;
    int count[kGapMaxFrames];
    int pad[3];
};
static_assert(sizeof(GapHeader) == 64, "the history state's arrays start at byte 64");

// the host-known row offsets of a state's frames: frame f owns rows off[f] .. off[f + 1] (off[n] = all rows)
struct GapFrames {
    int n;
    int off[kGapMaxFrames + 1];
};

// The KIND of a history state, wherever a `kind` is passed below (false / true of the two older kinds convert to 0 / 1): without
// velocities, with velocities, or the Kalman linker's -- the state with velocities whose pos and vel slots hold the FILTERED values, plus
// cov fp64 [C][3] behind vel and age int32 [C] behind succ (still every 8-byte array before the 4-byte ones).  The layouts of the two older
// kinds are as they were, byte for byte.
enum : int { kStatePlain = 0, kStateVel = 1, kStateKalman = 2 };

__host__ __device__ inline size_t hist_track_off(long long cap, int kind) {
    return sizeof(GapHeader) + (size_t)cap * (kind == kStateKalman ? 56 : kind == kStateVel ? 32 : 16);
}
__host__ __device__ inline size_t hist_emb_off(long long cap, int kind) { return hist_track_off(cap, kind) + (size_t)cap * 8; }
__host__ __device__ inline size_t hist_succ_off(long long cap, int R, int kind) {
    return hist_emb_off(cap, kind) + (size_t)cap * (size_t)R * sizeof(float);
}

// the arrays of a state of `cap` rows (Byte = char: a state to write; const char: one to read)
template <class Byte>
struct StateView {
    template <class T>
    using Ptr = std::conditional_t<std::is_const_v<Byte>, const T, T>*;
    Ptr<GapHeader> head;
    Ptr<double> pos, vel;   // vel: nullptr in a state without velocities
    Ptr<double> cov;        // nullptr except in a Kalman state
    Ptr<long long> track;
    Ptr<float> emb;
    Ptr<int> succ;
    Ptr<int> age;           // nullptr except in a Kalman state
    __device__ StateView(Byte* base, long long cap, int R, int kind)
        : head(reinterpret_cast<Ptr<GapHeader>>(base)), pos(reinterpret_cast<Ptr<double>>(base + sizeof(GapHeader))),
          vel(kind != kStatePlain ? pos + 2 * (size_t)cap : nullptr), cov(kind == kStateKalman ? pos + 4 * (size_t)cap : nullptr),
          track(reinterpret_cast<Ptr<long long>>(base + hist_track_off(cap, kind))),
          emb(reinterpret_cast<Ptr<float>>(base + hist_emb_off(cap, kind))),
          succ(reinterpret_cast<Ptr<int>>(base + hist_succ_off(cap, R, kind))), age(kind == kStateKalman ? succ + (size_t)cap : nullptr) {}
};

// cluster count of history frame f if the state holds one that fits its rows (0 otherwise: such a frame links to nothing)
__device__ __forceinline__ int hist_count(const char* state_in, int row0, int row1, int f, int P_lds) {
    const int c = reinterpret_cast<const GapHeader*>(state_in)->count[f];
    return (c >= 0 && c <= row1 - row0 && c <= P_lds) ? c : 0;
}

// Side B of level k for frame g: the clusters of frame s = g - 1 - k, a frame of the batch (s >= 0; its velocities at batch_vel, if any)
// or frame n_hist + s of the carried history (its row offsets at hist_off, which may be in LDS).  -> the side without its mask, its
// count 0 if there is no such frame or it is not usable; row: the COMBINED row of its rank 0 (history row i is i, batch row v is S + v).
__device__ __forceinline__ LinkSide side_b(int s, const int* __restrict__ node_ptr, int N_all, const int* __restrict__ count,
                                           const double* __restrict__ pos, const double* batch_vel, const float* __restrict__ emb, int R,
                                           const char* state_in, int n_hist, const int* hist_off, int S, int kind, int P_lds, int& row) {
    LinkSide b{nullptr, nullptr, nullptr, nullptr, 0, 0};
    row = 0;
    if (s >= 0) {
        int u0, m;
        if (frame_range(node_ptr, s, N_all, u0, m)) {
            b.n = usable_count(count, s, m, P_lds);
            b.pos = pos + 2 * (size_t)u0;
            b.vel = batch_vel ? batch_vel + 2 * (size_t)u0 : nullptr;
            b.emb = emb + (size_t)u0 * R;
            row = S + u0;
        }
    } else if (state_in && n_hist + s >= 0) {
        const int f = n_hist + s;
        row = __builtin_amdgcn_readfirstlane(hist_off[f]);   // (the same in every lane)
        b.n = hist_count(state_in, row, __builtin_amdgcn_readfirstlane(hist_off[f + 1]), f, P_lds);
        const StateView in(state_in, S, R, kind);
        b.pos = in.pos + 2 * (size_t)row;
        b.vel = kind != kStatePlain ? in.vel + 2 * (size_t)row : nullptr;
        b.emb = in.emb + (size_t)row * R;
    }
    return b;
}

// Time stamps (the _timed entries): frame_time is fp64 [history frames + G] over the COMBINED frame list, in units of the nominal frame
// period.  dt = T[t] - T[s] (one fp64 subtraction) stands where the untimed rule has (double)(k + 1); a table with
// !(dt > 0 && dt <= max_dt) has no admissible pair and is skipped whole -- which is also what a NaN or a disordered array gets.
// t, s: indices into the combined list, s >= 0 (the caller has found side B there).
__device__ __forceinline__ bool level_dt(const double* frame_time, int t, int s, double max_dt, double& dt) {
    dt = frame_time[t] - frame_time[s];
    return dt > 0.0 && dt <= max_dt;
}

// ---- the constant-velocity Kalman filter's arithmetic, written once: the smoother (identities_smooth.cuh) and the Kalman linker
// (identities_kalman.cuh) run these lines, one fp64 operation per operator as written, left to right, no FMA (fp contract is off) --------
// the predicted position variance after dt, from the covariance (a, b, c) = (var pos, cov pos/vel, var vel) and the process noise q
__device__ __forceinline__ double cv_predicted_var(double a, double b, double c, double dt, double q) {
    const double dt2 = dt * dt;
    const double dt3 = dt2 * dt;
    return ((a + (2.0 * dt) * b) + dt2 * c) + (q * dt3) / 3.0;
}

// One link: x = (px, py, vx, vy, a, b, c) of the predecessor becomes the linked cluster's, given its measurement (zx, zy), the elapsed
// time dt, the process noise q and the measurement variance re; -> nis.
__device__ __forceinline__ double cv_kalman_step(double (&x)[7], double zx, double zy, double dt, double q, double re) {
    const double dt2 = dt * dt;
    const double ppx = x[0] + dt * x[2];
    const double ppy = x[1] + dt * x[3];
    const double a_ = cv_predicted_var(x[4], x[5], x[6], dt, q);
    const double b_ = (x[5] + dt * x[6]) + (q * dt2) / 2.0;
    const double c_ = x[6] + q * dt;
    const double s = a_ + re;
    const double k1 = a_ / s, k2 = b_ / s;
    const double ix = zx - ppx, iy = zy - ppy;
    x[0] = ppx + k1 * ix, x[1] = ppy + k1 * iy;
    x[2] = x[2] + k2 * ix, x[3] = x[3] + k2 * iy;
    x[4] = a_ - k1 * a_, x[5] = b_ - k1 * b_, x[6] = c_ - k2 * b_;
    return (ix * ix + iy * iy) / s;
}

// c rows of one frame -> slot j of the new state, whose rows start at orow: count, pos, vel (where the state has them), track, succ, emb,
// and in a Kalman state (KALMAN) cov and age
template <int BLOCK, bool KALMAN = false>
__device__ void write_slot(const StateView<char>& out, int j, int orow, int c, int R, const double* __restrict__ pos, const double* __restrict__ vel,
                           const long long* track, const int* __restrict__ succ, const float* __restrict__ emb,
                           const double* __restrict__ cov = nullptr, const int* __restrict__ age = nullptr) {
    const int tid = threadIdx.x;
    if (tid == 0) out.head->count[j] = c;
    for (int i = tid; i < 2 * c; i += BLOCK) {
        out.pos[2 * (size_t)orow + i] = pos[i];
        if (out.vel) out.vel[2 * (size_t)orow + i] = vel[i];
    }
    for (int i = tid; i < c; i += BLOCK) {
        out.track[orow + i] = track[i];
        out.succ[orow + i] = succ[i];
    }
    if constexpr (KALMAN) {
        for (int i = tid; i < 3 * c; i += BLOCK) out.cov[3 * (size_t)orow + i] = cov[i];
        for (int i = tid; i < c; i += BLOCK) out.age[orow + i] = age[i];
    }
    for (size_t i = tid; i < (size_t)c * R; i += BLOCK) out.emb[(size_t)orow * R + i] = emb[i];
}

// Slot j of the new state when it is frame f of the OLD one (a history frame that stays): its rows as they are, the flags from the workspace.
template <int BLOCK, bool KALMAN = false>
__device__ void keep_slot(const StateView<char>& out, const GapFrames& of, int j, const char* state_in, const GapFrames& in, int f, int R,
                          int kind, const int* __restrict__ succ_ws, int P_lds) {
    const int orow = of.off[j], irow = in.off[f];
    int c = hist_count(state_in, irow, in.off[f + 1], f, P_lds);
    if (c > of.off[j + 1] - orow) c = 0;
    const StateView old(state_in, in.off[in.n], R, kind);
    write_slot<BLOCK, KALMAN>(out, j, orow, c, R, old.pos + 2 * (size_t)irow, kind != kStatePlain ? old.vel + 2 * (size_t)irow : nullptr,
                              old.track + irow, succ_ws + irow, old.emb + (size_t)irow * R, KALMAN ? old.cov + 3 * (size_t)irow : nullptr,
                              KALMAN ? old.age + irow : nullptr);
}

// ---- launch 1 of both history linkers: predecessor record (matched_prev, matched_gap) of the N batch rows = none, their velocity (if
// the linker has one) = 0; successor flags of the S history rows copied from the old state (never written), of the batch rows cleared.
// The flags live in the workspace as one array over the COMBINED rows.
__global__ __launch_bounds__(256) void link_init_kernel(const int* __restrict__ in_succ, int S, int N_all, int* __restrict__ succ_ws,
                                                        int* __restrict__ matched_prev, int* __restrict__ matched_gap,
                                                        double* __restrict__ velocity) {
    const long long total = (long long)S + N_all;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (i < S) {
            succ_ws[i] = in_succ[i] != 0;
        } else {
            succ_ws[i] = 0;
            matched_prev[i - S] = -1;
            matched_gap[i - S] = -1;
            if (velocity) velocity[2 * (i - S)] = 0.0, velocity[2 * (i - S) + 1] = 0.0;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
// the rule's numbers as every entry takes them -> are they valid; then `rule` holds them
static bool link_rule(double max_step, double lam, int32_t has_max_cos, double max_cos, LinkRule& rule) {
    if (!(max_step > 0.0) || !(max_step < __builtin_inf()) || !(lam >= 0.0) || !(lam < __builtin_inf())) return false;
    if (has_max_cos && !(max_cos >= 0.0 && max_cos <= 2.0)) return false;
    rule.max_step = max_step, rule.lam = lam, rule.max_cos = max_cos;
    rule.has_max_cos = has_max_cos != 0;
    rule.need_emb = lam != 0.0 || has_max_cos != 0;
    return true;
}

// rows[0 .. n) -> running offsets; false if a frame is negative or above the per-frame limit
static bool gap_frames(const int32_t* rows, int n, GapFrames& f) {
    f.n = n;
    f.off[0] = 0;
    for (int i = 0; i < kGapMaxFrames; ++i) {
        int r = 0;
        if (i < n) {
            r = rows[i];
            if (r < 0 || r > kTrackMaxNodes) return false;
        }
        f.off[i + 1] = f.off[i] + r;
    }
    return true;
}

// what a history entry (gnncca_link_frames_gap / _gap_ex / _motion and their _timed forms) works out before its first launch
struct HistoryPlan {
    bool nothing;          // n_frames == 0: no time passes, the caller keeps its state
    GapFrames in, out;     // the row offsets of the old and of the new state
    LinkRule rule;
    int R, S, P;           // appearance columns the rule reads; rows of the old state; LDS entries per frame array
    int carried;           // history frames that stay in the new state
    unsigned init_blocks;
    const char* sin;       // the old state, nullptr if it holds no frame
};

// The refusals of the history entries in their fixed order -- every one of them before any dereference of a device pointer and before
// any launch -- then the plan.  outputs: does the caller have every per-row array a batch with rows needs; ws_bytes: the entry's own
// workspace size; matching: the table of a frame pair lives in LDS.
static int plan_history(int64_t n_nodes, int32_t n_frames, int32_t reid_dim, int32_t max_frame_nodes, double max_step, double lam,
                        int32_t has_max_cos, double max_cos, int32_t max_gap, int32_t matching, const void* state_in,
                        const int32_t* state_in_frame_rows, int32_t state_in_frames, const void* state_out,
                        const int32_t* state_out_frame_rows, int32_t state_out_frames, const void* node_ptr_dev, const void* count,
                        const void* emb, bool outputs, const void* workspace, size_t workspace_bytes,
                        size_t (*ws_bytes)(int64_t, int64_t, int64_t), HistoryPlan& p) {
    p.nothing = false;
    if (n_nodes < 0 || n_frames < 0 || reid_dim < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_gap < 0 || max_gap > kTrackMaxGap) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kTrackMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (state_in_frames < 0 || state_in_frames > max_gap + 1 || (state_in_frames > 0 && (!state_in || !state_in_frame_rows)))
        return GNNCCA_ERR_INVALID_ARG;
    if (!gap_frames(state_in_frame_rows, state_in ? state_in_frames : 0, p.in)) return GNNCCA_ERR_INVALID_ARG;   // a history frame above the limit
    if (matching) {   // before any launch, for the batch and for the carried history alike
        if (max_frame_nodes > kTrackMaxOptimalNodes) return GNNCCA_ERR_INVALID_ARG;
        for (int f = 0; f < p.in.n; ++f)
            if (p.in.off[f + 1] - p.in.off[f] > kTrackMaxOptimalNodes) return GNNCCA_ERR_INVALID_ARG;
    }
    if (!link_rule(max_step, lam, has_max_cos, max_cos, p.rule)) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) {
        p.nothing = true;
        return GNNCCA_OK;
    }
    const long long seen = (long long)p.in.n + n_frames;
    const int kept = (int)(seen < max_gap + 1 ? seen : max_gap + 1);
    if (state_out_frames != kept || !state_out_frame_rows || !gap_frames(state_out_frame_rows, kept, p.out)) return GNNCCA_ERR_INVALID_ARG;
    if (!node_ptr_dev || !count || !state_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && !outputs) return GNNCCA_ERR_INVALID_ARG;
    // R is the rule's, not this batch's: a batch without rows (emb may then be NULL) must still carry the history's appearance rows along
    p.R = p.rule.need_emb ? (int)reid_dim : 0;
    if (p.R > 0 && n_nodes > 0 && !emb) return GNNCCA_ERR_INVALID_ARG;
    p.S = p.in.off[p.in.n];
    if (workspace_bytes < ws_bytes(n_nodes, n_frames, p.S)) return GNNCCA_ERR_WORKSPACE;
    if (n_nodes >= (1ll << 31) - 64 - p.S) return GNNCCA_ERR_UNSUPPORTED;
    p.P = 64;
    while (p.P < max_frame_nodes) p.P <<= 1;
    for (int f = 0; f < p.in.n; ++f)
        while (p.P < p.in.off[f + 1] - p.in.off[f]) p.P <<= 1;
    p.carried = kept > n_frames ? kept - n_frames : 0;
    p.sin = p.in.n ? static_cast<const char*>(state_in) : nullptr;
    const long long cells = (long long)p.S + n_nodes;
    p.init_blocks = (unsigned)(cells <= 0 ? 1 : (cells + 255) / 256 > 1024 ? 1024 : (cells + 255) / 256);
    return GNNCCA_OK;
}

// launch 1 of a history entry (velocity: nullptr for a linker without one)
static void launch_link_init(hipStream_t st, const HistoryPlan& p, int kind, int64_t n_nodes, int* succ_ws, int* matched_prev,
                             int* matched_gap, double* velocity) {
    const int* in_succ = p.sin ? reinterpret_cast<const int*>(p.sin + hist_succ_off(p.S, p.R, kind)) : nullptr;
    hipLaunchKernelGGL(link_init_kernel, dim3(p.init_blocks), dim3(256), 0, st, in_succ, p.S, (int)n_nodes, succ_ws, matched_prev, matched_gap,
                       velocity);
}

}  // namespace gnncca
