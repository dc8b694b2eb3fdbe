// identities_smooth.cuh -- a constant-velocity Kalman filter along every track (gnncca_track_smooth), included at the end of identities.hip
// after the linkers and the re-entry gallery: a stage BEHIND the linkers that turns their links into trajectories -- filtered position,
// velocity, covariance, how far a detection lay from where its track was expected (nis) and the links since birth (age).  It decides
// nothing: matched_prev / matched_gap are inputs.  frame_range, usable_count, GapFrames / gap_frames, round256 and the combined-row
// convention (history row i is i, batch row v is S + v) are the linkers', shared through identities.hip / link_common.cuh.
//
// The rule (include/gnncca_mpn.h has it in full, tests/track_smooth_oracle.py as loops).  Two independent ground-plane axes share one
// 2 x 2 covariance (a, b, c) = (var pos, cov pos/vel, var vel); re = r, or r / (double)size with per_detection.  For cluster a of frame t
// with measurement z = pos(a):
//   Birth (matched_gap(a) == -1):  p = z, v = (0, 0), (a, b, c) = (re, 0, vel_var), age = 0, nis = 0.
//   Link to cluster m = matched_prev(a) of frame t - 1 - k, k = matched_gap(a):  dt = (double)(k + 1), or T[t] - T[t - 1 - k] with time
//   stamps (frames counted among frames present); from that cluster's filtered state, one fp64 operation per operator as written, left
//   to right, no FMA (this translation unit is compiled with fp contract(off)):
//     dt2 = dt*dt;  dt3 = dt2*dt
//     pp  = p + dt*v                               (per axis)
//     a_  = ((a + (2.0*dt)*b) + dt2*c) + (q*dt3)/3.0
//     b_  = (b + dt*c) + (q*dt2)/2.0
//     c_  = c + q*dt
//     s   = a_ + re
//     k1  = a_/s;  k2 = b_/s
//     i   = z - pp                                 (per axis)
//     p'  = pp + k1*i;  v' = v + k2*i              (per axis)
//     a'  = a_ - k1*a_;  b' = b_ - k1*b_;  c' = c_ - k2*b_
//     nis = (ix*ix + iy*iy)/s
//     age' = age + 1
//   Non-finite inputs propagate.  Rows at or beyond a frame's count, and every row of a refused frame, are zero with age = -1.
// Tracks are independent and a track is a chain of predecessor links, so the work is chain-parallel.  Three launches, kernels only,
// whatever max_gap and G are:
//   1. smooth_init_kernel: the successor row of every combined row (S history rows + N batch rows), and the frame and the new-state row of
//      every batch row = -1.  A kernel and not a hipMemsetAsync, so that a captured call holds kernel nodes only (DESIGN.md section 9 has
//      why); and every index the walk takes from the workspace is checked against its own range: no bound rests on what it holds.
//   2. smooth_succ_kernel (a workgroup per frame): every batch row learns its frame and, if the new state keeps that frame, its row
//      there; a usable cluster with a valid predecessor writes its own combined row into the predecessor's slot.  Links are one-to-one,
//      so these are plain stores: no atomics.
//   3. smooth_walk_kernel (a thread per combined row).  A row beyond its frame's count writes its zeros.  A chain HEAD -- a usable batch
//      cluster that is not its predecessor's recorded successor (a birth, or the loser of a malformed many-to-one input), or a history
//      row whose successor is in the batch -- walks forward along the successor array, at most G steps (every step moves to a later
//      frame of the batch: the loop is bounded by G, not by data), applies the rule, writes the five outputs and, for a frame the new
//      state keeps, the row of the new state.  A step waits for two memory round trips, three with time stamps: the successor, then
//      everything about it at once -- launch 2 recorded a successor only where the link is valid, so the walk does not look it up
//      again.  A history row that stays (G < max_gap + 1) is copied to its new slot.  Thread 0 writes the header.  Every batch row is
//      written exactly once, by its own thread or by the head of its chain.
// No workgroup waits for another, nothing is read back, no cooperative launch: capturable.  The serial depth is the longest chain, paid
// once for all chains side by side.
// State: SmoothHeader (64 bytes: the number of frames, the usable cluster count per frame), then for a capacity of C rows fp64 [C][7]
// (px, py, vx, vy, a, b, c), then int32 age [C] (-1: not a cluster) -- the 8-byte array before the 4-byte one.  The rows are aligned with
// the linker's kept frames: the last max_gap + 1 frames, frame f owning rows off[f] .. off[f + 1] of the host-known capacities.
#pragma once

namespace gnncca {

struct SmoothHeader {
    int n_frames;
    int count[kGapMaxFrames];
    int pad[6];
};
static_assert(sizeof(SmoothHeader) == 64, "the smoother state's arrays start at byte 64");

__host__ __device__ inline size_t smooth_age_off(long long cap) { return sizeof(SmoothHeader) + (size_t)cap * 56; }

struct SmoothParams {
    double q, r, vel_var;
    int per_detection;
};

// everything the two kernels need to find a row's predecessor; the arrays of the old state start at state_in (nullptr: no history)
struct SmoothIn {
    const int* node_ptr;
    const int* count;
    const int* matched_prev;
    const int* matched_gap;
    const char* state_in;
    int N_all, G, max_gap, P_lds, S;
    GapFrames in;
};

// usable cluster count of history frame f of a smoother state (0 if it does not fit its rows)
__device__ __forceinline__ int smooth_hist_count(const SmoothIn& si, int f) {
    const int c = reinterpret_cast<const SmoothHeader*>(si.state_in)->count[f];
    return (c >= 0 && c <= si.in.off[f + 1] - si.in.off[f]) ? c : 0;
}

// The COMBINED row of the predecessor of batch row `row` = rank a (a usable cluster) of frame t, or -1: no link, or one that points at
// nothing (a level outside 0 .. max_gap, a frame before the history, a rank at or beyond that frame's count).
__device__ __forceinline__ int smooth_pred_row(const SmoothIn& si, int t, int row) {
    const int k = si.matched_gap[row], m = si.matched_prev[row];
    if (k < 0 || k > si.max_gap || m < 0) return -1;
    const int s = t - 1 - k;
    if (s >= 0) {
        int u0, n;
        if (!frame_range(si.node_ptr, s, si.N_all, u0, n)) return -1;
        return m < usable_count(si.count, s, n, si.P_lds) ? si.S + u0 + m : -1;
    }
    const int f = si.in.n + s;
    if (!si.state_in || f < 0) return -1;
    return m < smooth_hist_count(si, f) ? si.in.off[f] + m : -1;
}

// ---- launch 1 -----------------------------------------------------------------------------------------------------------------------------
// the workspace's three arrays = -1 (a kernel, not a memset: see the head of the file)
__global__ __launch_bounds__(256) void smooth_init_kernel(int* __restrict__ ws, long long cells) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long long)gridDim.x * 256) ws[i] = -1;
}

// ---- launch 2 -----------------------------------------------------------------------------------------------------------------------------
// succ: int32 [S + N] over the combined rows; row_frame, row_slot: int32 [N] (a batch row's frame, and its row in the new state if the
// new state keeps its frame); all -1 from launch 1.  succ[p] = r is written only where p is the valid predecessor of the usable
// cluster r: the walk below follows it without looking r's predecessor up again.
__global__ __launch_bounds__(256) void smooth_succ_kernel(SmoothIn si, GapFrames out, int* __restrict__ succ, int* __restrict__ row_frame,
                                                          int* __restrict__ row_slot) {
    const int t = blockIdx.x;
    int v0, n;
    // A frame whose node_ptr range is invalid owns no row: if the new state keeps it, its header count is 0 (so nobody reads its rows
    // as clusters) and its rows there stay as the caller allocated them -- the one case where the state is not the oracle's image.
    if (!frame_range(si.node_ptr, t, si.N_all, v0, n)) return;
    const int ca = usable_count(si.count, t, n, si.P_lds);
    const int j = t - (si.G - out.n);   // the slot of frame t in the new state
    const int cap = j >= 0 ? out.off[j + 1] - out.off[j] : 0;
    for (int a = threadIdx.x; a < n; a += 256) {
        row_frame[v0 + a] = t;
        if (a < cap) row_slot[v0 + a] = out.off[j] + a;
        if (a >= ca) continue;
        const int p = smooth_pred_row(si, t, v0 + a);
        if (p >= 0) succ[p] = si.S + v0 + a;
    }
}

// ---- launch 3 -----------------------------------------------------------------------------------------------------------------------------
struct SmoothOut {
    double* pos;
    double* vel;
    double* cov;
    double* nis;
    int* age;
    char* state_out;
    GapFrames out;
};

// a filtered state -> row orow of the new state
__device__ __forceinline__ void smooth_keep(const SmoothOut& so, int orow, const double (&x)[7], int age) {
    double* sx = reinterpret_cast<double*>(so.state_out + sizeof(SmoothHeader)) + 7 * (size_t)orow;
#pragma unroll
    for (int i = 0; i < 7; ++i) sx[i] = x[i];
    reinterpret_cast<int*>(so.state_out + smooth_age_off(so.out.off[so.out.n]))[orow] = age;
}

// batch row `row` -> the five outputs and, if the new state keeps its frame (orow >= 0), its row there.  orow comes from the workspace:
// it is used only inside the new state's rows, whatever the workspace holds.
__device__ __forceinline__ void smooth_write(const SmoothOut& so, int row, int orow, const double (&x)[7], double nis, int age) {
    so.pos[2 * (size_t)row] = x[0], so.pos[2 * (size_t)row + 1] = x[1];
    so.vel[2 * (size_t)row] = x[2], so.vel[2 * (size_t)row + 1] = x[3];
    so.cov[3 * (size_t)row] = x[4], so.cov[3 * (size_t)row + 1] = x[5], so.cov[3 * (size_t)row + 2] = x[6];
    so.nis[row] = nis;
    so.age[row] = age;
    if (orow >= 0 && orow < so.out.off[so.out.n]) smooth_keep(so, orow, x, age);
}

__global__ __launch_bounds__(256) void smooth_walk_kernel(SmoothIn si, const int* __restrict__ size, const double* __restrict__ pos,
                                                          const int* __restrict__ succ, const int* __restrict__ row_frame,
                                                          const int* __restrict__ row_slot, SmoothParams prm,
                                                          const double* __restrict__ frame_time, SmoothOut so) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int S = si.S, HN = si.in.n, G = si.G;
    const int first_kept = G - so.out.n;   // the batch frame that becomes slot 0 of the new state (negative: history frames stay)
    if (gid == 0) {   // the header of the new state
        SmoothHeader* h = reinterpret_cast<SmoothHeader*>(so.state_out);
        h->n_frames = so.out.n;
        for (int j = 0; j < kGapMaxFrames; ++j) {
            int c = 0;
            const int g = first_kept + j;
            if (j < so.out.n && g >= 0) {
                int v0, n;
                if (frame_range(si.node_ptr, g, si.N_all, v0, n)) c = usable_count(si.count, g, n, si.P_lds);
                if (c > so.out.off[j + 1] - so.out.off[j]) c = 0;   // (a frame with more clusters than its slot has rows is carried as empty)
            } else if (j < so.out.n && HN + g >= 0) {
                c = smooth_hist_count(si, HN + g);
            }
            h->count[j] = c;
        }
        for (int j = 0; j < 6; ++j) h->pad[j] = 0;
    }
    if (gid >= (long long)S + si.N_all) return;
    const int me = (int)gid;
    double x[7];
    int age;
    if (me < S) {   // a history row: it moves to its new slot if its frame stays, and heads a chain if its successor is in the batch
        int f = 0;
        for (int j = 1; j < kGapMaxFrames; ++j) f += (j < HN && me >= si.in.off[j]);
        const double* ix = reinterpret_cast<const double*>(si.state_in + sizeof(SmoothHeader)) + 7 * (size_t)me;
#pragma unroll
        for (int i = 0; i < 7; ++i) x[i] = ix[i];
        age = reinterpret_cast<const int*>(si.state_in + smooth_age_off(S))[me];
        const int j = f - HN - first_kept, a = me - si.in.off[f];
        if (j >= 0 && a < so.out.off[j + 1] - so.out.off[j]) smooth_keep(so, so.out.off[j] + a, x, age);
        if (succ[me] < S || age < 0) return;
    } else {
        const int row = me - S;
        const int t = row_frame[row], orow = row_slot[row];
        int v0 = 0, n = 0;
        const bool ok = t >= 0 && t < G && frame_range(si.node_ptr, t, si.N_all, v0, n);
        const int a = row - v0;
        if (!ok || a < 0 || a >= usable_count(si.count, t, n, si.P_lds)) {   // not a cluster (or a row no frame owns): zeros, age -1
            const double zero[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            smooth_write(so, row, orow, zero, 0.0, -1);
            return;
        }
        const int p = smooth_pred_row(si, t, row);
        if (p >= 0 && succ[p] == me) return;   // its chain's head writes this row
        const double re = prm.per_detection ? prm.r / (double)size[row] : prm.r;
        x[0] = pos[2 * (size_t)row], x[1] = pos[2 * (size_t)row + 1], x[2] = 0.0, x[3] = 0.0, x[4] = re, x[5] = 0.0, x[6] = prm.vel_var;
        age = 0;
        smooth_write(so, row, orow, x, 0.0, 0);
    }
    // Forward along the chain: every step lands in a later frame of the batch, so G steps are enough.  A step's chain of dependent
    // loads is succ[cur], then the row's frame, slot, level, size and position together (then, with time stamps, the two times).
    int cur = me;
    for (int step = 0; step < G; ++step) {
        const int nxt = succ[cur];
        if (nxt < S || nxt >= S + si.N_all) return;
        const int row = nxt - S;
        const int tn = row_frame[row], orow = row_slot[row], k = si.matched_gap[row];
        const double zx = pos[2 * (size_t)row], zy = pos[2 * (size_t)row + 1];
        const double re = prm.per_detection ? prm.r / (double)size[row] : prm.r;
        // launch 2 recorded this successor, so 0 <= k <= max_gap, 0 <= tn < G and frame tn - 1 - k is in the combined list; the walk
        // checks it all the same (registers only): no index below rests on what the workspace holds
        if (tn < 0 || tn >= G || k < 0 || k > si.max_gap || HN + tn - 1 - k < 0) return;
        const double dt = frame_time ? frame_time[HN + tn] - frame_time[HN + tn - 1 - k] : (double)(k + 1);
        const double nis = cv_kalman_step(x, zx, zy, dt, prm.q, re);   // (the rule's lines: link_common.cuh)
        age = age + 1;
        smooth_write(so, row, orow, x, nis, age);
        cur = nxt;
    }
}

}  // namespace gnncca

extern "C" {

size_t gnncca_track_smooth_state_bytes(int64_t capacity_rows, int32_t n_frames_kept) {
    if (capacity_rows < 0 || n_frames_kept < 0 || n_frames_kept > gnncca::kGapMaxFrames) return 0;
    return gnncca::round256(gnncca::smooth_age_off(capacity_rows) + (size_t)capacity_rows * sizeof(int32_t));
}

size_t gnncca_track_smooth_workspace_bytes(int64_t n_nodes, int64_t n_frames, int64_t state_rows) {
    if (n_nodes < 0 || n_frames < 0 || state_rows < 0) return 0;
    return gnncca::round256(((size_t)state_rows + 3 * (size_t)n_nodes) * sizeof(int32_t));   // successor rows [S + N]; frame, new-state row of a row [N]
}

int gnncca_track_smooth(const int32_t* node_ptr_dev, const int32_t* count, const int32_t* size, const double* pos, const int32_t* matched_prev,
                        const int32_t* matched_gap, int64_t n_nodes, int32_t n_frames, int32_t max_frame_nodes, int32_t max_gap, double q,
                        double r, double vel_var, int32_t per_detection, const void* state_in, const int32_t* state_in_frame_rows,
                        int32_t state_in_frames, void* state_out, const int32_t* state_out_frame_rows, int32_t state_out_frames,
                        double* out_pos, double* out_vel, double* out_cov, double* out_nis, int32_t* out_age, void* workspace,
                        size_t workspace_bytes, gnncca_stream_t stream, const double* frame_time_dev, double max_dt) {
    using namespace gnncca;
    const double inf = __builtin_inf();
    if (n_nodes < 0 || n_frames < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_gap < 0 || max_gap > kTrackMaxGap) return GNNCCA_ERR_INVALID_ARG;
    if (max_frame_nodes < 0 || max_frame_nodes > kTrackMaxNodes || max_frame_nodes > n_nodes) return GNNCCA_ERR_INVALID_ARG;
    if (!(q >= 0.0) || !(q < inf) || !(r > 0.0) || !(r < inf) || !(vel_var > 0.0) || !(vel_var < inf)) return GNNCCA_ERR_INVALID_ARG;
    if (per_detection != 0 && per_detection != 1) return GNNCCA_ERR_INVALID_ARG;
    if (frame_time_dev && (!(max_dt > 0.0) || !(max_dt < inf))) return GNNCCA_ERR_INVALID_ARG;
    if (state_in_frames < 0 || state_in_frames > max_gap + 1 || (state_in_frames > 0 && (!state_in || !state_in_frame_rows)))
        return GNNCCA_ERR_INVALID_ARG;
    SmoothIn si;
    SmoothOut so;
    if (!gap_frames(state_in_frame_rows, state_in ? state_in_frames : 0, si.in)) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0) return GNNCCA_OK;   // no time passes: the caller keeps its state
    const long long seen = (long long)si.in.n + n_frames;
    const int kept = (int)(seen < max_gap + 1 ? seen : max_gap + 1);
    if (state_out_frames != kept || !state_out_frame_rows || !gap_frames(state_out_frame_rows, kept, so.out)) return GNNCCA_ERR_INVALID_ARG;
    const int carried = kept > n_frames ? kept - n_frames : 0;
    for (int j = 0; j < carried; ++j)   // a history frame that stays keeps its rows
        if (state_out_frame_rows[j] != state_in_frame_rows[si.in.n - carried + j]) return GNNCCA_ERR_INVALID_ARG;
    if (!node_ptr_dev || !count || !state_out || !workspace) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes > 0 && (!size || !pos || !matched_prev || !matched_gap || !out_pos || !out_vel || !out_cov || !out_nis || !out_age))
        return GNNCCA_ERR_INVALID_ARG;
    si.S = si.in.off[si.in.n];
    if (workspace_bytes < gnncca_track_smooth_workspace_bytes(n_nodes, n_frames, si.S)) return GNNCCA_ERR_WORKSPACE;
    if (n_nodes >= (1ll << 31) - 256 - si.S) return GNNCCA_ERR_UNSUPPORTED;
    si.P_lds = 64;
    while (si.P_lds < max_frame_nodes) si.P_lds <<= 1;
    si.node_ptr = node_ptr_dev, si.count = count, si.matched_prev = matched_prev, si.matched_gap = matched_gap;
    si.state_in = si.in.n ? static_cast<const char*>(state_in) : nullptr;
    si.N_all = (int)n_nodes, si.G = (int)n_frames, si.max_gap = (int)max_gap;
    so.pos = out_pos, so.vel = out_vel, so.cov = out_cov, so.nis = out_nis, so.age = out_age;
    so.state_out = static_cast<char*>(state_out);
    const SmoothParams prm{q, r, vel_var, (int)per_detection};
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* succ = static_cast<int*>(workspace);
    int* row_frame = succ + si.S + n_nodes;
    int* row_slot = row_frame + n_nodes;
    const long long cells = (long long)si.S + n_nodes;
    const long long ws_cells = (long long)si.S + 3 * n_nodes;
    if (ws_cells > 0) {
        hipLaunchKernelGGL(smooth_init_kernel, dim3((unsigned)((ws_cells + 255) / 256 > 1024 ? 1024 : (ws_cells + 255) / 256)), dim3(256), 0, st, succ,
                           ws_cells);
        HIP_TRY(hipGetLastError());
    }
    if (n_nodes > 0) {   // (a batch without rows has no link: the walk below only moves the history to its new slots)
        hipLaunchKernelGGL(smooth_succ_kernel, dim3((unsigned)n_frames), dim3(256), 0, st, si, so.out, succ, row_frame, row_slot);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(smooth_walk_kernel, dim3((unsigned)(cells <= 0 ? 1 : (cells + 255) / 256)), dim3(256), 0, st, si, size, pos, succ, row_frame,
                       row_slot, prm, frame_time_dev, so);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
