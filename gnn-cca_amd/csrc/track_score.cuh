// track_score.cuh -- identity-tracking scores accumulated on the device (gnncca_track_score_*), included at the end of identities.hip.  It
// joins the caller's person ids, the cameras and a linker's node tracks over the frames of a sequence; nothing above is touched.
//
// The rule (include/gnncca_mpn.h has it in full): a detection is VALID iff 0 <= id < max_ids, 0 <= cam < max_cams and 0 <= track < 2^40;
// it is SCORED iff no valid detection of its frame with a larger node id has the same (id, cam); a scored detection is a SWITCH iff the
// latest earlier scored detection of its stream k = id * max_cams + cam (however many frames or calls back) had another track; and n[p][t]
// counts the scored detections of person p with track t.
// The state: one int64 buffer [8 + 2 cap] = { header: scored, ignored, switches, pairs, overflow, 3 unused | keys [cap] | counts [cap] } --
// an open-addressing table, cap a power of two, key = p << 40 | t, all ones = empty, linear probing -- and last int64 [K], the last track
// of every stream (-1: none yet).  One buffer, so that the host reads everything it needs in ONE copy.
// An add call, three launches and a memset:
//   0. the slot image int32 [G][K] is cleared;
//   1. score_scatter_kernel, one thread per detection: switched = -1; a valid one finds its frame (binary search in node_ptr, at most 32
//      steps) and raises slot[f][k] to node + 1 with an integer atomicMax -- the winner is the largest node id whatever the arrival order;
//   2. score_walk_kernel, one thread per stream: frames in order (adjacent threads read adjacent slots: coalesced), from last[k]; every
//      winner is compared with the track before it and gets its switched flag from the one thread that owns it; runs of equal track go to
//      the table as ONE add (atomicCAS on the key, atomicAdd on the count); last[k] is written back; the counters are summed per wave
//      (shuffles), per workgroup (LDS) and then take one integer atomic per workgroup and counter.
// All atomics are integer and device scope: every number is reproducible, only the slot a pair lands in is not.  Every loop is bounded at
// launch: the probe gives up after cap steps, sets the overflow word and drops the run (the caller sizes cap >= 2 x the detections seen,
// and pairs <= detections, so this cannot happen; the guard is there so that a wrong size can never spin).
// gnncca_track_score_rehash re-inserts the cells of a table into a larger one (memset, header copy, one launch).
#pragma once

namespace gnncca {

constexpr int kScoreHeaderLen = GNNCCA_SCORE_HEADER_LEN;
constexpr unsigned long long kScoreEmpty = ~0ull;
constexpr int kScoreTrackBits = 40;
enum { kScScored = 0, kScIgnored = 1, kScSwitches = 2, kScPairs = 3, kScOverflow = 4 };

static bool score_cap_ok(int64_t cap) { return cap >= GNNCCA_SCORE_MIN_CAP && cap <= (1ll << 40) && (cap & (cap - 1)) == 0; }

__device__ __forceinline__ unsigned long long score_hash(unsigned long long x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// count += add at the cell of `key`; true if the key is new.  At most cap probes: a full table sets the overflow word and drops the add.
__device__ __forceinline__ bool score_insert(unsigned long long* header, unsigned long long* keys, unsigned long long* counts,
                                             unsigned long long cap, unsigned long long key, unsigned long long add) {
    const unsigned long long mask = cap - 1;
    unsigned long long h = score_hash(key) & mask;
    for (unsigned long long step = 0; step < cap; ++step) {
        unsigned long long seen = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == kScoreEmpty) seen = atomicCAS(&keys[h], kScoreEmpty, key);
        if (seen == kScoreEmpty || seen == key) {
            atomicAdd(&counts[h], add);
            return seen == kScoreEmpty;
        }
        h = (h + 1) & mask;
    }
    atomicMax(&header[kScOverflow], 1ull);
    return false;
}

__global__ __launch_bounds__(256) void score_scatter_kernel(const long long* __restrict__ ids, const int* __restrict__ cam,
                                                            const long long* __restrict__ node_track, const int* __restrict__ node_ptr,
                                                            long long node_base, int N, int G, int max_ids, int max_cams, int K,
                                                            int* __restrict__ slot, int* __restrict__ switched) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    switched[i] = -1;
    const long long p = ids[i], t = node_track[i];
    const int c = cam[i];
    if (p < 0 || p >= max_ids || c < 0 || c >= max_cams || t < 0 || t >= (1ll << kScoreTrackBits)) return;
    int lo = 0, hi = G - 1;   // the last frame that starts at or before node i; lo and hi stay inside [0, G) whatever node_ptr holds
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)node_ptr[mid] - node_base <= i) lo = mid;
        else hi = mid - 1;
    }
    atomicMax(&slot[(size_t)lo * K + (size_t)((int)p * max_cams + c)], i + 1);
}

__global__ __launch_bounds__(256) void score_walk_kernel(const long long* __restrict__ node_track, int N, int G, int max_cams, int K,
                                                         const int* __restrict__ slot, unsigned long long* header, unsigned long long cap,
                                                         long long* __restrict__ last, int* __restrict__ switched) {
    __shared__ int s_sum[3];
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long* keys = header + kScoreHeaderLen;
    unsigned long long* counts = keys + cap;
    int scored = 0, switches = 0, pairs = 0;
    if (k < K) {
        const unsigned long long p = (unsigned long long)(k / max_cams);
        long long cur = last[k], run_t = -1;
        unsigned long long run_len = 0;
        for (int f0 = 0; f0 < G; f0 += 8) {
            int w[8];
            long long t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = f0 + j < G ? slot[(size_t)(f0 + j) * K + k] : 0;   // (the loads go out before the first use)
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = (w[j] > 0 && w[j] <= N) ? node_track[w[j] - 1] : -1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (t[j] < 0) continue;   // (no winner in this frame; a winner's track is >= 0: the scatter checked it)
                const int sw = cur >= 0 && cur != t[j];
                switched[w[j] - 1] = sw;
                ++scored;
                switches += sw;
                if (run_len > 0 && run_t != t[j]) {
                    pairs += score_insert(header, keys, counts, cap, p << kScoreTrackBits | (unsigned long long)run_t, run_len);
                    run_len = 0;
                }
                run_t = cur = t[j];
                ++run_len;
            }
        }
        if (run_len > 0) pairs += score_insert(header, keys, counts, cap, p << kScoreTrackBits | (unsigned long long)run_t, run_len);
        last[k] = cur;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        scored += __shfl_xor(scored, o);
        switches += __shfl_xor(switches, o);
        pairs += __shfl_xor(pairs, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (scored) atomicAdd(&s_sum[0], scored);
        if (switches) atomicAdd(&s_sum[1], switches);
        if (pairs) atomicAdd(&s_sum[2], pairs);
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // one atomic per workgroup and counter; `ignored` is N minus the scored ones (two's complement: the sum is exact)
        const int sc = s_sum[0], sw = s_sum[1], pr = s_sum[2];
        if (sc) atomicAdd(&header[kScScored], (unsigned long long)sc);
        const long long ign = (blockIdx.x == 0 ? (long long)N : 0ll) - sc;
        if (ign) atomicAdd(&header[kScIgnored], (unsigned long long)ign);
        if (sw) atomicAdd(&header[kScSwitches], (unsigned long long)sw);
        if (pr) atomicAdd(&header[kScPairs], (unsigned long long)pr);
    }
}

__global__ __launch_bounds__(256) void score_rehash_kernel(const unsigned long long* __restrict__ in, unsigned long long cap_in,
                                                           unsigned long long* out, unsigned long long cap_out) {
    const unsigned long long* in_keys = in + kScoreHeaderLen;
    const unsigned long long* in_counts = in_keys + cap_in;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < cap_in; i += (unsigned long long)gridDim.x * 256) {
        const unsigned long long key = in_keys[i];
        if (key != kScoreEmpty) score_insert(out, out + kScoreHeaderLen, out + kScoreHeaderLen + cap_out, cap_out, key, in_counts[i]);
    }
}

}  // namespace gnncca

extern "C" {

size_t gnncca_track_score_table_bytes(int64_t cap) {
    if (!gnncca::score_cap_ok(cap)) return 0;
    return ((size_t)gnncca::kScoreHeaderLen + 2 * (size_t)cap) * sizeof(int64_t);
}

int gnncca_track_score_reset(void* table, int64_t cap, int64_t* last, int64_t n_streams, gnncca_stream_t stream) {
    using namespace gnncca;
    if (!table || !last || !score_cap_ok(cap) || n_streams < 1 || n_streams > GNNCCA_SCORE_MAX_STREAMS) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(table);
    const size_t head = (size_t)kScoreHeaderLen * 8, cells = (size_t)cap * 8;
    HIP_TRY(hipMemsetAsync(base, 0, head, st));
    HIP_TRY(hipMemsetAsync(base + head, 0xFF, cells, st));           // keys: empty
    HIP_TRY(hipMemsetAsync(base + head + cells, 0, cells, st));      // counts
    HIP_TRY(hipMemsetAsync(last, 0xFF, (size_t)n_streams * 8, st));  // -1: the stream has not been seen
    return GNNCCA_OK;
}

int gnncca_track_score_rehash(const void* table_in, int64_t cap_in, void* table_out, int64_t cap_out, gnncca_stream_t stream) {
    using namespace gnncca;
    if (!table_in || !table_out || table_in == table_out || !score_cap_ok(cap_in) || !score_cap_ok(cap_out) || cap_out < cap_in)
        return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(table_out);
    const size_t head = (size_t)kScoreHeaderLen * 8, cells = (size_t)cap_out * 8;
    HIP_TRY(hipMemcpyAsync(base, table_in, head, hipMemcpyDeviceToDevice, st));   // the counters carry over; `pairs` does not change
    HIP_TRY(hipMemsetAsync(base + head, 0xFF, cells, st));
    HIP_TRY(hipMemsetAsync(base + head + cells, 0, cells, st));
    const long long blocks = (cap_in + 255) / 256;
    hipLaunchKernelGGL(score_rehash_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st,
                       static_cast<const unsigned long long*>(table_in), (unsigned long long)cap_in,
                       static_cast<unsigned long long*>(table_out), (unsigned long long)cap_out);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

int gnncca_track_score_add(const int64_t* ids, const int32_t* cam, const int64_t* node_track, const int32_t* node_ptr_dev, int64_t node_base,
                           int64_t n_nodes, int32_t n_frames, int32_t max_ids, int32_t max_cams, void* table, int64_t cap, int64_t* last,
                           int32_t* slot, int32_t* switched, gnncca_stream_t stream) {
    using namespace gnncca;
    if (n_nodes < 0 || n_frames < 0 || node_base < 0) return GNNCCA_ERR_INVALID_ARG;
    if (max_ids < 1 || max_ids > GNNCCA_SCORE_MAX_IDS || max_cams < 1 || max_cams > GNNCCA_SCORE_MAX_CAMS) return GNNCCA_ERR_INVALID_ARG;
    const long long K = (long long)max_ids * max_cams;
    if (K > GNNCCA_SCORE_MAX_STREAMS || (long long)n_frames * K > GNNCCA_SCORE_MAX_SLOTS) return GNNCCA_ERR_INVALID_ARG;
    if (n_nodes >= (1ll << 31) - 256) return GNNCCA_ERR_INVALID_ARG;
    if (!score_cap_ok(cap) || !table || !last) return GNNCCA_ERR_INVALID_ARG;
    if (n_frames == 0 || n_nodes == 0) return GNNCCA_OK;   // nothing to score: the state holds no time, so nothing changes
    if (!ids || !cam || !node_track || !node_ptr_dev || !slot || !switched) return GNNCCA_ERR_INVALID_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(slot, 0, (size_t)n_frames * (size_t)K * sizeof(int32_t), st));
    hipLaunchKernelGGL(score_scatter_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const long long*>(ids),
                       cam, reinterpret_cast<const long long*>(node_track), node_ptr_dev, (long long)node_base, (int)n_nodes, (int)n_frames,
                       (int)max_ids, (int)max_cams, (int)K, slot, switched);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(score_walk_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const long long*>(node_track),
                       (int)n_nodes, (int)n_frames, (int)max_cams, (int)K, slot, static_cast<unsigned long long*>(table), (unsigned long long)cap,
                       reinterpret_cast<long long*>(last), switched);
    HIP_TRY(hipGetLastError());
    return GNNCCA_OK;
}

}  // extern "C"
