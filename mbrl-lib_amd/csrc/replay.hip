// replay.hip -- SAC transitions on the device (layout: transition_layout.hpp): hipets_compact_transitions / hipets_ring_compact_transitions
// (mbpo.py:53-63, numpy's boolean indexing with ~accum_dones, as three ordered launches) and hipets_replay_gather.  Kernels, then entry points.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "engine.hpp"
#include "transition_layout.hpp"

namespace hipets {

namespace {

// The compaction: rows with accum_dones == 0 keep their order.  Blocks of kCompactThreads rows: (1) every block counts its kept rows,
// (2) ONE workgroup turns the counts into exclusive offsets, kScanThreads blocks per pass with a running carry, reads the staging
// area's fill and advances it, (3) every block ranks its own kept rows (ballots) and copies them.  Launch order is the only
// synchronisation between the three.  Plain copies: the staged floats are the source's bits.
constexpr int kCompactThreads = 256;
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(const unsigned char* __restrict__ accum, int n, int* __restrict__ counts) {
    __shared__ int wsum[kCompactThreads / kWave];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * kCompactThreads + tid;
    const bool keep = i < n && accum[i] == 0;
    const unsigned long long m = __ballot(keep);
    if ((tid & 63) == 0) wsum[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < kCompactThreads / kWave; ++w) s += wsum[w];
        counts[blockIdx.x] = s;
    }
}

// counts [nb] -> exclusive offsets in place; *base_out = *offset (the step's first staging row); *offset += kept; *count_out = kept.
// kRing: `offset` is a replay buffer's (cur_idx, num_stored) over `cap` rows; *base_out = cur_idx, then ReplayBuffer.add_batch's
// bookkeeping (replay_buffer.py:598-599): cur_idx = (cur_idx + kept) % cap, num_stored = min(num_stored + kept, cap).  A cur_idx
// outside [0, cap) is folded into it first, so the scatter's rows are in bounds whatever the cursor held.
template <bool kRing>
__global__ __launch_bounds__(kScanThreads) void compact_scan_kernel(int* __restrict__ counts, int nb, long long* __restrict__ offset,
                                                                    int* __restrict__ count_out, long long* __restrict__ base_out,
                                                                    long long cap) {
    __shared__ int wtot[kScanThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;  // (kept rows <= n < 2^31)
    for (int c0 = 0; c0 < nb; c0 += kScanThreads) {
        const int i = c0 + tid;
        const int v = i < nb ? counts[i] : 0;
        int x = v;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == kWave - 1) wtot[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kScanThreads / kWave; ++w) {
            const int s = wtot[w];
            if (w < wave) before += s;
            total += s;
        }
        if (i < nb) counts[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) {
        if constexpr (kRing) {
            long long base = offset[0] % cap;
            if (base < 0) base += cap;
            *base_out = base;
            offset[0] = (base + carry) % cap;
            offset[1] = min(max(offset[1], 0ll) + carry, cap);
        } else {
            const long long base = *offset;
            *base_out = base;
            *offset = base + carry;
        }
        *count_out = carry;
    }
}

// kRing: row k of the step lands at ring row (*base_p + k) % cap (k < n <= cap and *base_p < cap: one subtraction); nothing is dropped
template <bool kRing>
__global__ __launch_bounds__(kCompactThreads) void compact_scatter_kernel(const float* __restrict__ obs, const float* __restrict__ action,
                                                                          const float* __restrict__ next_obs, const float* __restrict__ rewards,
                                                                          const unsigned char* __restrict__ dones, unsigned char* __restrict__ accum,
                                                                          int n, int od, int ad, float* __restrict__ staging, long long cap,
                                                                          const long long* __restrict__ base_p, const int* __restrict__ offs) {
    __shared__ long long dst_s[kCompactThreads];
    __shared__ int wsum[kCompactThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long blk0 = (long long)blockIdx.x * kCompactThreads;
    const long long i = blk0 + tid;
    const bool keep = i < n && accum[i] == 0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();  // (every read of accum is above this line; the update is at the end)
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    long long d = -1;
    if (keep) {
        d = *base_p + offs[blockIdx.x] + before + __popcll(m & ((1ull << lane) - 1ull));
        if (d >= cap) d = kRing ? d - cap : -1;
    }
    dst_s[tid] = d;
    __syncthreads();
    const TransitionLayout L(od, ad, cap);
    const int W = L.width;
    const int rows_here = (int)min((long long)kCompactThreads, (long long)n - blk0);
    for (int t = tid; t < rows_here * W; t += kCompactThreads) {
        const int r = t / W, c = t - r * W;
        const long long dst = dst_s[r];
        if (dst < 0) continue;
        const long long row = blk0 + r;
        if (c < L.c_act) staging[dst * od + c] = obs[row * od + c];
        else if (c < L.c_next) staging[L.o_act + dst * ad + (c - L.c_act)] = action[row * ad + (c - L.c_act)];
        else if (c < L.c_rew) staging[L.o_nobs + dst * od + (c - L.c_next)] = next_obs[row * od + (c - L.c_next)];
        else if (c == L.c_rew) staging[L.o_rew + dst] = rewards[row];
        else staging[L.o_done + dst] = dones[row] ? 1.f : 0.f;
    }
    if (i < n && dones[i]) accum[i] = 1;
}

// The gather: out[j] = (obs[i], action[i], next_obs[i], reward[i], mask) of ring row i = indices[j], the batch row hipets_sac_update
// reads.  A block owns kGatherRows output rows, their indices staged in LDS, and walks them as ONE flat (row, column) range: the
// output write is contiguous over the whole block, each segment read contiguous within its row.  Plain copies.  An index outside
// [0, cap) reads nothing: its row is quiet NaN.
constexpr int kGatherThreads = 256;
constexpr int kGatherRows = 16;

__global__ __launch_bounds__(kGatherThreads) void replay_gather_kernel(const float* __restrict__ ring, long long cap, int od, int ad,
                                                                       const long long* __restrict__ indices, long long n_rows, int reverse_mask,
                                                                       float* __restrict__ out) {
    __shared__ long long idx_s[kGatherRows];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * kGatherRows;
    const int rows_here = (int)min((long long)kGatherRows, n_rows - row0);
    if (tid < rows_here) {
        const long long i = indices[row0 + tid];
        idx_s[tid] = (i >= 0 && i < cap) ? i : -1;
    }
    __syncthreads();
    const TransitionLayout L(od, ad, cap);
    const int W = L.width;
    float* __restrict__ dst = out + row0 * W;
    for (int t = tid; t < rows_here * W; t += kGatherThreads) {
        const int r = t / W, c = t - r * W;
        const long long i = idx_s[r];
        float v = __int_as_float(0x7fc00000);
        if (i >= 0) {
            if (c < L.c_act) v = ring[i * od + c];
            else if (c < L.c_next) v = ring[L.o_act + i * ad + (c - L.c_act)];
            else if (c < L.c_rew) v = ring[L.o_nobs + i * od + (c - L.c_next)];
            else if (c == L.c_rew) v = ring[L.o_rew + i];
            else {
                const float done = ring[L.o_done + i];
                v = reverse_mask ? (done == 0.f ? 1.f : 0.f) : done;
            }
        }
        dst[t] = v;
    }
}

// count, scan, scatter of one step's n rows into `area` (cap rows; kRing: `offset` is the ring's cursor), behind the checks of its form
template <bool kRing>
int compact_impl(hipets_engine* e, const float* obs, const float* action, const float* next_obs, const float* rewards, const uint8_t* dones,
                 uint8_t* accum_dones, int n, int obs_dim, int act_dim, float* area, long long cap, int64_t* offset, int32_t* count_out, void* stream) {
    if (!e) return fail("null engine");
    if (!obs || !action || !next_obs || !rewards || !dones || !accum_dones || !area || !offset || !count_out) return fail("null argument");
    if (n < 1) return fail("bad row count");
    if (obs_dim < 1 || obs_dim > 4096 || act_dim < 1 || act_dim > 4096) return fail("obs_dim / act_dim outside [1, 4096]");
    if (!kRing && cap < 0) return fail("negative staging capacity");
    if (kRing && cap < 1) return fail("ring capacity < 1");
    if (kRing && n > cap) return fail("a step of %d rows does not fit a ring of %lld", n, cap);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const int nb = (int)(((long long)n + kCompactThreads - 1) / kCompactThreads);
    if (e->compact_counts.ensure(8 + (size_t)nb * 4)) return 1;
    long long* base = e->compact_counts.as<long long>();
    int* counts = reinterpret_cast<int*>(base + 1);
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, accum_dones, n, counts);
    hipLaunchKernelGGL(compact_scan_kernel<kRing>, dim3(1), dim3(kScanThreads), 0, st, counts, nb, reinterpret_cast<long long*>(offset), count_out, base,
                       cap);
    hipLaunchKernelGGL(compact_scatter_kernel<kRing>, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, obs, action, next_obs, rewards, dones, accum_dones,
                       n, obs_dim, act_dim, area, cap, base, counts);
    HCHECK(hipGetLastError());
    return 0;
}

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_compact_transitions(hipets_engine* e, const float* obs, const float* action, const float* next_obs, const float* rewards,
                               const uint8_t* dones, uint8_t* accum_dones, int32_t n, int32_t obs_dim, int32_t act_dim, float* staging,
                               int64_t cap, int64_t* offset, int32_t* count_out, void* stream) {
    return compact_impl<false>(e, obs, action, next_obs, rewards, dones, accum_dones, n, obs_dim, act_dim, staging, cap, offset, count_out, stream);
}

int hipets_ring_compact_transitions(hipets_engine* e, const float* obs, const float* action, const float* next_obs, const float* rewards,
                                    const uint8_t* dones, uint8_t* accum_dones, int32_t n, int32_t obs_dim, int32_t act_dim, float* ring,
                                    int64_t capacity, int64_t* cursor, int32_t* count_out, void* stream) {
    return compact_impl<true>(e, obs, action, next_obs, rewards, dones, accum_dones, n, obs_dim, act_dim, ring, capacity, cursor, count_out, stream);
}

int hipets_replay_gather(hipets_engine* e, const float* ring, int64_t capacity, int32_t obs_dim, int32_t act_dim, const int64_t* indices,
                         int64_t n_rows, int32_t reverse_mask, float* out, void* stream) {
    if (!e) return fail("null engine");
    if (!ring || !indices || !out) return fail("null argument");
    if (obs_dim < 1 || obs_dim > 4096 || act_dim < 1 || act_dim > 4096) return fail("obs_dim / act_dim outside [1, 4096]");
    if (capacity < 1) return fail("ring capacity < 1");
    const long long nb = ((long long)n_rows + kGatherRows - 1) / kGatherRows;
    if (n_rows < 1 || nb > 0x7fffffffll) return fail("bad row count");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    hipLaunchKernelGGL(replay_gather_kernel, dim3((unsigned)nb), dim3(kGatherThreads), 0, st, ring, (long long)capacity, obs_dim, act_dim,
                       reinterpret_cast<const long long*>(indices), (long long)n_rows, reverse_mask, out);
    HCHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
