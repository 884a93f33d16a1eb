// policy.hip -- the model-side pieces of an MBPO rollout (mbrl/algorithms/mbpo.py:31-63) that are not the dynamics model: the SAC
// Gaussian actor's forward (hipets_policy_set / _act / _normals / _geometry) and the stable compaction of a step's transitions into a
// device staging area (hipets_compact_transitions).  The kernels, then the entry points.
//   policy_act_kernel          GaussianPolicy.forward / sample (third_party/pytorch_sac_pranz24/model.py:88-108), one launch per call
//   compact_{count,scan,scatter}_kernel   mbpo.py:53-63: numpy's boolean indexing with ~accum_dones as three ordered launches; the
//                                         scan and the scatter also in a RING form (hipets_ring_compact_transitions: the kept rows go
//                                         where ReplayBuffer.add_batch puts them)
//   replay_gather_kernel                  rows of a ring by index -> the [n, 2 obs + act + 2] batch hipets_sac_update reads
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "engine.hpp"
#include "lds_optin.hpp"
#include "policy_layer.hpp"

namespace hipets {

namespace {

// ---------------------------------------------------------------------------------------------
// The actor.  A workgroup owns 16 R consecutive rows; their activations live in two LDS buffers that the layers alternate between
// (A: obs, then h2; B: h1, then the heads), the packed weights stream from L2.  The layer itself -- MFMA product, LDS layout, padding
// rule -- is policy_layer.hpp's, shared with the critic kernel (value.hip).
// ---------------------------------------------------------------------------------------------
constexpr float kLogSigMin = -20.f, kLogSigMax = 2.f;  // LOG_SIG_MIN / LOG_SIG_MAX (pytorch_sac_pranz24/model.py:6-7)

struct PolicyArgs {
    const float* obs;      // [B, obs_dim]
    const float* eps;      // [B, act] or null
    float* actions;        // [B, act]
    float* mean_out;       // [B, act] or null
    float* log_std_out;    // [B, act] or null
    const float *w1, *w2, *wh;  // packed [kp0][hp], [hp][hp], [hp][nph]
    const float *b1, *b2, *bh;  // [hp], [hp], [nph] (zero padded)
    const float *scale, *bias;  // [act]
    int B, obs_dim, act;
    int kp0, hp, nph;  // obs_dim, hidden, 2 act rounded up to 16
    int ld_a, ld_b;
    int sample;
    unsigned long long seed, stream_id;
};

// eps of (row, dims 4 blk .. 4 blk + 3): Philox4x32-10 with the counter word "POLI" where the rollouts' draws carry their step, under a
// key of its own -- no actor draw shares a (counter, key) with a model draw of the same (seed, stream)
__device__ __forceinline__ void policy_normals4(uint32_t row, uint32_t blk, unsigned long long seed, unsigned long long stream_id, float (&nrm)[4]) {
    const Philox4 r4 = philox4x32_10(row, 0x504F4C49u /* "POLI" */, blk, (uint32_t)stream_id, (uint32_t)seed,
                                     (uint32_t)(seed >> 32) ^ (uint32_t)(stream_id >> 32) ^ 0xAC7012ACu);
    box_muller(r4.x, r4.y, nrm[0], nrm[1]);
    box_muller(r4.z, r4.w, nrm[2], nrm[3]);
}

template <int R>
__global__ __launch_bounds__(kPolicyThreads) void policy_act_kernel(const PolicyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float policy_smem[];
    constexpr int kRows = kTile * R;
    float* bufA = policy_smem;                  // [kRows][ld_a]
    float* bufB = policy_smem + kRows * a.ld_a;  // [kRows][ld_b]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kRows;
    // the observations, zero padded to kp0 columns; rows past the batch are zeros
    for (int t = tid; t < kRows * a.kp0; t += kPolicyThreads) {
        const int r = t / a.kp0, k = t - r * a.kp0;
        const long long row = row0 + r;
        bufA[r * a.ld_a + k] = (row < a.B && k < a.obs_dim) ? a.obs[row * a.obs_dim + k] : 0.f;
    }
    __syncthreads();
    policy_layer<R, true>(bufA, a.ld_a, a.kp0, a.w1, a.b1, a.hp, bufB, a.ld_b, wave, lane);
    __syncthreads();
    policy_layer<R, true>(bufB, a.ld_b, a.hp, a.w2, a.b2, a.hp, bufA, a.ld_a, wave, lane);
    __syncthreads();
    policy_layer<R, false>(bufA, a.ld_a, a.hp, a.wh, a.bh, a.nph, bufB, a.ld_b, wave, lane);  // columns [0, act) mean, [act, 2 act) log_std
    __syncthreads();
    const int nblk = (a.act + 3) >> 2;
    for (int t = tid; t < kRows * nblk; t += kPolicyThreads) {
        const int r = t / nblk, blk = t - r * nblk;
        const long long row = row0 + r;
        if (row >= a.B) continue;
        float nrm[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.sample && !a.eps) policy_normals4((uint32_t)row, (uint32_t)blk, a.seed, a.stream_id, nrm);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int d = 4 * blk + s;
            if (d < a.act) {
                const float mean = bufB[r * a.ld_b + d];
                float ls = bufB[r * a.ld_b + a.act + d];
                ls = ls < kLogSigMin ? kLogSigMin : (ls > kLogSigMax ? kLogSigMax : ls);  // torch.clamp (a NaN stays a NaN)
                const long long o = row * a.act + d;
                float x = mean;
                if (a.sample) {
                    const float e = a.eps ? a.eps[o] : nrm[s];
                    x = mean + expf(ls) * e;  // Normal.rsample: loc + eps * scale
                }
                a.actions[o] = tanhf(x) * a.scale[d] + a.bias[d];
                if (a.mean_out) a.mean_out[o] = mean;
                if (a.log_std_out) a.log_std_out[o] = ls;
            }
        }
    }
}

__global__ void policy_normals_kernel(float* out, int B, int act, unsigned long long seed, unsigned long long stream_id) {
    const int nblk = (act + 3) >> 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * nblk) return;
    const long long row = i / nblk;
    const int blk = (int)(i - row * nblk);
    float nrm[4];
    policy_normals4((uint32_t)row, (uint32_t)blk, seed, stream_id, nrm);
    for (int s = 0; s < 4; ++s) {
        const int d = 4 * blk + s;
        if (d < act) out[row * act + d] = nrm[s];
    }
}

struct PolicyGeo {
    int kp0, hp, nph, ld_a, ld_b, R;
    size_t lds;
};

// The R rule is policy_layer.hpp's policy_row_tiles.
PolicyGeo policy_geometry(const hipets_engine* e, long long batch) {
    PolicyGeo g{};
    g.kp0 = pad16(e->policy_obs);
    g.hp = pad16(e->policy_hid);
    g.nph = pad16(2 * e->policy_act);
    g.ld_a = std::max(g.kp0, g.hp) + 4;
    g.ld_b = std::max(g.hp, g.nph) + 4;
    const size_t per_tile = (size_t)kTile * 4 * (size_t)(g.ld_a + g.ld_b);
    g.R = policy_row_tiles(per_tile, e->lds_max, batch);
    g.lds = per_tile * g.R;
    return g;
}

template <int R>
hipError_t launch_policy(const PolicyGeo& g, int lds_max, const PolicyArgs& a, hipStream_t st) {
    static LdsOptIn once;
    if (g.lds > 64 * 1024) {
        const hipError_t err = full_lds_once(once, reinterpret_cast<const void*>(&policy_act_kernel<R>), lds_max);
        if (err != hipSuccess) return err;
    }
    const unsigned grid = (unsigned)(((long long)a.B + kTile * R - 1) / (kTile * R));
    hipLaunchKernelGGL(policy_act_kernel<R>, dim3(grid), dim3(kPolicyThreads), g.lds, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The compaction: rows with accum_dones == 0 keep their order.  Blocks of kCompactThreads rows: (1) every block counts its kept rows,
// (2) ONE workgroup turns the counts into exclusive offsets, kScanThreads blocks per pass with a running carry, reads the staging
// area's fill and advances it, (3) every block ranks its own kept rows (ballots) and copies them.  Launch order is the only
// synchronisation between the three.  Plain copies: the staged floats are the source's bits.
// ---------------------------------------------------------------------------------------------
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
    const int W = 2 * od + ad + 2;
    // the five arrays of the staging area, one behind the other (hipets.h)
    const long long o_act = cap * od, o_nobs = cap * (od + ad), o_rew = cap * (2 * od + ad), o_done = o_rew + cap;
    const int rows_here = (int)min((long long)kCompactThreads, (long long)n - blk0);
    for (int t = tid; t < rows_here * W; t += kCompactThreads) {
        const int r = t / W, c = t - r * W;
        const long long dst = dst_s[r];
        if (dst < 0) continue;
        const long long row = blk0 + r;
        if (c < od) staging[dst * od + c] = obs[row * od + c];
        else if (c < od + ad) staging[o_act + dst * ad + (c - od)] = action[row * ad + (c - od)];
        else if (c < 2 * od + ad) staging[o_nobs + dst * od + (c - od - ad)] = next_obs[row * od + (c - od - ad)];
        else if (c == 2 * od + ad) staging[o_rew + dst] = rewards[row];
        else staging[o_done + dst] = dones[row] ? 1.f : 0.f;
    }
    if (i < n && dones[i]) accum[i] = 1;
}

// ---------------------------------------------------------------------------------------------
// The gather: out[j] = (obs[i], action[i], next_obs[i], reward[i], mask) of ring row i = indices[j], the batch row hipets_sac_update
// reads.  A block owns kGatherRows output rows, their indices staged in LDS, and walks them as ONE flat (row, column) range: the
// output write is contiguous over the whole block, each segment read contiguous within its row.  Plain copies.  An index outside
// [0, cap) reads nothing: its row is quiet NaN.
// ---------------------------------------------------------------------------------------------
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
    const int W = 2 * od + ad + 2;
    const long long o_act = cap * od, o_nobs = cap * (od + ad), o_rew = cap * (2 * od + ad), o_done = o_rew + cap;
    float* __restrict__ dst = out + row0 * W;
    for (int t = tid; t < rows_here * W; t += kGatherThreads) {
        const int r = t / W, c = t - r * W;
        const long long i = idx_s[r];
        float v = __int_as_float(0x7fc00000);
        if (i >= 0) {
            if (c < od) v = ring[i * od + c];
            else if (c < od + ad) v = ring[o_act + i * ad + (c - od)];
            else if (c < 2 * od + ad) v = ring[o_nobs + i * od + (c - od - ad)];
            else if (c == 2 * od + ad) v = ring[o_rew + i];
            else {
                const float done = ring[o_done + i];
                v = reverse_mask ? (done == 0.f ? 1.f : 0.f) : done;
            }
        }
        dst[t] = v;
    }
}

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_policy_set(hipets_engine* e, int32_t obs_dim, int32_t hidden, int32_t act_dim, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* wm, const float* bm, const float* ws, const float* bs, const float* action_scale,
                      const float* action_bias, void* stream) {
    if (!e) return fail("null engine");
    if (!w1 || !b1 || !w2 || !b2 || !wm || !bm || !ws || !bs || !action_scale || !action_bias) return fail("null argument");
    if (obs_dim < 1 || obs_dim > HIPETS_POLICY_MAX_OBS) return fail("policy obs_dim %d outside [1, %d]", obs_dim, HIPETS_POLICY_MAX_OBS);
    if (hidden < 1 || hidden > HIPETS_POLICY_MAX_HIDDEN) return fail("policy hidden width %d outside [1, %d]", hidden, HIPETS_POLICY_MAX_HIDDEN);
    if (act_dim < 1 || act_dim > HIPETS_POLICY_MAX_ACT) return fail("policy act_dim %d outside [1, %d]", act_dim, HIPETS_POLICY_MAX_ACT);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    e->has_policy = false;
    e->policy_obs = obs_dim;
    e->policy_hid = hidden;
    e->policy_act = act_dim;
    const PolicyGeo g = policy_geometry(e, 1);
    if ((size_t)kTile * 4 * (size_t)(g.ld_a + g.ld_b) > e->lds_max) return fail("policy too wide for LDS");
    const size_t n1 = (size_t)g.kp0 * g.hp, n2 = (size_t)g.hp * g.hp, n3 = (size_t)g.hp * g.nph;
    const size_t nb = (size_t)2 * g.hp + g.nph + 2 * (size_t)act_dim;
    if (e->policy_w.ensure((n1 + n2 + n3) * 4) || e->policy_b.ensure(nb * 4)) return 1;
    float* W = e->policy_w.as<float>();
    float* Bv = e->policy_b.as<float>();
    HCHECK(hipMemsetAsync(W, 0, (n1 + n2 + n3) * 4, st));
    HCHECK(hipMemsetAsync(Bv, 0, nb * 4, st));
    auto pack = [&](float* dst, const float* src, int K, int N, int np, int col0) {
        const long long n = (long long)K * N;
        hipLaunchKernelGGL(policy_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, K, N, np, col0);
    };
    pack(W, w1, obs_dim, hidden, g.hp, 0);
    pack(W + n1, w2, hidden, hidden, g.hp, 0);
    pack(W + n1 + n2, wm, hidden, act_dim, g.nph, 0);
    pack(W + n1 + n2, ws, hidden, act_dim, g.nph, act_dim);
    HCHECK(hipGetLastError());
    float* bh = Bv + 2 * g.hp;
    float* sc = bh + g.nph;
    HCHECK(hipMemcpyAsync(Bv, b1, (size_t)hidden * 4, hipMemcpyDeviceToDevice, st));
    HCHECK(hipMemcpyAsync(Bv + g.hp, b2, (size_t)hidden * 4, hipMemcpyDeviceToDevice, st));
    HCHECK(hipMemcpyAsync(bh, bm, (size_t)act_dim * 4, hipMemcpyDeviceToDevice, st));
    HCHECK(hipMemcpyAsync(bh + act_dim, bs, (size_t)act_dim * 4, hipMemcpyDeviceToDevice, st));
    HCHECK(hipMemcpyAsync(sc, action_scale, (size_t)act_dim * 4, hipMemcpyDeviceToDevice, st));
    HCHECK(hipMemcpyAsync(sc + act_dim, action_bias, (size_t)act_dim * 4, hipMemcpyDeviceToDevice, st));
    e->has_policy = true;
    return 0;
}

int hipets_policy_act(hipets_engine* e, const float* obs, int32_t batch, int32_t sample, uint64_t seed, uint64_t stream_id, const float* eps,
                      float* actions, float* mean_out, float* log_std_out, void* stream) {
    if (!e || !e->has_policy) return fail("engine has no policy (call hipets_policy_set)");
    if (!obs || !actions) return fail("null argument");
    if (batch < 1) return fail("bad batch");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const PolicyGeo g = policy_geometry(e, batch);
    const size_t n1 = (size_t)g.kp0 * g.hp, n2 = (size_t)g.hp * g.hp;
    PolicyArgs a{};
    a.obs = obs; a.eps = eps; a.actions = actions; a.mean_out = mean_out; a.log_std_out = log_std_out;
    a.w1 = e->policy_w.as<float>(); a.w2 = a.w1 + n1; a.wh = a.w2 + n2;
    a.b1 = e->policy_b.as<float>(); a.b2 = a.b1 + g.hp; a.bh = a.b2 + g.hp;
    a.scale = a.bh + g.nph; a.bias = a.scale + e->policy_act;
    a.B = batch; a.obs_dim = e->policy_obs; a.act = e->policy_act;
    a.kp0 = g.kp0; a.hp = g.hp; a.nph = g.nph; a.ld_a = g.ld_a; a.ld_b = g.ld_b;
    a.sample = sample != 0;
    a.seed = seed; a.stream_id = stream_id;
    hipError_t err;
    switch (g.R) {
        case 4: err = launch_policy<4>(g, (int)e->lds_max, a, st); break;
        case 2: err = launch_policy<2>(g, (int)e->lds_max, a, st); break;
        default: err = launch_policy<1>(g, (int)e->lds_max, a, st); break;
    }
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "policy kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

int hipets_policy_normals(hipets_engine* e, int32_t batch, int32_t act_dim, uint64_t seed, uint64_t stream_id, float* out, void* stream) {
    if (!e || !out) return fail("null argument");
    if (batch < 1) return fail("bad batch");
    if (act_dim < 1 || act_dim > HIPETS_POLICY_MAX_ACT) return fail("policy act_dim %d outside [1, %d]", act_dim, HIPETS_POLICY_MAX_ACT);
    HCHECK(hipSetDevice(e->device));
    const long long n = (long long)batch * ((act_dim + 3) / 4);
    hipLaunchKernelGGL(policy_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, batch, act_dim,
                       (unsigned long long)seed, (unsigned long long)stream_id);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_policy_geometry(hipets_engine* e, int32_t batch, int32_t* row_tiles, int32_t* lds_bytes) {
    if (!e || !e->has_policy) return fail("engine has no policy (call hipets_policy_set)");
    if (batch < 1) return fail("bad batch");
    const PolicyGeo g = policy_geometry(e, batch);
    if (row_tiles) *row_tiles = g.R;
    if (lds_bytes) *lds_bytes = (int32_t)g.lds;
    return 0;
}

int hipets_compact_transitions(hipets_engine* e, const float* obs, const float* action, const float* next_obs, const float* rewards,
                               const uint8_t* dones, uint8_t* accum_dones, int32_t n, int32_t obs_dim, int32_t act_dim, float* staging,
                               int64_t cap, int64_t* offset, int32_t* count_out, void* stream) {
    if (!e) return fail("null engine");
    if (!obs || !action || !next_obs || !rewards || !dones || !accum_dones || !staging || !offset || !count_out) return fail("null argument");
    if (n < 1) return fail("bad row count");
    if (obs_dim < 1 || obs_dim > 4096 || act_dim < 1 || act_dim > 4096) return fail("obs_dim / act_dim outside [1, 4096]");
    if (cap < 0) return fail("negative staging capacity");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const int nb = (int)(((long long)n + kCompactThreads - 1) / kCompactThreads);
    if (e->compact_counts.ensure(8 + (size_t)nb * 4)) return 1;
    long long* base = e->compact_counts.as<long long>();
    int* counts = reinterpret_cast<int*>(base + 1);
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, accum_dones, n, counts);
    hipLaunchKernelGGL(compact_scan_kernel<false>, dim3(1), dim3(kScanThreads), 0, st, counts, nb, reinterpret_cast<long long*>(offset), count_out, base,
                       (long long)cap);
    hipLaunchKernelGGL(compact_scatter_kernel<false>, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, obs, action, next_obs, rewards, dones, accum_dones,
                       n, obs_dim, act_dim, staging, (long long)cap, base, counts);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_ring_compact_transitions(hipets_engine* e, const float* obs, const float* action, const float* next_obs, const float* rewards,
                                    const uint8_t* dones, uint8_t* accum_dones, int32_t n, int32_t obs_dim, int32_t act_dim, float* ring,
                                    int64_t capacity, int64_t* cursor, int32_t* count_out, void* stream) {
    if (!e) return fail("null engine");
    if (!obs || !action || !next_obs || !rewards || !dones || !accum_dones || !ring || !cursor || !count_out) return fail("null argument");
    if (n < 1) return fail("bad row count");
    if (obs_dim < 1 || obs_dim > 4096 || act_dim < 1 || act_dim > 4096) return fail("obs_dim / act_dim outside [1, 4096]");
    if (capacity < 1) return fail("ring capacity < 1");
    if ((int64_t)n > capacity) return fail("a step of %d rows does not fit a ring of %lld", n, (long long)capacity);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const int nb = (int)(((long long)n + kCompactThreads - 1) / kCompactThreads);
    if (e->compact_counts.ensure(8 + (size_t)nb * 4)) return 1;
    long long* base = e->compact_counts.as<long long>();
    int* counts = reinterpret_cast<int*>(base + 1);
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, accum_dones, n, counts);
    hipLaunchKernelGGL(compact_scan_kernel<true>, dim3(1), dim3(kScanThreads), 0, st, counts, nb, reinterpret_cast<long long*>(cursor), count_out, base,
                       (long long)capacity);
    hipLaunchKernelGGL(compact_scatter_kernel<true>, dim3((unsigned)nb), dim3(kCompactThreads), 0, st, obs, action, next_obs, rewards, dones, accum_dones,
                       n, obs_dim, act_dim, ring, (long long)capacity, base, counts);
    HCHECK(hipGetLastError());
    return 0;
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
