// agent_wide.hip -- the wide form of the SAC actor's and critic's forward (agent_wide.hpp; hipets_set_agent_kernel): 64 rows per workgroup
// at every hidden width up to 1024, one launch per call, on the packed images hipets_policy_set / hipets_critic_set already make.
//   policy_act_wide_kernel<T>   GaussianPolicy.forward / sample, the tile form's tail (agent_forms.hpp: draws, head arithmetic, taps)
//   critic_q_wide_kernel<T>     QNetwork.forward, Q1 then Q2 through the same LDS
// T = 2, 4, 8: the h2 column tiles a wave can own (hidden <= 256, <= 512, <= 1024).  A unit of its own, compiled without packed fp32
// VALU instructions; policy.hip and value.hip, which hold the tile kernels, keep their flags and their code.
//
// The chain (wide_net).  The workgroup's 64 input rows sit in LDS, X [64][kp0 + 4].  h1 never exists at full width: for each chunk of
// wc of its columns
//   phase 1   the 8 waves compute relu(X W1[:, chunk] + b1[chunk]) into the chunk buffer H [64][wc + 4] (policy_layer's product: a
//             wave runs column tiles wave, wave + 8, ... of the chunk, 4 row tiles per weight fragment), barrier;
//   phase 2   every wave multiplies the chunk (K = wc) into ITS OWN column tiles of h2, whose accumulators stay in registers across all
//             chunks (up to 8 column tiles x 4 row tiles x 4 = 128 registers), barrier.
// Phase 2 runs TRANSPOSED: the weight fragment W2[16 kb + 4 q + s][n0 + r] is the A operand of v_mfma_f32_16x16x4_f32 and the
// ds_read_b128 of the h1 rows its B operand -- policy_layer's very loads, swapped -- so result lane (r, q) holds h2[row r][n0 + 4 q + j],
// j = 0..3: the A-operand layout of the NEXT layer for k-block n0.  After relu(acc + b2) the last layer therefore reads h2 from
// registers: each wave multiplies its k-blocks of h2 by the matching rows of the last layer's image, the 8 partial sums per (row,
// column) go through LDS (X and H are dead by then) and are added in wave order 0..7, then the bias.
// One LDS read of h1 feeds up to 8 column tiles (the tile form: one), and a weight element is fetched once per 64 rows at every width
// (the tile form at hidden 1024: once per 16).
// Summation order of every output element: k ascending through the chunks in ONE accumulator, the head partials in wave order -- fixed
// by the shape alone, so a row's result does not depend on its batch, its position or the grid.  Rows past the batch and columns past
// the real ones are staged as zeros; padded weights and biases are zeros (policy_pack_kernel), so no loop tests a bound.
#include <hip/hip_runtime.h>

#include "agent_forms.hpp"
#include "agent_wide.hpp"
#include "common.hpp"
#include "lds_optin.hpp"
#include "policy_layer.hpp"

namespace hipets {

namespace {

static_assert(kWideWaves * kWave == kPolicyThreads && kWideRows == 4 * kTile, "mlp_stage_input<4> stages the wide form's rows");
// phase 1: k-blocks whose weight loads a wave issues ahead of their MFMAs (policy_layer's kAhead).  4, the critic's choice, spills 10
// registers in critic_q_wide_kernel<8>, whose 128 accumulators are live through phase 1.
constexpr int kWideAhead = 2;

// H[64][cw] = relu(X[64][kp0] W[kp0][cw] + bias), W's rows `stride` floats apart (a column chunk of the [kp0][hp] image).
// One accumulator per row tile, k ascending.
__device__ __forceinline__ void wide_first_layer(const float* __restrict__ X, const int ld_x, const int kp0, const float* __restrict__ W,
                                                 const int stride, const float* __restrict__ bias, const int cw, float* __restrict__ H, const int ld_h,
                                                 const int wave, const int lane) {
    const int r = lane & 15, q = lane >> 4;
    for (int n0 = wave * kTile; n0 < cw; n0 += kWideWaves * kTile) {
        f32x4 c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* wp = W + (size_t)(4 * q) * stride + n0 + r;
        const float* ap = X + r * ld_x + 4 * q;
        int k0 = 0;
        for (; k0 + kWideAhead * kKChunk <= kp0; k0 += kWideAhead * kKChunk) {
            float bv[kWideAhead][4];
#pragma unroll
            for (int u = 0; u < kWideAhead; ++u) {
#pragma unroll
                for (int s = 0; s < 4; ++s) bv[u][s] = wp[(size_t)(u * kKChunk + s) * stride];
            }
#pragma unroll
            for (int u = 0; u < kWideAhead; ++u) {
                f32x4 av[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_x + u * kKChunk);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) c[i] = mfma4(av[i][s], bv[u][s], c[i]);
                }
            }
            wp += (size_t)(kWideAhead * kKChunk) * stride;
            ap += kWideAhead * kKChunk;
        }
        for (; k0 < kp0; k0 += kKChunk) {
            float bv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) bv[s] = wp[(size_t)s * stride];
            f32x4 av[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_x);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int i = 0; i < 4; ++i) c[i] = mfma4(av[i][s], bv[s], c[i]);
            }
            wp += (size_t)kKChunk * stride;
            ap += kKChunk;
        }
        const float bc = bias[n0 + r];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = c[i][j] + bc;
                H[(i * kTile + 4 * q + j) * ld_h + n0 + r] = v > 0.f ? v : 0.f;
            }
        }
    }
}

// acc[t][i] += (H[64][cw] W[cw][hp]) transposed, for this wave's `nt` column tiles n0 = 16 (wave + 8 t): lane (r, q) of acc[t][i] holds
// the sums of row 16 i + r, columns n0 + 4 q + j.  Per k-block: the weight fragments of all of the wave's tiles first (4 nt loads in
// flight), 4 ds_read_b128 of the chunk, then 16 nt MFMAs.
template <int T>
__device__ __forceinline__ void wide_second_layer(const float* __restrict__ H, const int ld_h, const int cw, const float* __restrict__ W, const int hp,
                                                  f32x4 (&acc)[T][4], const int nt, const int wave, const int lane) {
    const int r = lane & 15, q = lane >> 4;
    const float* hr = H + r * ld_h + 4 * q;
    const float* wp = W + (size_t)(4 * q) * hp + wave * kTile + r;
    for (int kb = 0; kb < cw; kb += kKChunk) {
        float a[T][4];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t < nt) {
#pragma unroll
                for (int s = 0; s < 4; ++s) a[t][s] = wp[(size_t)s * hp + t * kWideWaves * kTile];
            }
        }
        f32x4 b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = *reinterpret_cast<const f32x4*>(hr + i * kTile * ld_h);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t < nt) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[t][i] = mfma4(a[t][s], b[i][s], acc[t][i]);
                }
            }
        }
        wp += (size_t)kKChunk * hp;
        hr += kKChunk;
    }
}

// The whole network of the 64 staged rows X: leaves the 8 waves' partial sums of the last layer in P [8][64][np_last + 4] (P overlays X
// and H) behind a barrier.  The caller's barrier precedes it (X complete).
template <int T>
__device__ __forceinline__ void wide_net(const float* X, float* H, float* P, const WideNet& n, const WideGeo& g, const int wave, const int lane) {
    const int r = lane & 15, q = lane >> 4;
    const int ld_x = g.kp0 + 4, ld_h = g.wc + 4, ld_p = g.np_last + 4;
    const int left = g.hp / kTile - wave;  // column tiles wave, wave + 8, ... below hp / 16
    const int nt = left > 0 ? (left + kWideWaves - 1) / kWideWaves : 0;
    f32x4 acc[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int c0 = 0; c0 < g.hp; c0 += g.wc) {
        const int cw = min(g.wc, g.hp - c0);
        wide_first_layer(X, ld_x, g.kp0, n.w1 + c0, g.hp, n.b1 + c0, cw, H, ld_h, wave, lane);
        __syncthreads();
        wide_second_layer<T>(H, ld_h, cw, n.w2 + (size_t)c0 * g.hp, g.hp, acc, nt, wave, lane);
        __syncthreads();  // (the next chunk's phase 1 writes H; behind the last chunk P does)
    }
    // h2 = relu(acc + b2), in place: lane (r, q) holds columns n0 + 4 q + j
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t < nt) {
            const f32x4 b2 = *reinterpret_cast<const f32x4*>(n.b2 + (wave + t * kWideWaves) * kTile + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = acc[t][i][j] + b2[j];
                    acc[t][i][j] = v > 0.f ? v : 0.f;
                }
            }
        }
    }
    // the last layer, h2 from registers: this wave's k-blocks in ascending order into one accumulator per row tile (a wave without a
    // column tile leaves zeros)
    for (int m0 = 0; m0 < g.np_last; m0 += kTile) {
        f32x4 p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t < nt) {
                const float* wl = n.wl + (size_t)((wave + t * kWideWaves) * kTile + 4 * q) * g.np_last + m0 + r;
                float w[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) w[s] = wl[(size_t)s * g.np_last];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) p[i] = mfma4(acc[t][i][s], w[s], p[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) P[(wave * kWideRows + i * kTile + 4 * q + j) * ld_p + m0 + r] = p[i][j];
        }
    }
    __syncthreads();
}

// column `col` of the last layer for row `row` of the workgroup: the partial sums in wave order 0..7, then the bias
__device__ __forceinline__ float wide_head_sum(const float* P, const int ld_p, const int row, const int col, const float bias) {
    float v = P[row * ld_p + col];
#pragma unroll
    for (int w = 1; w < kWideWaves; ++w) v += P[(w * kWideRows + row) * ld_p + col];
    return v + bias;
}

template <int T>
__global__ __launch_bounds__(kPolicyThreads) void policy_act_wide_kernel(const WideActorArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wide_actor_smem[];
    float* X = wide_actor_smem;                             // [64][kp0 + 4]
    float* H = wide_actor_smem + kWideRows * (a.g.kp0 + 4);  // [64][wc + 4]
    float* P = wide_actor_smem;                             // [8][64][np_last + 4], behind the chain
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kWideRows;
    mlp_stage_input<4, false>(X, a.g.kp0 + 4, a.g.kp0, a.obs, a.obs_dim, nullptr, 0, a.B, row0, tid);
    __syncthreads();
    wide_net<T>(X, H, P, a.net, a.g, wave, lane);  // columns [0, act) mean, [act, 2 act) log_std
    // policy_act_kernel's tail on the summed heads
    const int ld_p = a.g.np_last + 4;
    const int nblk = (a.act + 3) >> 2;
    for (int t = tid; t < kWideRows * nblk; t += kPolicyThreads) {
        const int r = t / nblk, blk = t - r * nblk;
        const long long row = row0 + r;
        if (row >= a.B) continue;
        float nrm[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.sample && !a.eps) policy_normals4((uint32_t)row, (uint32_t)blk, a.seed, a.stream_id, nrm);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int d = 4 * blk + s;
            if (d < a.act) {
                const float mean = wide_head_sum(P, ld_p, r, d, a.net.bl[d]);
                const float raw = wide_head_sum(P, ld_p, r, a.act + d, a.net.bl[a.act + d]);
                const long long o = row * a.act + d;
                float ls;
                a.actions[o] = policy_head_action(mean, raw, a.sample != 0, a.sample ? (a.eps ? a.eps[o] : nrm[s]) : 0.f, a.scale[d], a.bias[d], ls);
                if (a.mean_out) a.mean_out[o] = mean;
                if (a.log_std_out) a.log_std_out[o] = ls;
            }
        }
    }
}

template <int T>
__global__ __launch_bounds__(kPolicyThreads) void critic_q_wide_kernel(const WideCriticArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wide_critic_smem[];
    float* X = wide_critic_smem;
    float* H = wide_critic_smem + kWideRows * (a.g.kp0 + 4);
    float* P = wide_critic_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kWideRows;
    float q1 = 0.f, q2 = 0.f;
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        // [s, a], staged again for Q2: P overlaid it
        mlp_stage_input<4, true>(X, a.g.kp0 + 4, a.g.kp0, a.obs, a.obs_dim, a.actions, a.act, a.B, row0, tid);
        __syncthreads();
        wide_net<T>(X, H, P, a.net[net], a.g, wave, lane);  // one column tile, column 0 real
        const float qn = tid < kWideRows ? wide_head_sum(P, a.g.np_last + 4, tid, 0, a.net[net].bl[0]) : 0.f;
        if (net == 0) q1 = qn;
        else q2 = qn;
        __syncthreads();  // (P is read; the next staging writes over it)
    }
    const long long row = row0 + tid;
    if (tid < kWideRows && row < a.B) {
        if (a.q1) a.q1[row] = q1;
        if (a.q2) a.q2[row] = q2;
        // torch.min(q1, q2) as critic_q_kernel selects it: the smaller one, q2 on a tie, NaN when either is NaN
        if (a.qmin) a.qmin[row] = (q1 < q2 || q1 != q1) ? q1 : q2;
    }
}

// one launch of a kernel family (its T = 2, 4, 8 instances) at g.tiles column tiles per wave
template <auto kK2, auto kK4, auto kK8, class Args>
hipError_t launch_wide(const Args& a, size_t lds_max, hipStream_t st) {
    static LdsOptIn opted[3];
    void (*kernel)(Args) = kK8;
    LdsOptIn* once = &opted[2];
    if (a.g.tiles <= 2) { kernel = kK2; once = &opted[0]; }
    else if (a.g.tiles <= 4) { kernel = kK4; once = &opted[1]; }
    if (a.g.lds > 64 * 1024) {
        const hipError_t err = full_lds_once(*once, reinterpret_cast<const void*>(kernel), (int)lds_max);
        if (err != hipSuccess) return err;
    }
    const unsigned grid = (unsigned)(((long long)a.B + kWideRows - 1) / kWideRows);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPolicyThreads), (size_t)a.g.lds, st, a);
    return hipGetLastError();
}

}  // namespace

int wide_geometry_query(int batch, int k0, int hidden, int last_cols, size_t lds_max, int* row_tiles, int* lds_bytes) {
    if (batch < 1) return fail("bad batch");
    WideGeo g{};
    if (!agent_wide_geometry(k0, hidden, last_cols, lds_max, g)) return fail("network does not fit the wide kernel's LDS");
    if (row_tiles) *row_tiles = kWideRows / kTile;
    if (lds_bytes) *lds_bytes = g.lds;
    return 0;
}

hipError_t launch_actor_wide(const WideActorArgs& a, size_t lds_max, hipStream_t st) {
    return launch_wide<policy_act_wide_kernel<2>, policy_act_wide_kernel<4>, policy_act_wide_kernel<8>>(a, lds_max, st);
}

hipError_t launch_critic_wide(const WideCriticArgs& a, size_t lds_max, hipStream_t st) {
    return launch_wide<critic_q_wide_kernel<2>, critic_q_wide_kernel<4>, critic_q_wide_kernel<8>>(a, lds_max, st);
}

}  // namespace hipets
