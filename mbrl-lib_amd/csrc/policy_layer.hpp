// policy_layer.hpp -- everything the SAC actor kernel (policy.hip) and the SAC critic kernel (value.hip) share, an MLP whose activations
// live in two LDS buffers: one dense layer of a workgroup's 16 R rows on v_mfma_f32_16x16x4_f32, the staging of a workgroup's input rows,
// the geometry (padding, LDS row lengths, the R rule), the launch, the packing of nn.Linear layers into the layer's W[k][n] image, the
// size limits, and the log_std clamp of GaussianPolicy (sac.hip's tails use it too).  One definition each, so a layer's arithmetic and
// a network's host scaffold are the same in both kernels.  Internal linkage: each unit gets its own copy of the small pack kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "common.hpp"
#include "engine.hpp"
#include "lds_optin.hpp"

namespace hipets {

namespace {

// A workgroup owns 16 R consecutive rows; their activations live in two LDS buffers that the layers alternate between, the packed
// weights stream from L2.  Every product runs on v_mfma_f32_16x16x4_f32 through the compiler's builtin (its own hazard handling: no
// asm MFMA here).  A wave owns column tiles; for one column tile it keeps the R row tiles' accumulators, so a B fragment (4 coalesced
// loads of 16 consecutive floats per k-block of 16) feeds 4 R MFMAs.
// Inside a k-block of 16 lane group q = lane >> 4 supplies k = 16 kb + 4 q + s to MFMA s, for A and B alike (any assignment of the 16
// k to the 4 x 4 (step, group) slots sums the same products): the A operand of the four steps is ONE ds_read_b128.
//   packed weights  W[k][n], k < Kp (K rounded up to 16), n < Np (N rounded up to 16), zeros outside K x N (policy_pack_kernel)
//   LDS rows        ld = columns + 4 floats with columns a multiple of 16: ld = 4 (mod 16), so the 16 rows x 4 groups of an A read and
//                   the 4 row groups x 16 columns of a result store each fall on distinct banks
// Padding needs no bounds test in the loops: input columns past the real ones and rows past the batch are loaded as zeros, a padded
// output column is relu(0 + 0) = 0, which is what the next layer's padded k rows want.
constexpr int kPolicyThreads = 512;
constexpr int kPolicyWaves = kPolicyThreads / kWave;

// out[16 R][np] = act(in[16 R][kp] W[kp][np] + bias): wave `wave` of kPolicyWaves runs column tiles wave, wave + kPolicyWaves, ...
// kAhead > 1: the k loop runs kAhead k-blocks per trip and issues all of their weight loads before the first MFMA, so a wave has 4 kAhead
// loads in flight instead of 4 (scheduling only: every accumulator sees the same products in the same order; k-blocks that do not fill
// a trip run through the plain loop).  kAhead = 1 is the plain loop alone.  (The compiler does not unroll this loop on request: it
// reports "loop not unrolled" for the pragma below, hence the explicit form.)
template <int R, bool kRelu, int kAhead = 1>
__device__ __forceinline__ void policy_layer(const float* __restrict__ in, const int ld_in, const int kp, const float* __restrict__ W,
                                             const float* __restrict__ bias, const int np, float* __restrict__ out, const int ld_out, const int wave,
                                             const int lane) {
    const int r = lane & 15, q = lane >> 4;
    for (int n0 = wave * kTile; n0 < np; n0 += kPolicyWaves * kTile) {
        f32x4 c0[R], c1[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            c0[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            c1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* wp = W + (size_t)(4 * q) * np + n0 + r;
        const float* ap = in + r * ld_in + 4 * q;
        int k_done = 0;
        if constexpr (kAhead > 1) {
            // kAhead k-blocks per trip: all of their B fragments first, then the MFMAs in k order
            for (; k_done + kAhead * kKChunk <= kp; k_done += kAhead * kKChunk) {
                float bv[kAhead][4];
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) bv[u][s] = wp[(size_t)(u * kKChunk) * np + (size_t)s * np];
                }
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const f32x4 av = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_in + u * kKChunk);
                        c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[u][0], c0[i], 0, 0, 0);
                        c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[u][1], c1[i], 0, 0, 0);
                        c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[u][2], c0[i], 0, 0, 0);
                        c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[u][3], c1[i], 0, 0, 0);
                    }
                }
                wp += (size_t)(kAhead * kKChunk) * np;
                ap += kAhead * kKChunk;
            }
        }
        // the plain loop: every k-block (kAhead = 1), or those that did not fill a trip
#pragma unroll 2
        for (int k0 = kAhead > 1 ? k_done : 0; k0 < kp; k0 += kKChunk) {
            const float b0 = wp[0], b1 = wp[np], b2 = wp[2 * np], b3 = wp[3 * np];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_in);
                c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], b0, c0[i], 0, 0, 0);
                c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], b1, c1[i], 0, 0, 0);
                c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], b2, c0[i], 0, 0, 0);
                c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], b3, c1[i], 0, 0, 0);
            }
            wp += (size_t)kKChunk * np;
            ap += kKChunk;
        }
        const float bc = bias[n0 + r];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const f32x4 c = c0[i] + c1[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = c[j] + bc;
                if (kRelu) v = v > 0.f ? v : 0.f;
                out[(i * kTile + 4 * q + j) * ld_out + n0 + r] = v;
            }
        }
    }
}

// policy_layer's sibling for a network whose activation is a run-time fact (the dynamics ensemble, ensemble.hip): the same products in
// the same order into the same accumulators -- the kAhead form always -- and out = post(acc + bias), `post` a callable on the f32x4 a
// lane holds of one row tile (4 rows of one column; the identity for a network's last layer), so that a run-time switch over the
// activation is taken once per four values.  policy_layer itself is left as it is: the kernels built on it keep their code.
template <int R, int kAhead, class Post>
__device__ __forceinline__ void mlp_layer_post(const float* __restrict__ in, const int ld_in, const int kp, const float* __restrict__ W,
                                               const float* __restrict__ bias, const int np, float* __restrict__ out, const int ld_out, const int wave,
                                               const int lane, const Post post) {
    static_assert(kAhead > 1, "the plain loop alone is policy_layer<R, kRelu, 1>");
    const int r = lane & 15, q = lane >> 4;
    for (int n0 = wave * kTile; n0 < np; n0 += kPolicyWaves * kTile) {
        f32x4 c0[R], c1[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            c0[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            c1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* wp = W + (size_t)(4 * q) * np + n0 + r;
        const float* ap = in + r * ld_in + 4 * q;
        int k_done = 0;
        for (; k_done + kAhead * kKChunk <= kp; k_done += kAhead * kKChunk) {
            float bv[kAhead][4];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
#pragma unroll
                for (int s = 0; s < 4; ++s) bv[u][s] = wp[(size_t)(u * kKChunk) * np + (size_t)s * np];
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_in + u * kKChunk);
                    c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[u][0], c0[i], 0, 0, 0);
                    c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[u][1], c1[i], 0, 0, 0);
                    c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[u][2], c0[i], 0, 0, 0);
                    c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[u][3], c1[i], 0, 0, 0);
                }
            }
            wp += (size_t)(kAhead * kKChunk) * np;
            ap += kAhead * kKChunk;
        }
#pragma unroll 2
        for (int k0 = k_done; k0 < kp; k0 += kKChunk) {
            const float b0 = wp[0], b1 = wp[np], b2 = wp[2 * np], b3 = wp[3 * np];
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_in);
                c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], b0, c0[i], 0, 0, 0);
                c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], b1, c1[i], 0, 0, 0);
                c0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], b2, c0[i], 0, 0, 0);
                c1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], b3, c1[i], 0, 0, 0);
            }
            wp += (size_t)kKChunk * np;
            ap += kKChunk;
        }
        const float bc = bias[n0 + r];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const f32x4 c = post(c0[i] + c1[i] + f32x4{bc, bc, bc, bc});
#pragma unroll
            for (int j = 0; j < 4; ++j) out[(i * kTile + 4 * q + j) * ld_out + n0 + r] = c[j];
        }
    }
}

// nn.Linear's [N, K] -> packed[k][col0 + n] of a zeroed [Kp][np] image
__global__ void policy_pack_kernel(float* dst, const float* src, int K, int N, int np, int col0) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)K * N) return;
    const int n = (int)(i / K), k = (int)(i - (long long)n * K);
    dst[(size_t)k * np + col0 + n] = src[i];
}

inline int pad16(int x) { return (x + 15) & ~15; }

// The R rule: the largest of 4, 2, 1 row tiles whose two activation buffers (per_tile bytes per row tile) fit the opt-in LDS limit
// (more rows per workgroup = fewer passes over the weights), cut down to what the batch fills.  A row's arithmetic does not depend on R.
inline int policy_row_tiles(size_t per_tile, size_t lds_max, long long batch) {
    int R = 4;
    while (R > 1 && per_tile * R > lds_max) R >>= 1;
    while (R > 1 && (long long)kTile * (R >> 1) >= batch) R >>= 1;
    return R;
}

// Buffer A holds the input (kp0 columns), then h2; buffer B h1, then the last layer's np_last columns (the actor's heads: 2 act; the
// critic's q: one tile of 16, so ld_b = hp + 4).  per_tile: the bytes of both buffers per row tile.
struct MlpGeo { int kp0, hp, np_last, ld_a, ld_b, R; size_t per_tile, lds; };

inline MlpGeo mlp_geometry(int k0, int hidden, int last_cols, size_t lds_max, long long batch) {
    MlpGeo g{};
    g.kp0 = pad16(k0); g.hp = pad16(hidden); g.np_last = pad16(last_cols);
    g.ld_a = std::max(g.kp0, g.hp) + 4; g.ld_b = std::max(g.hp, g.np_last) + 4;
    g.per_tile = (size_t)kTile * 4 * (size_t)(g.ld_a + g.ld_b);
    g.R = policy_row_tiles(g.per_tile, lds_max, batch);
    g.lds = g.per_tile * g.R;
    return g;
}

// the body of hipets_policy_geometry / hipets_critic_geometry behind their "is one set" test (`g`: the geometry of `batch` rows)
inline int mlp_geometry_query(int32_t batch, const MlpGeo& g, int32_t* row_tiles, int32_t* lds_bytes) {
    if (batch < 1) return fail("bad batch");
    if (row_tiles) *row_tiles = g.R;
    if (lds_bytes) *lds_bytes = (int32_t)g.lds;
    return 0;
}

// One launch of a kernel family (its R = 4, 2, 1 instances) at g.R row tiles; LDS past the 64 KiB window is opted in to once per instance and device.
template <auto kK4, auto kK2, auto kK1, class Args>
hipError_t launch_mlp(const MlpGeo& g, size_t lds_max, int batch, const Args& a, hipStream_t st) {
    static LdsOptIn opted[3];
    void (*kernel)(Args) = kK1;
    LdsOptIn* once = &opted[0];
    switch (g.R) {
        case 4: kernel = kK4; once = &opted[2]; break;
        case 2: kernel = kK2; once = &opted[1]; break;
    }
    if (g.lds > 64 * 1024) {
        const hipError_t err = full_lds_once(*once, reinterpret_cast<const void*>(kernel), (int)lds_max);
        if (err != hipSuccess) return err;
    }
    const unsigned grid = (unsigned)(((long long)batch + kTile * g.R - 1) / (kTile * g.R));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPolicyThreads), g.lds, st, a);
    return hipGetLastError();
}

// A workgroup's 16 R input rows into buffer A, zero padded to kp0 columns; rows past the batch are zeros.  One source array [B, n0]
// (the actor's observations), or with kTwo a row of src0 followed by a row of src1 [B, n1] (the critic's [s, a], which exists in LDS only).
template <int R, bool kTwo>
__device__ __forceinline__ void mlp_stage_input(float* bufA, const int ld_a, const int kp0, const float* src0, const int n0, const float* src1,
                                                const int n1, const int B, const long long row0, const int tid) {
    const int K = kTwo ? n0 + n1 : n0;
    for (int t = tid; t < kTile * R * kp0; t += kPolicyThreads) {
        const int r = t / kp0, k = t - r * kp0;
        const long long row = row0 + r;
        float v = 0.f;
        if (row < B && k < K) v = (!kTwo || k < n0) ? src0[row * n0 + k] : src1[row * n1 + (k - n0)];
        bufA[r * ld_a + k] = v;
    }
}

// one nn.Linear of a packed network: weight [N, K] -> columns [col0, col0 + N) of the [Kp][np] image at W + w_off, bias [N] -> Bv + b_off
struct MlpLinear { const float *w, *b; int K, N, np, col0; size_t w_off, b_off; };

// zero the image W [nw] and the biases Bv [nb], pack the layers' weights into it, copy their biases (device to device, on `st`)
inline int mlp_pack(hipStream_t st, float* W, size_t nw, float* Bv, size_t nb, const MlpLinear* layers, int n_layers) {
    HCHECK(hipMemsetAsync(W, 0, nw * 4, st));
    HCHECK(hipMemsetAsync(Bv, 0, nb * 4, st));
    auto pack = [&](const MlpLinear& l) {
        const long long n = (long long)l.K * l.N;
        hipLaunchKernelGGL(policy_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W + l.w_off, l.w, l.K, l.N, l.np, l.col0);
    };
    for (int i = 0; i < n_layers; ++i) pack(layers[i]);
    HCHECK(hipGetLastError());
    for (int i = 0; i < n_layers; ++i) HCHECK(hipMemcpyAsync(Bv + layers[i].b_off, layers[i].b, (size_t)layers[i].N * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

// the sizes hipets_policy_set, hipets_critic_set and hipets_sac_bind accept (`who`: "policy" / "critic" / "sac")
inline int check_mlp_dims(const char* who, int obs_dim, int hidden, int act_dim) {
    if (obs_dim < 1 || obs_dim > HIPETS_POLICY_MAX_OBS) return fail("%s obs_dim %d outside [1, %d]", who, obs_dim, HIPETS_POLICY_MAX_OBS);
    if (hidden < 1 || hidden > HIPETS_POLICY_MAX_HIDDEN) return fail("%s hidden width %d outside [1, %d]", who, hidden, HIPETS_POLICY_MAX_HIDDEN);
    if (act_dim < 1 || act_dim > HIPETS_POLICY_MAX_ACT) return fail("%s act_dim %d outside [1, %d]", who, act_dim, HIPETS_POLICY_MAX_ACT);
    return 0;
}

// GaussianPolicy's LOG_SIG_MIN / LOG_SIG_MAX / epsilon (pytorch_sac_pranz24/model.py:6-8) and its torch.clamp of log_std (a NaN stays a NaN)
constexpr float kLogSigMin = -20.f, kLogSigMax = 2.f, kSacEpsilon = 1e-6f;
__device__ __forceinline__ float clamp_log_std(float ls) { return ls < kLogSigMin ? kLogSigMin : (ls > kLogSigMax ? kLogSigMax : ls); }

}  // namespace

}  // namespace hipets
