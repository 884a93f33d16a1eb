// policy_layer.hpp -- what the SAC actor kernel (policy.hip) and the SAC critic kernel (value.hip) share: one dense layer of a
// workgroup's 16 R rows on v_mfma_f32_16x16x4_f32, the packing of an nn.Linear weight into the layer's W[k][n] image, and the R rule.
// One definition, so a layer's arithmetic is the same in both kernels.  Internal linkage: each unit gets its own copy of the small
// pack kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "common.hpp"

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

}  // namespace

}  // namespace hipets
