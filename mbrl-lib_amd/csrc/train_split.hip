// train_split.hip -- the row-split training step (HIPETS_TRAIN_KERNEL_SPLIT; train_split.hpp): Model.update + torch.optim.Adam for one
// minibatch as three stream-ordered launches, so a member's step spreads over many CUs and serves minibatches of up to 1024 rows.
//   train_rows_kernel  a workgroup owns 32 rows of one member: forward with the activation panel in LDS (ping-pong over the layers),
//                      the loss tail, then dA = dZ W^T back through the pre-update weights.  It leaves A_l, Z_l and dZ_l in the slab.
//   train_dw_kernel    a workgroup owns a 64 x 64 block of one W_l: dW = A_l^T dZ_l over all rows, both panels staged through LDS in
//                      double-buffered 32-row chunks, Adam fused into the epilogue; the first row of blocks forms db as well.
//   train_split_finish_kernel  sums the loss and grad_sq partials of the step in a fixed order.
// Every product runs on v_mfma_f32_16x16x4_f32.  Operands are fetched as vectors and feed several MFMAs: a k-contiguous operand (the
// activation panel; W^T of the dA product, whose rows are contiguous along k) as one 16-byte load of k .. k + 3 per lane -- lane group q
// takes k0 + 4 q + s in MFMA s -- an n-contiguous one (W of the forward product, the dW panels) as one 8-byte load whose two values
// belong to two tiles of interleaved columns.  No float atomics, no polling: every sum has one owner and a fixed order.
// Shared with train.hip and sac.hip: the vector types and mfma4 (common.hpp), the activations and the MSE tail (train_math.hpp),
// the 64 x 64 block walk of the dW kernel (tile_walk.hpp), the host fill of the argument block (train.hpp), Adam's rule (adam.hpp).
// The k-loops, the dW kernel's fetch / stage / multiply chunk loop, the NLL tail and the Kahan sum are this file's own (DESIGN.md
// section 29).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "engine.hpp"
#include "lds_optin.hpp"
#include "tile_walk.hpp"
#include "train_math.hpp"
#include "train_split.hpp"
#include "train_wide.hpp"

namespace hipets {

namespace {

constexpr int kRowsWaves = kSplitRowsThreads / 64;
constexpr int kDwWaves = kSplitDwThreads / 64;

// One block of 16 k-steps of a 32 x 32 result block: rows 0..15 / 16..31 of the panel (pa0 / pa1: the lane's row, k-contiguous, 16-byte
// aligned) against 32 columns of B.  Lane (r, q) = (lane & 15, lane >> 4) holds k0 + 4 q + s in MFMA s, on both sides.
//   kBT  B[k][n] = W[n * K + k] (the dA product: W_l^T): tile j is columns nb0 + 16 j + r, one 16-byte load along k per tile
//  !kBT  B[k][n] = W[k * N + n] (the forward product): tile j is columns nb0 + 2 r + j, one 8-byte load of both per k
// kTail: the block may reach past K: operands at k >= K are zeros (selected, never multiplied: the panel's padding is not initialised).
template <bool kBT, bool kTail>
__device__ __forceinline__ void mm_rows_step(f32x4 (&acc)[2][2], const float* pa0, const float* pa1, const float* __restrict__ W, int K, int N,
                                             int nb0, int k0, int r, int q) {
    const int k = k0 + 4 * q, left = K - k;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 a[2];
    if (!kTail || left > 0) {  // (left > 0: k .. k + 3 lie inside the row's padded storage)
        a[0] = *reinterpret_cast<const f32x4*>(pa0 + k);
        a[1] = *reinterpret_cast<const f32x4*>(pa1 + k);
    } else {
        a[0] = a[1] = zero;
    }
    if (kTail) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s >= left) a[0][s] = a[1][s] = 0.f;
    }
    if constexpr (kBT) {
        f32x4 b[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = nb0 + 16 * j + r;
            const float* p = W + (int64_t)n * K + k;
            b[j] = zero;
            if (n < N) {
                if (!kTail || left >= 4) {
                    b[j] = *reinterpret_cast<const f32x4u*>(p);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (s < left) b[j][s] = p[s];
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[i][0] = mfma4(a[i][s], b[0][s], acc[i][0]);
                acc[i][1] = mfma4(a[i][s], b[1][s], acc[i][1]);
            }
        }
    } else {
        const int n = nb0 + 2 * r, cv = N - n;  // columns this lane may read: >= 2 both, 1 the first, <= 0 none
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float* p = W + (int64_t)(k + s) * N + n;
            f32x2 b = {0.f, 0.f};
            if (!kTail || s < left) {
                if (cv >= 2) b = *reinterpret_cast<const f32x2u*>(p);
                else if (cv == 1) b[0] = p[0];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[i][0] = mfma4(a[i][s], b[0], acc[i][0]);
                acc[i][1] = mfma4(a[i][s], b[1], acc[i][1]);
            }
        }
    }
}

// acc = panel rows 0..31 (K wide) times 32 columns of B from nb0, k in order
template <bool kBT>
__device__ __forceinline__ void mm_rows(f32x4 (&acc)[2][2], const float* pa0, const float* pa1, const float* __restrict__ W, int K, int N, int nb0,
                                        int lane) {
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    int k0 = 0;
    for (; k0 + 16 <= K; k0 += 16) mm_rows_step<kBT, false>(acc, pa0, pa1, W, K, N, nb0, k0, r, q);
    if (k0 < K) mm_rows_step<kBT, true>(acc, pa0, pa1, W, K, N, nb0, k0, r, q);
}

// Element v of acc[i][j] is row 16 i + 4 q + v of the block; its column is nb0 + 2 r + j after a forward product (interleaved tiles)
// and nb0 + 16 j + r after a dA product.

template <int kLoss>
__global__ __launch_bounds__(kSplitRowsThreads) void train_rows_kernel(const TrainSplitArgs a) {
    using acc_t = std::conditional_t<kLoss == kTrainLossMSE, double, float>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ acc_t red[kRowsWaves];
    __shared__ int32_t srow[kSplitRows];
    const int blk = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int L = a.n_layers, in = a.dims[0], out = a.out_dim, bmax = a.max_batch;
    const int nb = min(max(a.rows[0], 1), bmax), r0 = blk * kSplitRows;
    if (r0 >= nb) return;  // (the grid is sized by max_batch: the host does not know rows[s])
    const int nr = min(kSplitRows, nb - r0);
    float* slab = a.slab + (int64_t)e * a.at.stride;
    const int p1 = split_panel0_floats(in, a.dims[1]);  // where panel P1 starts
    // ---- gather the block's rows of x into P0 and the slab (an index outside the dataset reads zeros; rows past nr are zeros) ----
    if (tid < kSplitRows) {
        const int64_t row = tid < nr ? a.idx[(int64_t)e * bmax + r0 + tid] : -1;
        srow[tid] = (row >= 0 && row < a.n_rows) ? (int32_t)row : -1;
    }
    __syncthreads();
    {
        const int S = split_panel_stride(in), ld = split_ld(in);
        float* A0 = slab + a.at.off_a[0];
        for (int t = tid; t < kSplitRows * in; t += kSplitRowsThreads) {
            const int rr = t / in, k = t - rr * in;
            const float v = srow[rr] >= 0 ? a.x[(int64_t)srow[rr] * in + k] : 0.f;
            lds[rr * S + k] = v;
            if (rr < nr) A0[(int64_t)(r0 + rr) * ld + k] = v;
        }
    }
    __syncthreads();
    // ---- forward: Z_l = A_l W_l + b_l, A_{l+1} = act(Z_l); the output layer's raw columns go to the slab's dZ_{L-1} ----
    for (int l = 0; l < L; ++l) {
        const int din = a.dims[l], dout = a.dims[l + 1], ldz = split_ld(dout);
        const bool hidden = l < L - 1;
        const float* cur = lds + ((l & 1) ? p1 : 0);
        float* nxt = lds + ((l & 1) ? 0 : p1);
        const int Sc = split_panel_stride(din), Sn = split_panel_stride(dout);
        float* Zg = slab + (hidden ? a.at.off_z[l] : a.at.off_d[l]);
        float* Ag = slab + a.at.off_a[hidden ? l + 1 : 0];
        const float* W = a.w[l] + (int64_t)e * din * dout;
        const float* bias = a.b[l] + (int64_t)e * dout;
        for (int nb0 = wave * 32; nb0 < dout; nb0 += kRowsWaves * 32) {
            f32x4 acc[2][2];
            mm_rows<false>(acc, cur + r * Sc, cur + (16 + r) * Sc, W, din, dout, nb0, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = nb0 + 2 * r + j;
                if (col < dout) {
                    const float bc = bias[col];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int rr = 16 * i + 4 * q + v;
                            const float z = acc[i][j][v] + bc;
                            if (rr < nr) Zg[(int64_t)(r0 + rr) * ldz + col] = z;
                            if (hidden) {
                                const float av = act_fwd(a.activation, z, a.leaky_slope);
                                nxt[rr * Sn + col] = av;
                                if (rr < nr) Ag[(int64_t)(r0 + rr) * ldz + col] = av;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    // ---- the loss tail on the block's rows: the raw output in the slab becomes dZ_{L-1} in place ----
    const int ldo = split_ld(a.dims[L]);
    float* Dl = slab + a.at.off_d[L - 1];
    acc_t lsum = 0;
    if constexpr (kLoss == kTrainLossMSE) {
        for (int t = tid; t < nr * out; t += kSplitRowsThreads) {
            const int rr = t / out, j = t - rr * out;
            float* o = Dl + (int64_t)(r0 + rr) * ldo;
            const float tv = srow[rr] >= 0 ? a.y[(int64_t)srow[rr] * out + j] : 0.f;
            mse_tail(o[j], tv, a.grad_scale, lsum, o[j]);
        }
    } else {
        // train_step_kernel's NLL tail (train.hip), operation for operation (train_math.hpp: why not a function)
        const float scale = 1.f / (float)(nb * out) * a.grad_scale;  // the mean runs over ALL rows of the step, not the block's
        const float* mxv = a.max_logvar + (int64_t)e * a.bounds_stride;
        const float* mnv = a.min_logvar + (int64_t)e * a.bounds_stride;
        for (int t = tid; t < nr * out; t += kSplitRowsThreads) {
            const int rr = t / out, j = t - rr * out;
            float* o = Dl + (int64_t)(r0 + rr) * ldo;
            const float tv = srow[rr] >= 0 ? a.y[(int64_t)srow[rr] * out + j] : 0.f;
            const float mean = o[j], raw = o[out + j];
            const float mx = mxv[j], mn = mnv[j];
            const float u = mx - raw;
            const float lv1 = mx - softplus(u);
            const float w = lv1 - mn;
            const float lv = mn + softplus(w);
            const float d = mean - tv;
            const float iv = expf(-lv);
            const float l2iv = d * d * iv;
            lsum += l2iv + lv;
            o[j] = 2.f * d * (scale * iv);
            const float dlv = scale - scale * l2iv;
            o[out + j] = dlv * softplus_grad(w) * softplus_grad(u);
        }
    }
    lsum = wave_sum(lsum);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();  // (and: every dZ_{L-1} of the block is in the slab)
    if (tid == 0) {
        acc_t ls = 0;
        for (int w = 0; w < kRowsWaves; ++w) ls += red[w];
        a.loss_part[(int64_t)e * a.row_blocks + blk] = (double)ls;
    }
    // ---- backward: dZ_{l-1} = (dZ_l W_l^T) * act'(Z_{l-1}), the weights as the forward pass saw them.  The output layer's dZ (up to
    // 2 x 512 columns) is read from the slab, rows past nr clamped to the last one; the narrower ones ping-pong through the panels ----
    for (int l = L - 1; l >= 1; --l) {
        const int din = a.dims[l], dout = a.dims[l + 1], ldn = split_ld(din);
        const float* src = lds + ((l & 1) ? p1 : 0);
        float* dst = lds + ((l & 1) ? 0 : p1);
        const int Ss = split_panel_stride(dout), Sd = split_panel_stride(din);
        const float* W = a.w[l] + (int64_t)e * din * dout;
        const float* Zp = slab + a.at.off_z[l - 1];
        float* Dn = slab + a.at.off_d[l - 1];
        for (int nb0 = wave * 32; nb0 < din; nb0 += kRowsWaves * 32) {
            f32x4 acc[2][2];
            if (l == L - 1)  // (two call sites: one reads its panel from global memory, the other from LDS)
                mm_rows<true>(acc, Dl + (int64_t)(r0 + min(r, nr - 1)) * ldo, Dl + (int64_t)(r0 + min(16 + r, nr - 1)) * ldo, W, dout, din, nb0, lane);
            else
                mm_rows<true>(acc, src + r * Ss, src + (16 + r) * Ss, W, dout, din, nb0, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = nb0 + 16 * j + r;
                if (col < din) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int rr = 16 * i + 4 * q + v;
                            const float g = acc[i][j][v] * act_grad(a.activation, Zp[(int64_t)(r0 + min(rr, nr - 1)) * ldn + col], a.leaky_slope);
                            dst[rr * Sd + col] = g;
                            if (rr < nr) Dn[(int64_t)(r0 + rr) * ldn + col] = g;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// a float4 of a slab row at column `col` (a multiple of 4), zeros at and past `width` and for a row that is not there
__device__ __forceinline__ f32x4 slab_quad(const float* __restrict__ row, int col, int width, bool there) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (there && col < width) {  // (col + 3 < split_ld(width): inside the row's padded storage)
        v = *reinterpret_cast<const f32x4*>(row + col);
#pragma unroll
        for (int s = 1; s < 4; ++s)
            if (col + s >= width) v[s] = 0.f;
    }
    return v;
}

template <int kLoss>
__global__ __launch_bounds__(kSplitDwThreads) void train_dw_kernel(const TrainSplitArgs a) {
    using acc_t = std::conditional_t<kLoss == kTrainLossMSE, double, float>;
    constexpr int S = kSplitDwStride, KC = kSplitDwChunk;
    __shared__ __attribute__((aligned(16))) float sA[2][KC * S];
    __shared__ __attribute__((aligned(16))) float sD[2][KC * S];
    __shared__ acc_t red[kDwWaves];
    const int l = blockIdx.y, e = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int din = a.dims[l], dout = a.dims[l + 1];
    if ((int)blockIdx.x >= split_dw_blocks(din, dout)) return;  // (the grid's x extent is the widest layer's)
    const unsigned bn = blocks_across(dout);
    const int i0 = block_m0(blockIdx.x, bn), j0 = block_n0(blockIdx.x, bn);
    const int nb = min(max(a.rows[0], 1), a.max_batch);
    const float* slab = a.slab + (int64_t)e * a.at.stride;
    const float* Ag = slab + a.at.off_a[l];
    const float* Dg = slab + a.at.off_d[l];
    const int lda = split_ld(din), ldd = split_ld(dout);
    const int iw = block_wave_m0(wave), jw = block_wave_n0(wave);  // the wave's 32 x 32 block of the 64 x 64
    const int c4 = (tid & 15) * 4, sr = tid >> 4;                // staging: this thread's float4 column and its two rows sr, sr + 16
    const bool bias_col = i0 == 0 && tid < kBlock && j0 + tid < dout;  // this thread sums column j0 + tid of dZ for db
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gb = 0.f, comp = 0.f;
    f32x4 fa[2], fd[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = k0 + sr + 16 * h;
            fa[h] = slab_quad(Ag + (int64_t)row * lda, i0 + c4, din, row < nb);
            fd[h] = slab_quad(Dg + (int64_t)row * ldd, j0 + c4, dout, row < nb);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<f32x4*>(&sA[buf][(sr + 16 * h) * S + c4]) = fa[h];
            *reinterpret_cast<f32x4*>(&sD[buf][(sr + 16 * h) * S + c4]) = fd[h];
        }
    };
    fetch(0);
    stage(0);
    __syncthreads();
    for (int k0 = 0, buf = 0; k0 < nb; k0 += KC, buf ^= 1) {
        const bool more = k0 + KC < nb;
        if (more) fetch(k0 + KC);  // the next chunk travels while this one is multiplied
        const float* pA = sA[buf] + q * S + iw + 2 * r;
        const float* pD = sD[buf] + q * S + jw + 2 * r;
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            const f32x2 av = *reinterpret_cast<const f32x2*>(pA + kk * S);  // rows iw + 2 r, + 1 of the block: one for each row tile
            const f32x2 dv = *reinterpret_cast<const f32x2*>(pD + kk * S);
            acc[0][0] = mfma4(av[0], dv[0], acc[0][0]);
            acc[0][1] = mfma4(av[0], dv[1], acc[0][1]);
            acc[1][0] = mfma4(av[1], dv[0], acc[1][0]);
            acc[1][1] = mfma4(av[1], dv[1], acc[1][1]);
        }
        if (bias_col) {
            // db: the rows in order; under MSE compensated (Kahan), as train_step_kernel sums them
            const int kn = min(KC, nb - k0);
            for (int k = 0; k < kn; ++k) {
                const float dz = sD[buf][k * S + tid];
                if constexpr (kLoss == kTrainLossMSE) {
                    const float yk = dz - comp;
                    const float tk = gb + yk;
                    comp = (tk - gb) - yk;
                    gb = tk;
                } else {
                    gb += dz;
                }
            }
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
    }
    // ---- Adam on the block: element v of acc[ti][tj] is dW[i0 + iw + 2 (4 q + v) + ti][j0 + jw + 2 r + tj] ----
    acc_t gsq = 0;
    const int64_t wo = (int64_t)e * din * dout;
    float* W = a.w[l] + wo;
    float* mW = a.mw[l] + wo;
    float* vW = a.vw[l] + wo;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int col = j0 + jw + 2 * r + tj;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = i0 + iw + 2 * (4 * q + v) + ti;
                if (row < din && col < dout) {
                    const int64_t o = (int64_t)row * dout + col;
                    const float g = acc[ti][tj][v];
                    gsq += (acc_t)g * (acc_t)g;
                    const float p = W[o];
                    W[o] = adam_update(p, g + a.weight_decay * p, mW + o, vW + o, a.adam);  // (coupled weight decay)
                }
            }
        }
    }
    if (bias_col) {
        const int64_t o = (int64_t)e * dout + j0 + tid;
        gsq += (acc_t)gb * (acc_t)gb;
        const float p = a.b[l][o];
        a.b[l][o] = adam_update(p, gb + a.weight_decay * p, a.mb[l] + o, a.vb[l] + o, a.adam);
    }
    gsq = wave_sum(gsq);
    if (lane == 0) red[wave] = gsq;
    __syncthreads();
    if (tid == 0) {
        acc_t gs = 0;
        for (int w = 0; w < kDwWaves; ++w) gs += red[w];
        a.gsq_part[((int64_t)e * a.n_layers + l) * a.dw_blocks + blockIdx.x] = (double)gs;
    }
}

// loss[e] and grad_sq[e] of the step: one wave per member, lane t sums partials t, t + 64, ... in order, then a fixed tree
template <int kLoss>
__global__ __launch_bounds__(64) void train_split_finish_kernel(const TrainSplitArgs a) {
    const int e = blockIdx.x, lane = threadIdx.x;
    const int nb = min(max(a.rows[0], 1), a.max_batch), blocks = (nb + kSplitRows - 1) / kSplitRows;
    double ls = 0.0, gs = 0.0;
    for (int b = lane; b < blocks; b += 64) ls += a.loss_part[(int64_t)e * a.row_blocks + b];
    for (int l = 0; l < a.n_layers; ++l) {
        const int cnt = split_dw_blocks(a.dims[l], a.dims[l + 1]);
        for (int b = lane; b < cnt; b += 64) gs += a.gsq_part[((int64_t)e * a.n_layers + l) * a.dw_blocks + b];
    }
    ls = wave_sum(ls);
    gs = wave_sum(gs);
    if (lane == 0) {
        a.loss[e] = kLoss == kTrainLossMSE ? (float)ls : (float)ls / (float)(nb * a.out_dim);
        a.grad_sq[e] = (float)gs;
    }
}

// wide: the rows kernel is train_wide.hip's (one in-place panel, hidden widths up to 1024); the other two launches are the same
template <int kLoss>
hipError_t launch_split_step(const TrainSplitArgs& a, hipStream_t st, bool wide) {
    static LdsOptIn once;
    hipError_t err;
    if (wide) {
        if ((err = launch_train_wide_rows(a, kLoss, st)) != hipSuccess) return err;
    } else {
        err = full_lds_once(once, reinterpret_cast<const void*>(&train_rows_kernel<kLoss>), split_rows_lds_bytes(kTrainMaxIn, kTrainMaxHid));
        if (err != hipSuccess) return err;
        const size_t lds = (size_t)split_rows_lds_bytes(a.dims[0], a.dims[1]);
        hipLaunchKernelGGL(train_rows_kernel<kLoss>, dim3(a.row_blocks, a.ensemble_size), dim3(kSplitRowsThreads), lds, st, a);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    hipLaunchKernelGGL(train_dw_kernel<kLoss>, dim3(a.dw_blocks, a.n_layers, a.ensemble_size), dim3(kSplitDwThreads), 0, st, a);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(train_split_finish_kernel<kLoss>, dim3(a.ensemble_size), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace

int train_split_steps(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows, const int32_t* idx,
                      const int32_t* rows, int32_t n_steps, int64_t step0, float* loss, float* grad_sq, hipStream_t st, int32_t loss_kind,
                      int32_t bounds_per_member, float grad_scale, bool wide) {
    TrainSplitArgs a{};
    const int L = d->n_layers, E = d->ensemble_size, Bm = d->max_batch;
    train_fill(a, d, loss_kind, x, y, n_rows);
    train_fill_step(a, d, bounds_per_member, grad_scale);
    a.at = train_split_slab(a.dims, L, Bm);
    a.row_blocks = (Bm + kSplitRows - 1) / kSplitRows;
    for (int l = 0; l < L; ++l) a.dw_blocks = std::max(a.dw_blocks, split_dw_blocks(a.dims[l], a.dims[l + 1]));
    if (e->train_slab.ensure((size_t)E * a.at.stride * sizeof(float))) return 1;
    if (e->train_split_part.ensure((size_t)E * (a.row_blocks + (size_t)L * a.dw_blocks) * sizeof(double))) return 1;
    a.slab = e->train_slab.as<float>();
    a.loss_part = e->train_split_part.as<double>();
    a.gsq_part = a.loss_part + (size_t)E * a.row_blocks;
    for (int s = 0; s < n_steps; ++s) {
        a.adam = adam_scalars(d->lr, d->beta1, d->beta2, d->eps, step0 + s + 1);
        a.idx = idx + (int64_t)s * E * Bm;
        a.rows = rows + s;
        a.loss = loss + (int64_t)s * E;
        a.grad_sq = grad_sq + (int64_t)s * E;
        const hipError_t err = loss_kind == kTrainLossMSE ? launch_split_step<kTrainLossMSE>(a, st, wide) : launch_split_step<kTrainLossNLL>(a, st, wide);
        if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "%s train step launch failed: %s", wide ? "wide" : "split", hipGetErrorString(err));
    }
    return 0;
}

}  // namespace hipets
