// train_wide.hip -- the wide training step's rows kernel and the wide evaluate kernel (train_wide.hpp; HIPETS_TRAIN_WIDTH_WIDE): hidden
// widths up to 1024 on ONE activation panel of 32 rows in LDS.
// A layer's product is not written where it is read.  Its whole 32 x dout result (dout up to 1024) stays in the accumulators of the
// eight waves -- a wave owns up to kT column tiles of both row tiles, 8 kT registers -- while the k loop reads the panel; behind a
// barrier the waves overwrite the panel from their registers (bias and activation applied on the way, the slab's copies stored from
// the same registers), and the next layer reads it.  The dA chain runs back over the same panel the same way.
// Operand fetch, per lane (r, q) = (lane & 15, lane >> 4) and block of 16 k (MFMA s of the block sums k0 + 4 q + s over q):
//   A (the panel, k-contiguous)        one 16-byte LDS read per row tile: k0 + 4 q .. + 3 of row r / 16 + r, for the four tiles of a pass
//                                      (a wave's tiles run in passes of four: all of them up to 512 columns, two passes up to 1024)
//   B forward (W[k][n], n-contiguous)  per k one 16-byte load of columns nb0 + 4 r .. + 3: the values of FOUR interleaved column tiles
//                                      (tile j = columns nb0 + 4 r + j), so 16 lanes read 256 contiguous bytes of a row of W
//   B backward (W[n][k], k-contiguous) per tile one 16-byte load of k0 + 4 q .. + 3 of row nb0 + r, as train_rows_kernel reads it
// Every fragment feeds both row tiles.  The loads of block k0 + 16 are issued ahead of the MFMAs of block k0.  An operand past K, past N
// or in a row past the block's nr rows is a selected zero, never a product with whatever the panel holds there.
// Every result element is summed in one accumulator, k ascending in blocks of 16, whatever the batch size, the row block, the grid, the
// instance (kT) or the cut of a run into calls: the order is the layer's shape's alone.
// The loss tails and the loss partial are train_rows_kernel's (train_split.hip), read from and written to the panel; dW, Adam and the
// step's sums are train_split.hip's kernels, unchanged.  DESIGN.md section 34.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "lds_optin.hpp"
#include "train_math.hpp"
#include "train_wide.hpp"

namespace hipets {

namespace {

// A wave's columns are units dealt round robin over the waves -- forward a group of four interleaved tiles (64 columns), backward one tile
// (16) -- and a product runs over them in passes of four tiles: forward pass h is the wave's unit h, backward pass h its units 4 h .. 4 h + 3.
// (One pass at a time keeps two sets of operands in flight beside ALL of the wave's accumulators; eight tiles' operands at once spilt.)
__device__ __forceinline__ int wide_unit(int wave, int i) { return wave + kWideWaves * i; }

// the operands of one block of 16 k of a pass: forward b[s] = the four interleaved tiles' values (components) at k-step s; backward
// b[j] = k-steps 0 .. 3 (components) of tile j of the pass
struct WideFrag {
    f32x4 a[2];
    f32x4 b[4];
};

// kTail: the block may reach past K
template <bool kBT, bool kTail>
__device__ __forceinline__ void wide_fetch(WideFrag& f, const float* pa0, const float* pa1, bool row0, bool row1, const float* __restrict__ W, int K,
                                           int N, int ldw, int k0, int h, int wave, int r, int q) {
    const int k = k0 + 4 * q, left = K - k;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f.a[0] = f.a[1] = zero;
    if (!kTail || left > 0) {  // (left > 0: k .. k + 3 lie inside the row's padded storage)
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(pa0 + k), v1 = *reinterpret_cast<const f32x4*>(pa1 + k);
        f.a[0] = row0 ? v0 : zero;
        f.a[1] = row1 ? v1 : zero;
    }
    if (kTail) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (s >= left) f.a[0][s] = f.a[1][s] = 0.f;
    }
    if constexpr (kBT) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 16 * wide_unit(wave, 4 * h + j) + r;
            f.b[j] = zero;
            if (n < N) {  // (a whole tile past N: no lane loads)
                const float* p = W + (int64_t)n * K + k;
                if (!kTail || left >= 4) {
                    f.b[j] = *reinterpret_cast<const f32x4u*>(p);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (s < left) f.b[j][s] = p[s];
                }
            }
        }
    } else {
        const int n = 64 * wide_unit(wave, h) + 4 * r, cv = N - n;  // columns this lane may read: >= 4 all, 1 .. 3 the first, <= 0 none
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            f.b[s] = zero;
            if (cv > 0 && (!kTail || s < left)) {
                const float* p = W + (int64_t)(k + s) * ldw + n;
                if (cv >= 4) {
                    f.b[s] = *reinterpret_cast<const f32x4u*>(p);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (c < cv) f.b[s][c] = p[c];
                }
            }
        }
    }
}

// the MFMAs of one block of 16 k of pass kH; the guards are whole tiles: wave-uniform
template <bool kBT, int kT, int kH>
__device__ __forceinline__ void wide_mul(f32x4 (&acc)[2][kT], const WideFrag& f, int N, int wave) {
    if constexpr (kBT) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (16 * wide_unit(wave, 4 * kH + j) < N) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    acc[0][4 * kH + j] = mfma4(f.a[0][s], f.b[j][s], acc[0][4 * kH + j]);
                    acc[1][4 * kH + j] = mfma4(f.a[1][s], f.b[j][s], acc[1][4 * kH + j]);
                }
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][4 * kH + j] = mfma4(f.a[0][s], f.b[s][j], acc[0][4 * kH + j]);
                acc[1][4 * kH + j] = mfma4(f.a[1][s], f.b[s][j], acc[1][4 * kH + j]);
            }
        }
    }
}

// pass kH of a product: the k loop, the loads of block k0 + 16 issued ahead of the MFMAs of block k0
template <bool kBT, int kT, int kH>
__device__ __forceinline__ void wide_pass(f32x4 (&acc)[2][kT], const float* pa0, const float* pa1, bool row0, bool row1, const float* __restrict__ W,
                                          int K, int N, int ldw, int wave, int r, int q) {
    if ((kBT ? 16 * wide_unit(wave, 4 * kH) : 64 * wide_unit(wave, kH)) >= N) return;  // the wave owns no column of this pass
    WideFrag cur, nxt;
    if (K >= 16) wide_fetch<kBT, false>(cur, pa0, pa1, row0, row1, W, K, N, ldw, 0, kH, wave, r, q);
    else wide_fetch<kBT, true>(cur, pa0, pa1, row0, row1, W, K, N, ldw, 0, kH, wave, r, q);
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kn = k0 + 16;
        if (kn + 16 <= K) wide_fetch<kBT, false>(nxt, pa0, pa1, row0, row1, W, K, N, ldw, kn, kH, wave, r, q);
        else if (kn < K) wide_fetch<kBT, true>(nxt, pa0, pa1, row0, row1, W, K, N, ldw, kn, kH, wave, r, q);
        wide_mul<kBT, kT, kH>(acc, cur, N, wave);
        if (kn < K) cur = nxt;
    }
}

// acc = the panel's 32 rows (K wide, stride S; rows past nr count as zeros) times the wave's columns of B, k in order:
//   kBT  B[k][n] = W[n * K + k] (the dA product: W_l^T), N columns
//  !kBT  B[k][n] = W[k * ldw + n] (the forward product), the first N columns of a row of W
// Element v of acc[i][t] is row 16 i + 4 q + v; its column is 64 unit(t / 4) + 4 r + t % 4 forward and 16 unit(t) + r backward.
template <bool kBT, int kT>
__device__ __forceinline__ void wide_mm(f32x4 (&acc)[2][kT], const float* panel, int S, int nr, const float* __restrict__ W, int K, int N, int ldw,
                                        int wave, int lane) {
    static_assert(kT == 4 || kT == 8, "one or two passes of four tiles");
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int t = 0; t < kT; ++t) acc[0][t] = acc[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *pa0 = panel + r * S, *pa1 = panel + (16 + r) * S;
    const bool row0 = r < nr, row1 = 16 + r < nr;
    wide_pass<kBT, kT, 0>(acc, pa0, pa1, row0, row1, W, K, N, ldw, wave, r, q);
    if constexpr (kT == 8) wide_pass<kBT, kT, 1>(acc, pa0, pa1, row0, row1, W, K, N, ldw, wave, r, q);
}

// a forward result from the registers: f(row of the block, first of four adjacent columns, their values with the bias added); columns
// at and past N carry zeros plus a zero bias (col + 3 lies inside a row's padded storage, in the panel and in the slab)
template <int kT, class F>
__device__ __forceinline__ void wide_forward_out(const f32x4 (&acc)[2][kT], const float* __restrict__ bias, int N, int wave, int lane, F&& f) {
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int g = 0; g < kT / 4; ++g) {
        const int col = 64 * wide_unit(wave, g) + 4 * r;
        if (col < N) {
            f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (col + j < N) b4[j] = bias[col + j];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    f32x4 z;
#pragma unroll
                    for (int j = 0; j < 4; ++j) z[j] = acc[i][4 * g + j][v] + b4[j];
                    f(16 * i + 4 * q + v, col, z);
                }
            }
        }
    }
}

// one hidden layer of the forward chain, in place on the panel: A_{l+1} = act(A_l W + b).  kept(row, col, z, av) sees every four
// columns of the block's rows on their way (the step stores them to the slab; the evaluate pass keeps nothing).
template <int kT, class F>
__device__ __forceinline__ void wide_hidden_layer(float* panel, int S, int nr, const float* __restrict__ W, const float* __restrict__ bias, int din,
                                                  int dout, int activation, float slope, int wave, int lane, F&& kept) {
    f32x4 acc[2][kT];
    wide_mm<false, kT>(acc, panel, S, nr, W, din, dout, dout, wave, lane);
    __syncthreads();  // every wave has read A_l for the last time
    wide_forward_out<kT>(acc, bias, dout, wave, lane, [&](int rr, int col, f32x4 z) {
        f32x4 av;
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = act_fwd(activation, z[j], slope);
        *reinterpret_cast<f32x4*>(panel + rr * S + col) = av;
        if (rr < nr) kept(rr, col, z, av);
    });
    __syncthreads();
}

template <int kLoss, int kT>
__global__ __launch_bounds__(kWideThreads) void train_wide_rows_kernel(const TrainSplitArgs a) {
    using acc_t = std::conditional_t<kLoss == kTrainLossMSE, double, float>;
    extern __shared__ __attribute__((aligned(16))) float panel[];
    __shared__ acc_t red[kWideWaves];
    __shared__ int32_t srow[kSplitRows];
    const int blk = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int L = a.n_layers, in = a.dims[0], out = a.out_dim, bmax = a.max_batch;
    const int nb = min(max(a.rows[0], 1), bmax), r0 = blk * kSplitRows;
    if (r0 >= nb) return;  // (the grid is sized by max_batch: the host does not know rows[s])
    const int nr = min(kSplitRows, nb - r0);
    float* slab = a.slab + (int64_t)e * a.at.stride;
    int widest = 0;
    for (int l = 0; l <= L; ++l) widest = max(widest, a.dims[l]);
    const int S = split_panel_stride(widest);  // one stride for every layer: a row stays where it is
    // ---- gather the block's rows of x into the panel and the slab (an index outside the dataset reads zeros) ----
    if (tid < kSplitRows) {
        const int64_t row = tid < nr ? a.idx[(int64_t)e * bmax + r0 + tid] : -1;
        srow[tid] = (row >= 0 && row < a.n_rows) ? (int32_t)row : -1;
    }
    __syncthreads();
    {
        const int ld = split_ld(in);
        float* A0 = slab + a.at.off_a[0];
        for (int t = tid; t < nr * in; t += kWideThreads) {
            const int rr = t / in, k = t - rr * in;
            const float v = srow[rr] >= 0 ? a.x[(int64_t)srow[rr] * in + k] : 0.f;
            panel[rr * S + k] = v;
            A0[(int64_t)(r0 + rr) * ld + k] = v;
        }
    }
    __syncthreads();
    // ---- forward: Z_l = A_l W_l + b_l, A_{l+1} = act(Z_l), both to the slab; the output layer's raw columns stay in the panel ----
    for (int l = 0; l < L - 1; ++l) {
        const int din = a.dims[l], dout = a.dims[l + 1], ldz = split_ld(dout);
        float* Zg = slab + a.at.off_z[l] + (int64_t)r0 * ldz;
        float* Ag = slab + a.at.off_a[l + 1] + (int64_t)r0 * ldz;
        wide_hidden_layer<kT>(panel, S, nr, a.w[l] + (int64_t)e * din * dout, a.b[l] + (int64_t)e * dout, din, dout, a.activation, a.leaky_slope, wave,
                              lane, [&](int rr, int col, f32x4 z, f32x4 av) {
                                  *reinterpret_cast<f32x4*>(Zg + (int64_t)rr * ldz + col) = z;
                                  *reinterpret_cast<f32x4*>(Ag + (int64_t)rr * ldz + col) = av;
                              });
    }
    const int dlast = a.dims[L - 1], dcols = a.dims[L], ldo = split_ld(dcols);
    {
        f32x4 acc[2][kT];
        wide_mm<false, kT>(acc, panel, S, nr, a.w[L - 1] + (int64_t)e * dlast * dcols, dlast, dcols, dcols, wave, lane);
        __syncthreads();
        wide_forward_out<kT>(acc, a.b[L - 1] + (int64_t)e * dcols, dcols, wave, lane,
                             [&](int rr, int col, f32x4 z) { *reinterpret_cast<f32x4*>(panel + rr * S + col) = z; });
        __syncthreads();
    }
    // ---- the loss tail on the block's rows: the raw output in the panel becomes dZ_{L-1}, in the panel and in the slab ----
    float* Dl = slab + a.at.off_d[L - 1] + (int64_t)r0 * ldo;
    acc_t lsum = 0;
    if constexpr (kLoss == kTrainLossMSE) {
        for (int t = tid; t < nr * out; t += kWideThreads) {
            const int rr = t / out, j = t - rr * out;
            float* o = panel + rr * S;
            const float tv = srow[rr] >= 0 ? a.y[(int64_t)srow[rr] * out + j] : 0.f;
            mse_tail(o[j], tv, a.grad_scale, lsum, o[j]);
            Dl[(int64_t)rr * ldo + j] = o[j];
        }
    } else {
        // train_rows_kernel's NLL tail (train_split.hip), operation for operation (train_math.hpp: why not a function)
        const float scale = 1.f / (float)(nb * out) * a.grad_scale;  // the mean runs over ALL rows of the step, not the block's
        const float* mxv = a.max_logvar + (int64_t)e * a.bounds_stride;
        const float* mnv = a.min_logvar + (int64_t)e * a.bounds_stride;
        for (int t = tid; t < nr * out; t += kWideThreads) {
            const int rr = t / out, j = t - rr * out;
            float* o = panel + rr * S;
            float* og = Dl + (int64_t)rr * ldo;
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
            og[j] = o[j] = 2.f * d * (scale * iv);
            const float dlv = scale - scale * l2iv;
            og[out + j] = o[out + j] = dlv * softplus_grad(w) * softplus_grad(u);
        }
    }
    lsum = wave_sum(lsum);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();  // (and: every dZ_{L-1} of the block is in the panel)
    if (tid == 0) {
        acc_t ls = 0;
        for (int w = 0; w < kWideWaves; ++w) ls += red[w];
        a.loss_part[(int64_t)e * a.row_blocks + blk] = (double)ls;
    }
    // ---- backward: dZ_{l-1} = (dZ_l W_l^T) * act'(Z_{l-1}), the weights as the forward pass saw them, in place on the panel; the last
    // product (dZ_0) goes to the slab only ----
    for (int l = L - 1; l >= 1; --l) {
        const int din = a.dims[l], dout = a.dims[l + 1], ldn = split_ld(din);
        const float* Zp = slab + a.at.off_z[l - 1] + (int64_t)r0 * ldn;
        float* Dn = slab + a.at.off_d[l - 1] + (int64_t)r0 * ldn;
        f32x4 acc[2][kT];
        wide_mm<true, kT>(acc, panel, S, nr, a.w[l] + (int64_t)e * din * dout, dout, din, 0, wave, lane);
        if (l > 1) __syncthreads();  // every wave has read dZ_l for the last time
#pragma unroll
        for (int j = 0; j < kT; ++j) {
            const int col = 16 * wide_unit(wave, j) + r;
            if (col < din) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int rr = 16 * i + 4 * q + v;
                        if (rr < nr) {
                            const float g = acc[i][j][v] * act_grad(a.activation, Zp[(int64_t)rr * ldn + col], a.leaky_slope);
                            if (l > 1) panel[rr * S + col] = g;
                            Dn[(int64_t)rr * ldn + col] = g;
                        }
                    }
                }
            }
        }
        if (l > 1) __syncthreads();
    }
}

// evaluate: workgroup (tile, member) runs kEvalRows rows through the member on the same forward chain; the output layer computes its
// first out_dim (mean) columns only.  The tail is train_eval_kernel's (train.hip): squared errors into the panel, per-row sums (dims in
// order; compensated here), the tile's sum to partial[e, tile] (rows in order, one thread).
template <int kT>
__global__ __launch_bounds__(kWideThreads) void train_wide_eval_kernel(const TrainEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float panel[];
    __shared__ int64_t rows[kEvalRows];
    __shared__ float rsum[kEvalRows];
    const int tile = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.n_layers, in = a.dims[0], out = a.out_dim, S = split_panel_stride(a.max_width);
    const int64_t r0 = (int64_t)tile * kEvalRows;
    const int nr = (int)min((int64_t)kEvalRows, a.n_rows - r0);
    if (tid < nr) {
        const int64_t row = a.order ? (int64_t)a.order[r0 + tid] : r0 + tid;
        rows[tid] = (row >= 0 && row < a.n_rows) ? row : -1;
    }
    __syncthreads();
    for (int t = tid; t < nr * in; t += kWideThreads) {
        const int rr = t / in, k = t - rr * in;
        panel[rr * S + k] = rows[rr] >= 0 ? a.x[rows[rr] * in + k] : 0.f;
    }
    __syncthreads();
    for (int l = 0; l < L - 1; ++l) {
        const int din = a.dims[l], dout = a.dims[l + 1];
        wide_hidden_layer<kT>(panel, S, nr, a.w[l] + (int64_t)e * din * dout, a.b[l] + (int64_t)e * dout, din, dout, a.activation, a.leaky_slope, wave,
                              lane, [](int, int, f32x4, f32x4) {});
    }
    {
        const int din = a.dims[L - 1], ld = a.dims[L];
        f32x4 acc[2][kT];
        wide_mm<false, kT>(acc, panel, S, nr, a.w[L - 1] + (int64_t)e * din * ld, din, out, ld, wave, lane);
        __syncthreads();
        wide_forward_out<kT>(acc, a.b[L - 1] + (int64_t)e * ld, out, wave, lane, [&](int rr, int col, f32x4 z) {
            if (rr < nr) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (col + j < out) {
                        const float d = rows[rr] >= 0 ? z[j] - a.y[rows[rr] * out + col + j] : 0.f;
                        panel[rr * S + col + j] = d * d;
                    }
                }
            }
        });
        __syncthreads();
    }
    if (tid < nr) {
        // dims in order, as train_eval_kernel sums them, but compensated (Kahan; train_dw_kernel's db under MSE is the same sum): a plain
        // float32 sum of 512 squared errors drifts further from the float64 value than the trainer tests' rule allows
        float s = 0.f, comp = 0.f;
        for (int j = 0; j < out; ++j) {
            const float yk = panel[tid * S + j] - comp;
            const float tk = s + yk;
            comp = (tk - s) - yk;
            s = tk;
        }
        rsum[tid] = s;
        if (a.row_score) a.row_score[(int64_t)e * a.n_rows + r0 + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int rr = 0; rr < nr; ++rr) s += rsum[rr];
        a.partial[(int64_t)e * a.tiles + tile] = s;
    }
}

// one kernel instance at `lds` bytes of dynamic LDS, opted in to the widest panel once per device
template <class Args>
hipError_t launch_wide(void (*kernel)(const Args), LdsOptIn& once, dim3 grid, int lds, const Args& a, hipStream_t st) {
    const hipError_t err = full_lds_once(once, reinterpret_cast<const void*>(kernel), wide_lds_bytes(kTrainWideMaxHid));
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kernel, grid, dim3(kWideThreads), (size_t)lds, st, a);
    return hipGetLastError();
}

template <int kLoss, int kT>
hipError_t launch_rows(const TrainSplitArgs& a, int lds, hipStream_t st) {
    static LdsOptIn once;
    return launch_wide(&train_wide_rows_kernel<kLoss, kT>, once, dim3(a.row_blocks, a.ensemble_size), lds, a, st);
}

template <int kT>
hipError_t launch_eval(const TrainEvalArgs& a, int lds, hipStream_t st) {
    static LdsOptIn once;
    return launch_wide(&train_wide_eval_kernel<kT>, once, dim3(a.tiles, a.ensemble_size), lds, a, st);
}

}  // namespace

// The instance: by the widest RESULT of the call's layers (forward: d_1 .. d_L; the dA chain's are among them).
hipError_t launch_train_wide_rows(const TrainSplitArgs& a, int loss_kind, hipStream_t st) {
    int widest = a.dims[0], result = 0;
    for (int l = 1; l <= a.n_layers; ++l) result = std::max(result, (int)a.dims[l]);
    widest = std::max(widest, result);
    const int lds = wide_lds_bytes(widest);
    const bool full = result > wide_columns(kWideTilesNarrow);
    if (loss_kind == kTrainLossMSE)
        return full ? launch_rows<kTrainLossMSE, kWideTilesFull>(a, lds, st) : launch_rows<kTrainLossMSE, kWideTilesNarrow>(a, lds, st);
    return full ? launch_rows<kTrainLossNLL, kWideTilesFull>(a, lds, st) : launch_rows<kTrainLossNLL, kWideTilesNarrow>(a, lds, st);
}

// (the output layer's result is its out_dim mean columns: max_width = max(in, hid, out_dim) holds every panel of the pass)
hipError_t launch_train_wide_eval(const TrainEvalArgs& a, hipStream_t st) {
    const int result = std::max((int)a.dims[1], (int)a.out_dim), lds = wide_lds_bytes(a.max_width);
    return result > wide_columns(kWideTilesNarrow) ? launch_eval<kWideTilesFull>(a, lds, st) : launch_eval<kWideTilesNarrow>(a, lds, st);
}

}  // namespace hipets
