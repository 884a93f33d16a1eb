// train.hip -- GaussianMLP ensemble training (hipets_train_steps[_loss] / hipets_train_eval[_loss], include/hipets.h): the kernels, then the
// entry points.
//   train_step_kernel  Model.update (mbrl/models/model.py:129-167) + torch.optim.Adam for a chunk of consecutive minibatches, one
//                      instantiation per loss kind (NLL, MSE); a BasicEnsemble is per-member bounds and grad_scale = 1 / E
//   train_eval_kernel  GaussianMLP.eval_score over the whole evaluation set (gaussian_mlp.py:337-361), mean columns only
// Every product runs on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulate): mm_tile is the k-loop, tile_walk.hpp the tiles'
// numbering and the lane-to-element map, adam.hpp the optimizer's rule.  The host side by job: train_check (the arguments),
// train_slab (train.hpp: the slab's layout), train_fill (what both argument blocks share), train_chunk and the chunk loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "engine.hpp"
#include "lds_optin.hpp"
#include "tile_walk.hpp"
#include "train.hpp"

namespace hipets {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// One 16 x 16 tile of C = A . B (M x K by K x N), element (i, k) of A at A[i * sam + k * sak], (k, j) of B at B[k * sbk + j * sbn].
// Lane l feeds A[m0 + (l & 15)][k + (l >> 4)] and B[k + (l >> 4)][n0 + (l & 15)]; the result lies as tile_walk.hpp says.
// The operands come from L1 / L2 (or LDS) one float per lane, so the loop waits on load latency: kDeep blocks of 4
// k-steps issue their 8 loads before their 4 MFMAs (forward and dA products), the others blocks of 2 (the dW product: the deeper
// form there spilt SGPRs to scratch).  Two accumulators over alternate k-steps; out-of-range operands are zeros.
// (sac.hip's sac_seg_acc is the other k-loop of the learning kernels and stays apart: lane group q takes k0 + q, k0 + 4 + q, ... here
// and k0 + 4 q + s there, so the two sum along k in different orders -- other bits -- and load differently -- other speed.)
template <bool kDeep>
__device__ __forceinline__ f32x4 mm_tile(const float* __restrict__ A, int sam, int sak, int M, const float* __restrict__ B, int sbk, int sbn,
                                         int N, int K, int m0, int n0, int lane) {
    const int r = lane & 15, q = lane >> 4;
    const bool av = m0 + r < M, bv = n0 + r < N;
    const float* pa = A + (int64_t)(av ? m0 + r : 0) * sam;
    const float* pb = B + (int64_t)(bv ? n0 + r : 0) * sbn;
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    int k0 = 0;
    // per-lane pointers to k-steps 0..3 of the current block of 16 (VGPRs), advanced by 16 rows / columns per block
    const int64_t sa4 = (int64_t)4 * sak, sb4 = (int64_t)4 * sbk;
    const float* a0p = pa + (int64_t)q * sak;
    const float* b0p = pb + (int64_t)q * sbk;
    const float *a1p = a0p + sa4, *a2p = a0p + 2 * sa4, *a3p = a0p + 3 * sa4;
    const float *b1p = b0p + sb4, *b2p = b0p + 2 * sb4, *b3p = b0p + 3 * sb4;
    for (; kDeep && k0 + 16 <= K; k0 += 16) {
        const float a0 = av ? *a0p : 0.f, a1 = av ? *a1p : 0.f, a2 = av ? *a2p : 0.f, a3 = av ? *a3p : 0.f;
        const float b0 = bv ? *b0p : 0.f, b1 = bv ? *b1p : 0.f, b2 = bv ? *b2p : 0.f, b3 = bv ? *b3p : 0.f;
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, c1, 0, 0, 0);
        a0p += 4 * sa4; a1p += 4 * sa4; a2p += 4 * sa4; a3p += 4 * sa4;
        b0p += 4 * sb4; b1p += 4 * sb4; b2p += 4 * sb4; b3p += 4 * sb4;
    }
    for (; k0 + 8 <= K; k0 += 8) {
        const int ka = k0 + q, kb = k0 + 4 + q;
        const float a0 = av ? pa[(int64_t)ka * sak] : 0.f, b0 = bv ? pb[(int64_t)ka * sbk] : 0.f;
        const float a1 = av ? pa[(int64_t)kb * sak] : 0.f, b1 = bv ? pb[(int64_t)kb * sbk] : 0.f;
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, c1, 0, 0, 0);
    }
    for (; k0 < K; k0 += 4) {
        const int k = k0 + q;
        const float a0 = (av && k < K) ? pa[(int64_t)k * sak] : 0.f, b0 = (bv && k < K) ? pb[(int64_t)k * sbk] : 0.f;
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, c0, 0, 0, 0);
    }
    return c0 + c1;
}

// the activation modules of GaussianMLP (gaussian_mlp.py:88-96) and their derivatives in terms of the pre-activation z
__device__ __forceinline__ float act_fwd(int act, float z, float slope) {
    switch (act) {
        case HIPETS_ACT_RELU: return z > 0.f ? z : 0.f;
        case HIPETS_ACT_SILU: return z / (1.f + expf(-z));
        case HIPETS_ACT_LEAKY_RELU: return z > 0.f ? z : z * slope;
        case HIPETS_ACT_TANH: return tanhf(z);
        default: return 1.f / (1.f + expf(-z));
    }
}

__device__ __forceinline__ float act_grad(int act, float z, float slope) {
    switch (act) {
        case HIPETS_ACT_RELU: return z > 0.f ? 1.f : 0.f;
        case HIPETS_ACT_SILU: {
            const float s = 1.f / (1.f + expf(-z));
            return s * (1.f + z * (1.f - s));
        }
        case HIPETS_ACT_LEAKY_RELU: return z > 0.f ? 1.f : slope;
        case HIPETS_ACT_TANH: {
            const float t = tanhf(z);
            return 1.f - t * t;
        }
        default: {
            const float s = 1.f / (1.f + expf(-z));
            return s * (1.f - s);
        }
    }
}

// torch.nn.functional.softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float softplus_grad(float x) {
    if (x > 20.f) return 1.f;
    const float z = expf(x);
    return z / (z + 1.f);
}

template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// kLoss = the loss tail: kTrainLossNLL (output layer 2 out wide, mean | raw logvar) or kTrainLossMSE (output layer out wide).
// The MSE loss is a sum, not a mean: the loss and the gradient are not scaled down by rows x dims, so loss[s, e] and grad_sq[s, e]
// are large numbers whose float32 rounding shows; under MSE both are accumulated in double (same fixed order) and rounded once.
template <int kLoss>
__global__ __launch_bounds__(kTrainThreads) void train_step_kernel(const TrainStepArgs a) {
    using acc_t = std::conditional_t<kLoss == kTrainLossMSE, double, float>;
    __shared__ acc_t red[2][kTrainThreads / 64];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kTrainThreads / 64;
    const int E = a.ensemble_size, L = a.n_layers, in = a.dims[0], out = a.out_dim, out2 = 2 * out, bmax = a.max_batch;
    float* slab = a.slab + (int64_t)e * a.at.stride;
    float* A0 = slab + a.at.off_a[0];
    float* T = slab + a.at.off_t;
    float* O = slab + a.at.off_o;
    for (int s = 0; s < a.n_steps; ++s) {
        const int nb = min(max(a.rows[s], 1), bmax);
        const int32_t* ix = a.idx + ((int64_t)s * E + e) * bmax;
        // ---- gather the step's rows (an index outside the dataset reads zeros: never out of bounds) ----
        for (int t = tid; t < nb * in; t += kTrainThreads) {
            const int r = t / in, k = t - r * in;
            const int64_t row = ix[r];
            A0[t] = (row >= 0 && row < a.n_rows) ? a.x[row * in + k] : 0.f;
        }
        for (int t = tid; t < nb * out; t += kTrainThreads) {
            const int r = t / out, k = t - r * out;
            const int64_t row = ix[r];
            T[t] = (row >= 0 && row < a.n_rows) ? a.y[row * out + k] : 0.f;
        }
        __syncthreads();
        // ---- forward: Z_l = A_l W_l + b_l, A_{l+1} = act(Z_l); the output layer's raw columns go to O ----
        for (int l = 0; l < L; ++l) {
            const int din = a.dims[l], dout = a.dims[l + 1];
            const float* Ain = slab + a.at.off_a[l];
            const float* W = a.w[l] + (int64_t)e * din * dout;
            const float* bias = a.b[l] + (int64_t)e * dout;
            const bool hidden = l < L - 1;
            float* Z = hidden ? slab + a.at.off_z[l] : O;
            float* An = hidden ? slab + a.at.off_a[l + 1] : nullptr;
            const int tn = tiles_across(dout), tiles = tiles_across(nb) * tn;
            for (int t = wave; t < tiles; t += kWaves) {
                const int m0 = tile_m0(t, tn), n0 = tile_n0(t, tn);
                const f32x4 c = mm_tile<true>(Ain, din, 1, nb, W, dout, 1, dout, din, m0, n0, lane);
                const int col = tile_col(n0, lane);
                if (col < dout) {
                    const float bc = bias[col];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = tile_row(m0, lane, i);
                        if (row < nb) {
                            const float z = c[i] + bc;
                            Z[row * dout + col] = z;
                            if (hidden) An[row * dout + col] = act_fwd(a.activation, z, a.leaky_slope);
                        }
                    }
                }
            }
            __syncthreads();
        }
        float* D = slab + a.at.off_d0;
        acc_t lsum = 0;
        if constexpr (kLoss == kTrainLossMSE) {
            // ---- MSE tail (gaussian_mlp.py:283-289): the plain sum of squared errors; O and D are [nb, out] ----
            for (int t = tid; t < nb * out; t += kTrainThreads) {
                const float d = O[t] - T[t];
                lsum += (acc_t)d * (acc_t)d;
                D[t] = 2.f * d * a.grad_scale;
            }
        } else {
            // ---- NLL tail (gaussian_mlp.py:143-153, 291-305; util/math.py:41-64) and its gradient w.r.t. O ----
            const float scale = 1.f / (float)(nb * out) * a.grad_scale;  // mean over batch and output dims (times 1 / E: BasicEnsemble.loss)
            const float* mxv = a.max_logvar + (int64_t)e * a.bounds_stride;
            const float* mnv = a.min_logvar + (int64_t)e * a.bounds_stride;
            for (int t = tid; t < nb * out; t += kTrainThreads) {
                const int r = t / out, j = t - r * out;
                const float mean = O[r * out2 + j], raw = O[r * out2 + out + j];
                const float mx = mxv[j], mn = mnv[j];
                const float u = mx - raw;
                const float lv1 = mx - softplus(u);
                const float w = lv1 - mn;
                const float lv = mn + softplus(w);
                const float d = mean - T[t];
                const float iv = expf(-lv);
                const float l2iv = d * d * iv;
                lsum += l2iv + lv;
                D[r * out2 + j] = 2.f * d * (scale * iv);
                const float dlv = scale - scale * l2iv;
                D[r * out2 + out + j] = dlv * softplus_grad(w) * softplus_grad(u);
            }
        }
        __syncthreads();
        // ---- backward, last layer first: dA_l = dZ_l W_l^T (weights before the update), db, dW = A_l^T dZ_l with Adam fused ----
        acc_t gsq = 0;
        const float nss = a.neg_step_size[s], bc2s = a.bc2_sqrt[s];
        int cur = 0;
        for (int l = L - 1; l >= 0; --l) {
            const int din = a.dims[l], dout = a.dims[l + 1];
            const float* Dc = slab + (cur ? a.at.off_d1 : a.at.off_d0);
            float* Dn = slab + (cur ? a.at.off_d0 : a.at.off_d1);
            const int64_t wo = (int64_t)e * din * dout;
            float* W = a.w[l] + wo;
            float* mW = a.mw[l] + wo;
            float* vW = a.vw[l] + wo;
            if (l > 0) {
                const float* Zp = slab + a.at.off_z[l - 1];
                const int tn = tiles_across(din), tiles = tiles_across(nb) * tn;
                for (int t = wave; t < tiles; t += kWaves) {
                    const int m0 = tile_m0(t, tn), n0 = tile_n0(t, tn);
                    const f32x4 c = mm_tile<true>(Dc, dout, 1, nb, W, 1, dout, din, dout, m0, n0, lane);
                    const int col = tile_col(n0, lane);
                    if (col < din) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = tile_row(m0, lane, i);
                            if (row < nb) Dn[row * din + col] = c[i] * act_grad(a.activation, Zp[row * din + col], a.leaky_slope);
                        }
                    }
                }
            }
            {
                float* bias = a.b[l] + (int64_t)e * dout;
                float* mB = a.mb[l] + (int64_t)e * dout;
                float* vB = a.vb[l] + (int64_t)e * dout;
                for (int j = tid; j < dout; j += kTrainThreads) {
                    float g = 0.f;
                    if constexpr (kLoss == kTrainLossMSE) {
                        // the MSE loss is a sum, not a mean: gradients are not scaled down by rows x dims, a bias gradient sums rows of both
                        // signs, and its square is most of grad_sq -- so the rows are summed compensated (Kahan), to one rounding
                        float comp = 0.f;
                        for (int r = 0; r < nb; ++r) {
                            const float yk = Dc[r * dout + j] - comp;
                            const float tk = g + yk;
                            comp = (tk - g) - yk;
                            g = tk;
                        }
                    } else {
                        for (int r = 0; r < nb; ++r) g += Dc[r * dout + j];
                    }
                    gsq += (acc_t)g * (acc_t)g;
                    const float p = bias[j];
                    bias[j] = adam_update(p, g + a.weight_decay * p, mB + j, vB + j, a.adam, nss, bc2s);  // (coupled weight decay)
                }
            }
            __syncthreads();  // every read of the old W_l (dA above) is done
            {
                const float* Ain = slab + a.at.off_a[l];
                const int tn = tiles_across(dout), tiles = tiles_across(din) * tn;
                for (int t = wave; t < tiles; t += kWaves) {
                    const int m0 = tile_m0(t, tn), n0 = tile_n0(t, tn);
                    const f32x4 c = mm_tile<false>(Ain, 1, din, din, Dc, dout, 1, dout, nb, m0, n0, lane);
                    const int col = tile_col(n0, lane);
                    if (col < dout) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int row = tile_row(m0, lane, i);
                            if (row < din) {
                                const int64_t o = (int64_t)row * dout + col;
                                gsq += (acc_t)c[i] * (acc_t)c[i];
                                const float p = W[o];
                                W[o] = adam_update(p, c[i] + a.weight_decay * p, mW + o, vW + o, a.adam, nss, bc2s);
                            }
                        }
                    }
                }
            }
            __syncthreads();  // the next layer's dA reads Dn; the next step's forward reads the new weights
            cur ^= 1;
        }
        // ---- per-member loss and raw-gradient square sum of the step, reduced in a fixed order ----
        lsum = wave_sum(lsum);
        gsq = wave_sum(gsq);
        if (lane == 0) {
            red[0][wave] = lsum;
            red[1][wave] = gsq;
        }
        __syncthreads();
        if (tid == 0) {
            acc_t ls = 0, gs = 0;
            for (int w = 0; w < kWaves; ++w) {
                ls += red[0][w];
                gs += red[1][w];
            }
            a.loss[(int64_t)s * E + e] = kLoss == kTrainLossMSE ? (float)ls : (float)ls / (float)(nb * out);
            a.grad_sq[(int64_t)s * E + e] = (float)gs;
        }
        __syncthreads();
    }
}

// evaluate: workgroup (tile, member) runs kEvalRows rows through the member with activations in LDS; the output layer computes its
// first out_dim (mean) columns only.  Writes the tile's squared-error sum to partial[e, tile] (rows in order, one thread).
__global__ __launch_bounds__(kEvalThreads) void train_eval_kernel(const TrainEvalArgs a) {
    extern __shared__ float lds[];
    const int tile = blockIdx.x, e = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kEvalThreads / 64;
    const int L = a.n_layers, in = a.dims[0], out = a.out_dim;
    const int64_t r0 = (int64_t)tile * kEvalRows;
    const int nr = (int)min((int64_t)kEvalRows, a.n_rows - r0);
    float* cur = lds;
    float* nxt = lds + kEvalRows * a.max_width;
    __shared__ int64_t rows[kEvalRows];
    if (tid < nr) {
        int64_t r = a.order ? (int64_t)a.order[r0 + tid] : r0 + tid;
        rows[tid] = (r >= 0 && r < a.n_rows) ? r : -1;
    }
    __syncthreads();
    for (int t = tid; t < nr * in; t += kEvalThreads) {
        const int r = t / in, k = t - r * in;
        cur[t] = rows[r] >= 0 ? a.x[rows[r] * in + k] : 0.f;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        const int din = a.dims[l], ld = a.dims[l + 1];
        const bool hidden = l < L - 1;
        const int dout = hidden ? ld : out;
        const float* W = a.w[l] + (int64_t)e * din * ld;
        const float* bias = a.b[l] + (int64_t)e * ld;
        const int tn = tiles_across(dout), tiles = tiles_across(nr) * tn;
        for (int t = wave; t < tiles; t += kWaves) {
            const int m0 = tile_m0(t, tn), n0 = tile_n0(t, tn);
            const f32x4 c = mm_tile<true>(cur, din, 1, nr, W, ld, 1, dout, din, m0, n0, lane);
            const int col = tile_col(n0, lane);
            if (col < dout) {
                const float bc = bias[col];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = tile_row(m0, lane, i);
                    if (row < nr) {
                        const float z = c[i] + bc;
                        if (hidden) {
                            nxt[row * dout + col] = act_fwd(a.activation, z, a.leaky_slope);
                        } else {
                            const float d = rows[row] >= 0 ? z - a.y[rows[row] * out + col] : 0.f;
                            nxt[row * dout + col] = d * d;
                        }
                    }
                }
            }
        }
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    // cur = [nr, out] squared errors: per-row sums (dims in order), then the tile's sum (rows in order)
    __shared__ float rsum[kEvalRows];
    if (tid < nr) {
        float s = 0.f;
        for (int j = 0; j < out; ++j) s += cur[tid * out + j];
        rsum[tid] = s;
        if (a.row_score) a.row_score[(int64_t)e * a.n_rows + r0 + tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int r = 0; r < nr; ++r) s += rsum[r];
        a.partial[(int64_t)e * a.tiles + tile] = s;
    }
}

// score[e] = (sum over tiles of partial[e, tile]) / (n_rows * out): every thread sums a fixed strided subset, then a fixed tree
__global__ __launch_bounds__(256) void train_eval_reduce_kernel(const TrainEvalArgs a) {
    __shared__ float s[256];
    const int e = blockIdx.x, tid = threadIdx.x;
    float acc = 0.f;
    for (int t = tid; t < a.tiles; t += 256) acc += a.partial[(int64_t)e * a.tiles + t];
    s[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s[tid] += s[tid + h];
        __syncthreads();
    }
    if (tid == 0) a.score[e] = s[0] / ((float)a.n_rows * (float)a.out_dim);
}

// ---- the C ABI's argument checks (hipets_train_steps / hipets_train_eval below) ----

int train_check(const hipets_train_desc* d, bool adam, int loss_kind) {
    if (!d) return fail("null train desc");
    if (loss_kind != HIPETS_TRAIN_LOSS_NLL && loss_kind != HIPETS_TRAIN_LOSS_MSE) return fail("unknown loss kind %d", loss_kind);
    if (d->ensemble_size < 1 || d->ensemble_size > kTrainMaxMembers) return fail("ensemble_size %d outside [1, %d]", d->ensemble_size, kTrainMaxMembers);
    if (d->n_layers < 2 || d->n_layers > HIPETS_MAX_LAYERS) return fail("n_layers %d outside [2, %d]", d->n_layers, HIPETS_MAX_LAYERS);
    if (d->in_dim < 1 || d->in_dim > kTrainMaxIn) return fail("in_dim %d outside [1, %d]", d->in_dim, kTrainMaxIn);
    if (d->hid < 1 || d->hid > kTrainMaxHid) return fail("hid %d outside [1, %d]", d->hid, kTrainMaxHid);
    if (d->out_dim < 1 || d->out_dim > kTrainMaxOut) return fail("out_dim %d outside [1, %d]", d->out_dim, kTrainMaxOut);
    if (d->activation < HIPETS_ACT_RELU || d->activation > HIPETS_ACT_SIGMOID) return fail("unknown activation %d", d->activation);
    if (d->max_batch < 1 || d->max_batch > kTrainMaxBatch) return fail("max_batch %d outside [1, %d]", d->max_batch, kTrainMaxBatch);
    if (!d->weights || !d->biases) return fail("null parameter arrays");
    for (int l = 0; l < d->n_layers; ++l)
        if (!d->weights[l] || !d->biases[l]) return fail("null parameter of layer %d", l);
    if (adam) {
        if (!d->exp_avg_w || !d->exp_avg_b || !d->exp_avg_sq_w || !d->exp_avg_sq_b) return fail("null Adam state or logvar bounds");
        if (loss_kind == HIPETS_TRAIN_LOSS_NLL && (!d->min_logvar || !d->max_logvar)) return fail("null Adam state or logvar bounds");
        for (int l = 0; l < d->n_layers; ++l)
            if (!d->exp_avg_w[l] || !d->exp_avg_b[l] || !d->exp_avg_sq_w[l] || !d->exp_avg_sq_b[l]) return fail("null Adam state of layer %d", l);
        // torch.optim.Adam's own argument checks (torch/optim/adam.py)
        if (!(d->lr >= 0.0) || !(d->eps >= 0.0) || !(d->weight_decay >= 0.0)) return fail("invalid lr / eps / weight_decay");
        if (!(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0)) return fail("invalid betas");
        if (d->steps_per_launch < 0) return fail("steps_per_launch %d < 0", d->steps_per_launch);
    }
    return 0;
}

// what TrainStepArgs and TrainEvalArgs share: the layers' widths and parameters, the dataset, the counts
template <class Args>
void train_fill(Args& a, const hipets_train_desc* d, int loss_kind, const float* x, const float* y, int64_t n_rows) {
    a.dims[0] = d->in_dim;
    for (int l = 1; l < d->n_layers; ++l) a.dims[l] = d->hid;
    a.dims[d->n_layers] = loss_kind == HIPETS_TRAIN_LOSS_MSE ? d->out_dim : 2 * d->out_dim;
    for (int l = 0; l < d->n_layers; ++l) {
        a.w[l] = static_cast<float*>(d->weights[l]);
        a.b[l] = static_cast<float*>(d->biases[l]);
    }
    a.x = x;
    a.y = y;
    a.n_rows = n_rows;
    a.n_layers = d->n_layers;
    a.out_dim = d->out_dim;
    a.ensemble_size = d->ensemble_size;
    a.activation = d->activation;
    a.leaky_slope = d->leaky_slope;
}

// steps per launch: the caller's, or launches of ~50 ms at most: a step costs ~ 6 B P flops per member at the ~50 GFLOP/s per CU the
// kernel reaches (measured at both halfcheetah shapes)
int train_chunk(const hipets_train_desc* d, const int32_t* dims) {
    int chunk = d->steps_per_launch;
    if (chunk == 0) {
        double params = 0.0;
        for (int l = 0; l < d->n_layers; ++l) params += (double)dims[l] * dims[l + 1];
        const double step_us = 20.0 + 6.0 * d->max_batch * params / 5.0e4;
        chunk = (int)std::max(1.0, std::min((double)kTrainMaxSteps, 50000.0 / step_us));
    }
    return std::min(chunk, kTrainMaxSteps);
}

}  // namespace

hipError_t launch_train_steps(const TrainStepArgs& a, int loss_kind, hipStream_t st) {
    if (loss_kind == kTrainLossMSE)
        hipLaunchKernelGGL(train_step_kernel<kTrainLossMSE>, dim3(a.ensemble_size), dim3(kTrainThreads), 0, st, a);
    else
        hipLaunchKernelGGL(train_step_kernel<kTrainLossNLL>, dim3(a.ensemble_size), dim3(kTrainThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_train_eval(const TrainEvalArgs& a, hipStream_t st) {
    const size_t lds = (size_t)2 * kEvalRows * a.max_width * sizeof(float);
    static LdsOptIn once;
    hipError_t err = full_lds_once(once, reinterpret_cast<const void*>(&train_eval_kernel), 2 * kEvalRows * kTrainMaxIn * (int)sizeof(float));
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(train_eval_kernel, dim3(a.tiles, a.ensemble_size), dim3(kEvalThreads), lds, st, a);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(train_eval_reduce_kernel, dim3(a.ensemble_size), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace hipets

// ---- the C ABI: validation, workspace, chunking ----
using namespace hipets;

extern "C" {

int hipets_train_steps(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows, const int32_t* idx,
                       const int32_t* rows, int32_t n_steps, int64_t step0, float* loss, float* grad_sq, void* stream) {
    return hipets_train_steps_loss(e, d, x, y, n_rows, idx, rows, n_steps, step0, loss, grad_sq, stream, HIPETS_TRAIN_LOSS_NLL, 0, 1.0f);
}

int hipets_train_steps_loss(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows, const int32_t* idx,
                            const int32_t* rows, int32_t n_steps, int64_t step0, float* loss, float* grad_sq, void* stream, int32_t loss_kind,
                            int32_t bounds_per_member, float grad_scale) {
    if (!e) return fail("null engine");
    if (train_check(d, true, loss_kind)) return 1;
    if (!std::isfinite(grad_scale) || !(grad_scale > 0.f)) return fail("grad_scale %g is not a finite positive number", (double)grad_scale);
    if (!x || !y || !idx || !rows || !loss || !grad_sq) return fail("null argument");
    if (n_rows < 1 || n_rows > INT32_MAX) return fail("n_rows %lld outside [1, 2^31)", (long long)n_rows);
    if (n_steps < 0) return fail("n_steps %d < 0", n_steps);
    if (step0 < 0) return fail("step0 %lld < 0", (long long)step0);
    if (n_steps == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    TrainStepArgs a{};
    const int L = d->n_layers, E = d->ensemble_size, Bm = d->max_batch;
    train_fill(a, d, loss_kind, x, y, n_rows);
    a.at = train_slab(a.dims, L, d->out_dim, Bm);
    if (e->train_slab.ensure((size_t)E * a.at.stride * sizeof(float))) return 1;
    a.slab = e->train_slab.as<float>();
    for (int l = 0; l < L; ++l) {
        a.mw[l] = static_cast<float*>(d->exp_avg_w[l]);
        a.mb[l] = static_cast<float*>(d->exp_avg_b[l]);
        a.vw[l] = static_cast<float*>(d->exp_avg_sq_w[l]);
        a.vb[l] = static_cast<float*>(d->exp_avg_sq_b[l]);
    }
    a.min_logvar = d->min_logvar;
    a.max_logvar = d->max_logvar;
    a.bounds_stride = bounds_per_member ? d->out_dim : 0;
    a.grad_scale = grad_scale;
    a.max_batch = Bm;
    a.weight_decay = (float)d->weight_decay;  // (a python float handed to a float32 tensor op: one rounding)
    a.adam = adam_scalars(d->lr, d->beta1, d->beta2, d->eps, step0 + 1);  // (the part no step changes)
    const int chunk = train_chunk(d, a.dims);
    for (int s0 = 0; s0 < n_steps; s0 += chunk) {
        const int n = std::min(chunk, n_steps - s0);
        for (int i = 0; i < n; ++i) {
            const AdamScalars ad = adam_scalars(d->lr, d->beta1, d->beta2, d->eps, step0 + s0 + i + 1);
            a.neg_step_size[i] = ad.neg_step_size;
            a.bc2_sqrt[i] = ad.bc2_sqrt;
        }
        a.n_steps = n;
        a.idx = idx + (int64_t)s0 * E * Bm;
        a.rows = rows + s0;
        a.loss = loss + (int64_t)s0 * E;
        a.grad_sq = grad_sq + (int64_t)s0 * E;
        hipError_t err = launch_train_steps(a, loss_kind, st);
        if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "train step kernel launch failed: %s", hipGetErrorString(err));
    }
    return 0;
}

int hipets_train_eval(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows, const int32_t* order,
                      float* score, float* row_score, void* stream) {
    return hipets_train_eval_loss(e, d, x, y, n_rows, order, score, row_score, stream, HIPETS_TRAIN_LOSS_NLL);
}

int hipets_train_eval_loss(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows, const int32_t* order,
                           float* score, float* row_score, void* stream, int32_t loss_kind) {
    if (!e) return fail("null engine");
    if (train_check(d, false, loss_kind)) return 1;
    if (!x || !y || !score) return fail("null argument");
    if (n_rows < 1 || n_rows > INT32_MAX) return fail("n_rows %lld outside [1, 2^31)", (long long)n_rows);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    TrainEvalArgs a{};
    train_fill(a, d, loss_kind, x, y, n_rows);
    a.tiles = (int)((n_rows + kEvalRows - 1) / kEvalRows);
    if (e->train_partial.ensure((size_t)d->ensemble_size * a.tiles * sizeof(float))) return 1;
    a.partial = e->train_partial.as<float>();
    a.order = order;
    a.row_score = row_score;
    a.score = score;
    a.max_width = std::max(std::max(d->in_dim, d->hid), d->out_dim);
    hipError_t err = launch_train_eval(a, st);
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "train eval kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

}  // extern "C"
