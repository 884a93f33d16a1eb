// ensemble_bf16.hip -- the bf16 form of hipets_ensemble_predict (ensemble_bf16.hpp; hipets_set_ensemble_kernel): every member's mean and
// log-variance of a batch and the four uncertainty statistics in one launch on the bf16 matrix pipe, 16 R rows per workgroup (R = 4, or 2
// where LDS or registers do not allow 4).  Arithmetic: for every linear layer both operands rounded to bf16 nearest-even, exact
// products (8 x 8 significand bits), fp32 accumulation by v_mfma_f32_16x16x32_bf16 in k-chunk order; bias, activation, the head and the
// statistics in fp32, op by op (the unit is compiled without contraction and without packed fp32 VALU instructions).
//
// LDS holds X [16 R][64 kc0 + 16 bytes], the model input (built once in fp32 exactly as the other forms build it, rounded to bf16 as layer
// 0's operand, kept for all members), H [16 R][64 kch + 16 bytes], ONE hidden buffer, both in gemm_bf16.hpp's fragment row format -- per
// row [32-wide k chunk][4 groups][8 x bf16], so a lane's B-operand fragment is one ds_read_b128 -- and the waves' partial row sums
// [2][8][16 R].  Weights are the A operand, activations the B operand: lane (r = l & 15, g = l >> 4) of an accumulator holds output
// columns 16 tile + 4 g .. + 3 of batch row 16 i + r.  Per member:
//   hidden layers   wave w owns column tiles w, w + 8, ... (TH of them) and holds their TH x R accumulators over the full K; every weight
//                   fragment it loads meets all R row tiles.  Barrier (every wave has read H), act(acc + bias) rounded to bf16 back into H
//                   as one packed 8-byte write per tile -- that store IS the next layer's operand rounding --, barrier.
//   output layer    wave w owns MEAN column tiles w, w + 8, ... (T of them); the weight images keep the log-variance columns of the same
//                   dims as a tile of their own (ensemble_bf16.hpp), so one k loop feeds R x 2 accumulators.  Then the head of
//                   gaussian_mlp.py:150-153 on the registers and the stores of the requested elements.  Nothing of it touches LDS.
//   statistics      as the wide form: m0 and S1 = sum_m (mean_m - m0) per (row, column) in registers across the member loop, the shifted
//                   variance rule, never E[x^2] - E[x]^2.
// The k loops are paced by the weight fragment loads (1 KB per wave, tile and chunk from L2), not the MFMAs: a ring keeps
// ens_bf16_ahead(TH) chunks of them in flight; co-resident workgroups hide the rest.
// Row sums over the columns run in ONE order: a lane adds its own four columns and tiles ascending, a fixed butterfly over the 4 lanes that
// share a row (xor 16, xor 32), one partial per wave and row into LDS, and behind a barrier thread `row` adds the partials in wave order.
// With R fixed by the shape, a row's bits depend on the model's shape alone.  Rows past the batch and columns past the real ones are
// staged as zeros; padded weights and biases are zeros, so no loop tests a bound.
#include <hip/hip_runtime.h>

#include "agent_forms.hpp"
#include "common.hpp"
#include "ensemble_bf16.hpp"
#include "gemm_bf16.hpp"
#include "lds_optin.hpp"

namespace hipets {

namespace {

static_assert(kEnsBf16Waves * kWave == kPolicyThreads, "the bf16 ensemble kernel runs policy_layer.hpp's 512 threads");

// this wave's tiles among `tiles`: wave, wave + 8, ...
__device__ __forceinline__ int ens_bf16_own(const int tiles, const int wave) {
    const int left = tiles - wave;
    return left > 0 ? (left + kEnsBf16Waves - 1) / kEnsBf16Waves : 0;
}

// acc[t][i] += W_t[16][32 KC] in[16 i ..][32 KC]^T for `nt` column tiles whose fragments start at W + off[t] (16-byte entries, this
// lane's included; consecutive chunks 64 entries apart): a ring of AHEAD fragment sets, slot s holding chunks s, s + AHEAD, ...; a slot
// is refilled as soon as its MFMAs are issued (gemm_bf16.hpp's k loop).  The R activation fragments of a chunk are read from LDS right
// before its MFMAs.
template <int R, int NT, int AHEAD>
__device__ __forceinline__ void ens_bf16_gemm(const char* __restrict__ ap, const int ld, const int KC, const uint4* __restrict__ W, const unsigned (&off)[NT],
                                              const int nt, f32x4 (&acc)[NT][R]) {
    u32x4 f[AHEAD][NT];
    auto load = [&](u32x4 (&s)[NT], const int kk) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < nt) s[t] = *reinterpret_cast<const u32x4*>(W + off[t] + (size_t)kk * 64);
    };
    auto compute = [&](const u32x4 (&s)[NT], const int kk) __attribute__((always_inline)) {
        u32x4 a[R];
#pragma unroll
        for (int i = 0; i < R; ++i) a[i] = *reinterpret_cast<const u32x4*>(ap + i * 16 * ld + kk * 64);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t < nt) {
#pragma unroll
                for (int i = 0; i < R; ++i) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(s[t]), as_bf16x8(a[i]), acc[t][i], 0, 0, 0);
            }
        }
    };
#pragma unroll
    for (int s = 0; s < AHEAD; ++s)
        if (s < KC) load(f[s], s);
    for (int kk = 0; kk < KC; kk += AHEAD) {
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) {
            if (kk + s < KC) {
                __builtin_amdgcn_sched_barrier(0);
                compute(f[s], kk + s);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + s + AHEAD < KC) load(f[s], kk + s + AHEAD);
            }
        }
    }
}

// sum over the 4 lanes that share a batch row (lanes r, r + 16, r + 32, r + 48): every lane gets the same bits
__device__ __forceinline__ float ens_bf16_row_sum(float x) {
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
}

// this wave's partial of one row sum, for the rows its lanes hold: P[wave][16 i + r]
template <int R>
__device__ __forceinline__ void ens_bf16_put_partial(float* P, const float (&v)[R], const int wave, const int lane) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const float s = ens_bf16_row_sum(v[i]);
        if (lane < 16) P[wave * (kTile * R) + i * kTile + lane] = s;
    }
}

// the row sum of row `row`: the waves' partials in wave order
template <int R>
__device__ __forceinline__ float ens_bf16_get_sum(const float* P, const int row) {
    float v = P[row];
#pragma unroll
    for (int w = 1; w < kEnsBf16Waves; ++w) v += P[w * (kTile * R) + row];
    return v;
}

// R row tiles, T mean column tiles and TH hidden column tiles per wave at most; kStats: stats requested (without: no m0 / S1 state)
template <int R, int T, int TH, bool kStats>
__global__ __launch_bounds__(kPolicyThreads) void ensemble_predict_bf16_kernel(const EnsBf16Args a) {
    extern __shared__ __attribute__((aligned(16))) char ens_bf16_smem[];
    constexpr int kRows = kTile * R;
    constexpr int kAhead = ens_bf16_ahead(TH);
    const int ld_x = 64 * a.g.kc0 + kEnsBf16RowPad, ld_h = 64 * a.g.kch + kEnsBf16RowPad;  // bytes
    char* X = ens_bf16_smem;                                  // [kRows][ld_x]: the kept model input, bf16
    char* H = X + kRows * ld_x;                               // [kRows][ld_h]: the hidden buffer, bf16
    float* P = reinterpret_cast<float*>(H + kRows * ld_h);    // [kEnsBf16Sums][8][kRows]: the waves' partial row sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * kRows;

    // ---- the model input, once: fp32 as the other forms build it, then layer 0's operand rounding; rows past the batch and columns
    // past in_dim are zeros.  H's columns past pad16(hid) are never written: zeros from here on (their weight rows are zeros too) ----
    const int obs_in = a.in_dim - a.act_dim, kx = 32 * a.g.kc0;
    for (int t = tid; t < kRows * kx; t += kPolicyThreads) {
        const int xr = t / kx, k = t - xr * kx;
        const long long row = row0 + xr;
        float v = 0.f;
        if (row < a.B && k < a.in_dim) {
            if (a.model_in) {
                v = a.model_in[row * a.in_dim + k];
            } else {
                v = model_input_element(a.obs + row * a.obs_dim, a.actions + row * a.act_dim, k, obs_in, a.in_dim, a.obs_process, a.cols, a.normalizer, a.norm);
            }
        }
        // (the hardware's conversion: nearest-even, bf16_rne_bits for every finite value, and a NaN stays a NaN)
        *reinterpret_cast<__bf16*>(X + xr * ld_x + (k >> 5) * 64 + ((k & 31) >> 3) * 16 + (k & 7) * 2) = (__bf16)v;
    }
    for (int t = tid; t < kRows * (ld_h / 4); t += kPolicyThreads) reinterpret_cast<unsigned*>(H)[t] = 0u;

    const int nth = ens_bf16_own(a.g.th, wave);  // this wave's hidden column tiles
    const int ntm = ens_bf16_own(a.g.tm, wave);  // and its mean column tiles
    const int act = a.activation, L = a.n_layers;
    const float slope = a.slope;
    const bool gauss = !a.deterministic;
    const int hp = 16 * a.g.th;
    const char* xp = X + r * ld_x + g * 16;  // this lane's fragment of row tile 0, chunk 0
    const char* hpn = H + r * ld_h + g * 16;
    // the statistics' state: per (row, column) of this wave's mean tiles in registers, per row in thread `row`
    f32x4 m0[kStats ? T : 1][R], s1[kStats ? T : 1][R];
#pragma unroll
    for (int t = 0; t < (kStats ? T : 1); ++t) {
#pragma unroll
        for (int i = 0; i < R; ++i) m0[t][i] = s1[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float ssq = 0.f, sv = 0.f, max_std = 0.f, max_dev = 0.f;
    __syncthreads();  // X is complete, H is zeros

    for (int mi = 0; mi < a.n; ++mi) {
        const int m = a.members[mi];
        const uint4* w = a.wb + (size_t)m * a.wbmember + lane;
        const float* b = a.b + (size_t)m * a.bmember;
        // ---- the hidden layers, in place ----
        for (int l = 0; l < L - 1; ++l) {
            const int KC = l == 0 ? a.g.kc0 : a.g.kch;
            f32x4 acc[TH][R];
            unsigned off[TH];
#pragma unroll
            for (int t = 0; t < TH; ++t) {
                off[t] = (unsigned)((wave + t * kEnsBf16Waves) * KC * 64);
#pragma unroll
                for (int i = 0; i < R; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            ens_bf16_gemm<R, TH, kAhead>(l == 0 ? xp : hpn, l == 0 ? ld_x : ld_h, KC, w, off, nth, acc);
            __syncthreads();  // every wave has read H (this layer's input, or the previous member's last hidden layer under its output layer)
#pragma unroll
            for (int t = 0; t < TH; ++t) {
                if (t < nth) {
                    const int n0 = (wave + t * kEnsBf16Waves) * kTile + 4 * g;  // this lane's four columns (< pad16(hid))
                    const f32x4 bc = *reinterpret_cast<const f32x4*>(b + n0);
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        u32x2 pc[1];
                        split_x4<1>(ens_activate(act, acc[t][i] + bc, slope), pc);
                        *reinterpret_cast<u32x2*>(H + (i * kTile + r) * ld_h + b3_offset<1>(n0, 0)) = pc[0];
                    }
                }
            }
            __syncthreads();
            w += (size_t)a.g.th * KC * 64;
            b += hp;
        }
        // ---- the output layer and the head, on registers ----
        const int lvrow = a.lv_per_member ? m : 0;
        const float* mn = a.lv + (size_t)lvrow * a.out_dim;
        const float* mx = mn + (size_t)(a.lv_per_member ? a.lv_per_member : 1) * a.out_dim;
        float se[R], sd[R];
#pragma unroll
        for (int i = 0; i < R; ++i) se[i] = sd[i] = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t < ntm) {
                const int c = wave + t * kEnsBf16Waves;
                f32x4 cc[2][R];  // [0]: the mean tile, [1]: its log-variance tile
#pragma unroll
                for (int i = 0; i < R; ++i) cc[0][i] = cc[1][i] = f32x4{0.f, 0.f, 0.f, 0.f};
                const unsigned off[2] = {(unsigned)(c * a.g.kch * 64), (unsigned)((a.g.tm + c) * a.g.kch * 64)};
                ens_bf16_gemm<R, 2, kAhead>(hpn, ld_h, a.g.kch, w, off, gauss ? 2 : 1, cc);
                const long long row = row0 + r;  // row tile 0's; tile i: + 16 i
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int d = c * kTile + 4 * g + j;  // this lane's output dim (< pad16(out_dim) <= the bias image)
                    const bool real = d < a.out_dim;
                    const float bm = b[d], bl = b[(gauss && real) ? a.out_dim + d : d];
                    float lo = 0.f, hi = 0.f;
                    if (gauss && real) { lo = mn[d]; hi = mx[d]; }
                    const bool first = mi == 0;
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const bool live = real && row + i * kTile < a.B;
                        const size_t at = ((size_t)mi * a.B + (size_t)(row + i * kTile)) * a.out_dim + d;
                        const float mean = real ? cc[0][i][j] + bm : 0.f;
                        if (live && a.mean) a.mean[at] = mean;
                        if (gauss) {
                            float lv = hi - ens_softplus(hi - (cc[1][i][j] + bl));
                            lv = lo + ens_softplus(lv - lo);
                            if (live && a.logvar) a.logvar[at] = lv;
                            if (kStats) se[i] += real ? expf(lv) : 0.f;
                        }
                        if (kStats) {  // (the first requested member: m0 = its mean, S1 = 0, nothing to the squares)
                            m0[t][i][j] = first ? mean : m0[t][i][j];
                            const float delta = first ? 0.f : mean - m0[t][i][j];
                            s1[t][i][j] = first ? 0.f : s1[t][i][j] + delta;
                            sd[i] += delta * delta;
                        }
                    }
                }
            }
        }
        if (kStats) {
            // (the previous member's partials were read before the barriers of this member's hidden layers)
            ens_bf16_put_partial<R>(P, se, wave, lane);
            ens_bf16_put_partial<R>(P + kEnsBf16Waves * kRows, sd, wave, lane);
            __syncthreads();
            if (tid < kRows) {
                const float e = ens_bf16_get_sum<R>(P, tid), dd = ens_bf16_get_sum<R>(P + kEnsBf16Waves * kRows, tid);
                sv += e;
                ssq += dd;
                max_std = nan_max(max_std, sqrtf(e));
                max_dev = nan_max(max_dev, sqrtf(dd));
            }
        }
    }
    if (!kStats) return;
    // ---- sum_d (S1 / n)^2 the same way, and the four statistics ----
    const float n = (float)a.n;
    float sq[R];
#pragma unroll
    for (int i = 0; i < R; ++i) sq[i] = 0.f;
#pragma unroll
    for (int t = 0; t < (kStats ? T : 1); ++t) {
        if (t < ntm) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const float u = s1[t][i][j] / n;
                    sq[i] += u * u;
                }
            }
        }
    }
    __syncthreads();  // the last member's partials are read
    ens_bf16_put_partial<R>(P, sq, wave, lane);
    __syncthreads();
    const long long row = row0 + tid;
    if (tid < kRows && row < a.B) {
        float var = ssq / n - ens_bf16_get_sum<R>(P, tid);  // sum_d Var_m(mean), population
        var = var < 0.f ? 0.f : var;                         // (rounding only; a NaN stays)
        float* s = a.stats + (size_t)row * 4;
        s[0] = max_std;
        s[1] = sqrtf(var);
        s[2] = sqrtf(var + sv / n);
        s[3] = max_dev;
    }
}

// One layer's A-operand fragments of all members from the snapshot's fp32 images: entry (e, tile, chunk, lane) = the 8 values
// k = 32 chunk + 8 (lane >> 4) .. + 7 of one column, rounded to bf16 nearest-even.  Tiles below `tm` take column 16 tile + (lane & 15)
// where it is below `n_first`; tiles from `tm` on take column second + 16 (tile - tm) + (lane & 15) under the same limit (the output
// layer's log-variance set; a hidden layer has tm = tiles).  Rows past kp and columns past the limit are zeros.
__global__ void ensemble_bf16_pack_kernel(uint4* dst, const float* src, int E, int tiles, int KC, int kp, int np, int tm, int n_first, int second,
                                          size_t dmember, size_t doff, size_t smember, size_t soff) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)tiles * KC * 64;
    if (i >= per * E) return;
    const int e = (int)(i / per);
    const int rem = (int)(i - (long long)e * per);
    const int lane = rem & 63, kk = (rem >> 6) % KC, tile = (rem >> 6) / KC;
    const int cc = 16 * (tile < tm ? tile : tile - tm) + (lane & 15);
    const int col = tile < tm ? cc : second + cc;
    const float* s = src + (size_t)e * smember + soff;
    unsigned h[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = 32 * kk + 8 * (lane >> 4) + q;
        const float v = (cc < n_first && k < kp) ? s[(size_t)k * np + col] : 0.f;
        h[q] = bf16_rne_bits(v) >> 16;
    }
    dst[(size_t)e * dmember + doff + rem] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

using EnsBf16Kernel = void (*)(EnsBf16Args);

// The instances the geometry rule can ask for (ens_bf16_fits): with the statistics one per T, whose state costs T x R x 8 registers;
// without them one per (R, TH), at T = 4 (no state: T only bounds a loop).  TH: 2, or 8 for models wider than 256 hidden units.
EnsBf16Kernel ens_bf16_instance(const EnsBf16Geo& g, const bool stats) {
    if (g.R == 4) {  // TH <= 2, T <= 2
        if (!stats) return ensemble_predict_bf16_kernel<4, 4, 2, false>;
        return g.T == 1 ? ensemble_predict_bf16_kernel<4, 1, 2, true> : ensemble_predict_bf16_kernel<4, 2, 2, true>;
    }
    if (g.TH > 2) return stats ? ensemble_predict_bf16_kernel<2, 1, 8, true> : ensemble_predict_bf16_kernel<2, 4, 8, false>;  // T == 1
    if (!stats) return ensemble_predict_bf16_kernel<2, 4, 2, false>;
    switch (g.T) {
        case 1: return ensemble_predict_bf16_kernel<2, 1, 2, true>;
        case 2: return ensemble_predict_bf16_kernel<2, 2, 2, true>;
        case 3: return ensemble_predict_bf16_kernel<2, 3, 2, true>;
        default: return ensemble_predict_bf16_kernel<2, 4, 2, true>;
    }
}

}  // namespace

hipError_t pack_ensemble_bf16(uint4* wb, const float* w, size_t wmember, int E, int in_dim, int hid, int out_dim, int n_layers, int deterministic,
                              const EnsBf16Geo& g, hipStream_t st) {
    auto pad = [](int x) { return (x + 15) & ~15; };
    const int kp0 = pad(in_dim), hp = pad(hid), npo = pad(deterministic ? out_dim : 2 * out_dim);
    const size_t dmember = ens_bf16_member_entries(g, n_layers, deterministic);
    size_t doff = 0, soff = 0;
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l == n_layers - 1;
        const int kp = l == 0 ? kp0 : hp, np = last ? npo : hp, KC = l == 0 ? g.kc0 : g.kch;
        const int tiles = last ? g.tm * (deterministic ? 1 : 2) : g.th;
        const long long n = (long long)E * tiles * KC * 64;
        hipLaunchKernelGGL(ensemble_bf16_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wb, w, E, tiles, KC, kp, np, last ? g.tm : tiles,
                           last ? out_dim : hp, last ? out_dim : 0, dmember, doff, wmember, soff);
        doff += ens_bf16_layer_entries(g, l, n_layers, deterministic);
        soff += (size_t)kp * np;
    }
    return hipGetLastError();
}

hipError_t launch_ensemble_bf16(const EnsBf16Args& a, size_t lds_max, hipStream_t st) {
    static LdsOptIn opted[2][2][kEnsBf16MaxT + 1];  // [R == 4][TH > 2][T, 0: without statistics]
    const bool stats = a.stats != nullptr;
    const EnsBf16Kernel kernel = ens_bf16_instance(a.g, stats);
    if (a.g.lds > 64 * 1024) {
        const hipError_t err = full_lds_once(opted[a.g.R == 4][a.g.TH > 2][stats ? a.g.T : 0], reinterpret_cast<const void*>(kernel), (int)lds_max);
        if (err != hipSuccess) return err;
    }
    const int rows = kTile * a.g.R;
    const unsigned grid = (unsigned)(((long long)a.B + rows - 1) / rows);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPolicyThreads), (size_t)a.g.lds, st, a);
    return hipGetLastError();
}

}  // namespace hipets
