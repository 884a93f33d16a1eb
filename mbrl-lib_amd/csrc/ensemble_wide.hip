// ensemble_wide.hip -- the wide form of hipets_ensemble_predict (ensemble_wide.hpp; hipets_set_ensemble_kernel): every member's mean
// and log-variance of a batch and the four uncertainty statistics in one launch, 16 R rows per workgroup (R = 4, or 2 where the input
// is too wide for 4), on the packed images hipets_ensemble_set already makes.  A unit of its own, compiled without packed fp32 VALU
// instructions; ensemble.hip, which holds the tile kernel, keeps its flags and its code.
//
// LDS holds X [16 R][kp0 + 4], the model input (built once, kept for all members), H [16 R][hp + 4], ONE hidden buffer, and the waves'
// partial row sums [2][8][16 R].  Per member:
//   hidden layers   wave w owns column tiles w, w + 8, ... (TH of them) and holds their TH x R x 4 accumulators over the full K; layer 0
//                   reads X, the others H.  Barrier (every wave has read H), act(acc + bias) back into H, barrier: the layers run in place.
//   output layer    wave w owns MEAN column tiles w, w + 8, ... (T of them) and the log-variance columns of the same dims (out_dim
//                   further right in the image: not tile aligned, a lane simply loads its own column).  One tile at a time: H times both
//                   column sets into R x 4 x 2 accumulators, then the head of gaussian_mlp.py:150-153 on the registers and the stores of
//                   the requested mean / logvar elements.  Nothing of the output layer goes through LDS.
//   statistics      a wave owns its mean tiles for ALL members, so m0 (the first requested member's mean) and S1 = sum_m (mean_m - m0)
//                   of its (row, column) elements live in registers across the member loop: T x R x 4 x 2.  The variance rule is the tile
//                   form's shifted one: sum_d Var_m = sum_m sum_d (mean_m - m0)^2 / n - sum_d (S1 / n)^2, never E[x^2] - E[x]^2.
// Row sums over the columns (sum_d exp(logvar), sum_d delta^2, sum_d (S1 / n)^2) run in ONE order: a lane adds its own tiles ascending,
// a fixed butterfly over the 16 lanes that share a row, one partial per wave and row into LDS, and behind a barrier thread `row` adds the
// partials in wave order 0..7.  With R fixed by the shape, a row's bits depend on the model's shape alone: not on the batch, the row's
// place in it, or the outputs requested.
// Summation order of a prediction: k ascending in ONE accumulator, then the bias.  The tile form alternates two accumulators, so the
// two forms agree to rounding, not bit for bit.  Rows past the batch and columns past the real ones are staged as zeros; padded weights
// and biases are zeros (ensemble_pack_kernel), so no loop tests a bound.
#include <hip/hip_runtime.h>

#include "agent_forms.hpp"
#include "common.hpp"
#include "ensemble_wide.hpp"
#include "lds_optin.hpp"

namespace hipets {

namespace {

static_assert(kEnsWideWaves * kWave == kPolicyThreads, "the wide ensemble kernel runs policy_layer.hpp's 512 threads");

// this wave's tiles among `tiles`: wave, wave + 8, ...
__device__ __forceinline__ int ens_wide_own(const int tiles, const int wave) {
    const int left = tiles - wave;
    return left > 0 ? (left + kEnsWideWaves - 1) / kEnsWideWaves : 0;
}

// acc[t][i] += in[16 R][kp] W[kp][hp] for this wave's `nt` column tiles n0 = 16 (wave + 8 t): lane (r, q) of acc[t][i] holds rows
// 16 i + 4 q + j of column n0 + r.  Per k-block: the weight fragments of all of the wave's tiles first (4 nt loads in flight), R
// ds_read_b128 of the input, then 4 R nt MFMAs.
template <int R, int TH>
__device__ __forceinline__ void ens_wide_hidden(const float* __restrict__ in, const int ld_in, const int kp, const float* __restrict__ W, const int hp,
                                                f32x4 (&acc)[TH][R], const int nt, const int wave, const int lane) {
    const int r = lane & 15, q = lane >> 4;
    const float* ap = in + r * ld_in + 4 * q;
    const float* wp = W + (size_t)(4 * q) * hp + wave * kTile + r;
    for (int k0 = 0; k0 < kp; k0 += kKChunk) {
        float bv[TH][4];
#pragma unroll
        for (int t = 0; t < TH; ++t) {
            if (t < nt) {
#pragma unroll
                for (int s = 0; s < 4; ++s) bv[t][s] = wp[(size_t)s * hp + t * kEnsWideWaves * kTile];
            }
        }
        f32x4 av[R];
#pragma unroll
        for (int i = 0; i < R; ++i) av[i] = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_in);
#pragma unroll
        for (int t = 0; t < TH; ++t) {
            if (t < nt) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int i = 0; i < R; ++i) acc[t][i] = mfma4(av[i][s], bv[t][s], acc[t][i]);
                }
            }
        }
        wp += (size_t)kKChunk * hp;
        ap += kKChunk;
    }
}

// U k-blocks of one mean column and its log-variance column (kGauss) per lane: cm[i] += H[16 R][16 U] W[16 U][cm_col], cl[i] likewise;
// all 4 U (8 U) weight loads are issued ahead of the MFMAs
template <int R, bool kGauss, int U>
__device__ __forceinline__ void ens_wide_out_blocks(const float* __restrict__ ap, const int ld_h, const float* __restrict__ wm, const float* __restrict__ wl,
                                                    const int npo, f32x4 (&cm)[R], f32x4 (&cl)[R]) {
    float bm[U][4], bl[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            bm[u][s] = wm[(size_t)(u * kKChunk + s) * npo];
            if (kGauss) bl[u][s] = wl[(size_t)(u * kKChunk + s) * npo];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        f32x4 av[R];
#pragma unroll
        for (int i = 0; i < R; ++i) av[i] = *reinterpret_cast<const f32x4*>(ap + i * kTile * ld_h + u * kKChunk);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                cm[i] = mfma4(av[i][s], bm[u][s], cm[i]);
                if (kGauss) cl[i] = mfma4(av[i][s], bl[u][s], cl[i]);
            }
        }
    }
}

// cm[i] = H[16 R][hp] W[hp][cm_col], cl[i] = H W[hp][cl_col] (kGauss), k ascending, two k-blocks per trip
template <int R, bool kGauss>
__device__ __forceinline__ void ens_wide_out_tile(const float* __restrict__ H, const int ld_h, const int hp, const float* __restrict__ W, const int npo,
                                                  const int cm_col, const int cl_col, f32x4 (&cm)[R], f32x4 (&cl)[R], const int lane) {
    const int r = lane & 15, q = lane >> 4;
    const float* ap = H + r * ld_h + 4 * q;
    const float* wm = W + (size_t)(4 * q) * npo + cm_col;
    const float* wl = W + (size_t)(4 * q) * npo + cl_col;
    int k0 = 0;
    for (; k0 + 2 * kKChunk <= hp; k0 += 2 * kKChunk) {
        ens_wide_out_blocks<R, kGauss, 2>(ap, ld_h, wm, wl, npo, cm, cl);
        wm += (size_t)(2 * kKChunk) * npo;
        wl += (size_t)(2 * kKChunk) * npo;
        ap += 2 * kKChunk;
    }
    if (k0 < hp) ens_wide_out_blocks<R, kGauss, 1>(ap, ld_h, wm, wl, npo, cm, cl);
}

// sum over the 16 lanes that share a row (lanes 16 q .. 16 q + 15): every lane gets the same bits
__device__ __forceinline__ float ens_wide_row_sum(float x) {
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 8);
    return x;
}

// this wave's partial of one row sum, for the rows its lanes hold: P[wave][16 i + 4 q + j]
template <int R>
__device__ __forceinline__ void ens_wide_put_partial(float* P, const f32x4 (&v)[R], const int wave, const int lane) {
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = ens_wide_row_sum(v[i][j]);
            if (r == 0) P[wave * (kTile * R) + i * kTile + 4 * q + j] = s;
        }
    }
}

// the row sum of row `row`: the waves' partials in wave order
template <int R>
__device__ __forceinline__ float ens_wide_get_sum(const float* P, const int row) {
    float v = P[row];
#pragma unroll
    for (int w = 1; w < kEnsWideWaves; ++w) v += P[w * (kTile * R) + row];
    return v;
}

// R row tiles, T mean column tiles and TH hidden column tiles per wave at most; kStats: stats requested (without: no m0 / S1 state)
template <int R, int T, int TH, bool kStats>
__global__ __launch_bounds__(kPolicyThreads) void ensemble_predict_wide_kernel(const EnsWideArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ens_wide_smem[];
    constexpr int kRows = kTile * R;
    const int ld_x = a.g.kp0 + 4, ld_h = a.g.hp + 4;
    float* X = ens_wide_smem;        // [kRows][ld_x]: the kept model input
    float* H = X + kRows * ld_x;     // [kRows][ld_h]: the hidden buffer
    float* P = H + kRows * ld_h;     // [kEnsWideSums][8][kRows]: the waves' partial row sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const long long row0 = (long long)blockIdx.x * kRows;

    // ---- the model input, once: rows past the batch and columns past in_dim are zeros ----
    const int obs_in = a.in_dim - a.act_dim;
    for (int t = tid; t < kRows * a.g.kp0; t += kPolicyThreads) {
        const int xr = t / a.g.kp0, k = t - xr * a.g.kp0;
        const long long row = row0 + xr;
        float v = 0.f;
        if (row < a.B && k < a.in_dim) {
            if (a.model_in) {
                v = a.model_in[row * a.in_dim + k];
            } else {
                v = model_input_element(a.obs + row * a.obs_dim, a.actions + row * a.act_dim, k, obs_in, a.in_dim, a.obs_process, a.cols, a.normalizer, a.norm);
            }
        }
        X[xr * ld_x + k] = v;
    }

    const int nth = ens_wide_own(a.g.hp / kTile, wave);                     // this wave's hidden column tiles
    const int ntm = ens_wide_own((a.out_dim + kTile - 1) / kTile, wave);   // and its mean column tiles
    const int act = a.activation, L = a.n_layers;
    const float slope = a.slope;
    const bool gauss = !a.deterministic;
    // the statistics' state: per (row, column) of this wave's mean tiles in registers, per row in thread `row`
    f32x4 m0[kStats ? T : 1][R], s1[kStats ? T : 1][R];
    float ssq = 0.f, sv = 0.f, max_std = 0.f, max_dev = 0.f;
    __syncthreads();  // X is complete

    for (int mi = 0; mi < a.n; ++mi) {
        const int m = a.members[mi];
        const float* w = a.w + (size_t)m * a.wmember;
        const float* b = a.b + (size_t)m * a.bmember;
        // ---- the hidden layers, in place ----
        for (int l = 0; l < L - 1; ++l) {
            const int kp = l == 0 ? a.g.kp0 : a.g.hp;
            f32x4 acc[TH][R];
#pragma unroll
            for (int t = 0; t < TH; ++t) {
#pragma unroll
                for (int i = 0; i < R; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            ens_wide_hidden<R, TH>(l == 0 ? X : H, l == 0 ? ld_x : ld_h, kp, w, a.g.hp, acc, nth, wave, lane);
            __syncthreads();  // every wave has read H (this layer's input, or the previous member's last hidden layer under its output layer)
#pragma unroll
            for (int t = 0; t < TH; ++t) {
                if (t < nth) {
                    const int n = (wave + t * kEnsWideWaves) * kTile + r;
                    const float bc = b[n];
#pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const f32x4 z = ens_activate(act, acc[t][i] + f32x4{bc, bc, bc, bc}, slope);
#pragma unroll
                        for (int j = 0; j < 4; ++j) H[(i * kTile + 4 * q + j) * ld_h + n] = z[j];
                    }
                }
            }
            __syncthreads();
            w += (size_t)kp * a.g.hp;
            b += a.g.hp;
        }
        // ---- the output layer and the head, on registers ----
        const int lvrow = a.lv_per_member ? m : 0;
        const float* mn = a.lv + (size_t)lvrow * a.out_dim;
        const float* mx = mn + (size_t)(a.lv_per_member ? a.lv_per_member : 1) * a.out_dim;
        f32x4 se[R], sd[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            se[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            sd[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t < ntm) {
                const int d = (wave + t * kEnsWideWaves) * kTile + r;  // this lane's output dim (< pad16(out_dim) <= npo)
                const bool real = d < a.out_dim;
                const int dl = (gauss && real) ? a.out_dim + d : d;  // its log-variance column (a lane past out_dim reads a column of the image and drops the result)
                f32x4 cm[R], cl[R];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    cm[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    cl[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                if (gauss) ens_wide_out_tile<R, true>(H, ld_h, a.g.hp, w, a.g.npo, d, dl, cm, cl, lane);
                else ens_wide_out_tile<R, false>(H, ld_h, a.g.hp, w, a.g.npo, d, dl, cm, cl, lane);
                const float bm = b[d], bl = b[dl];
                float lo = 0.f, hi = 0.f;
                if (gauss && real) { lo = mn[d]; hi = mx[d]; }
                // element (i, j) of this lane: row row0 + 4 q + 16 i + j, stored at at0 + (16 i + j) out_dim; live where 16 i + j < rows_left
                const size_t at0 = ((size_t)mi * a.B + (size_t)(row0 + 4 * q)) * a.out_dim + d;
                const long long left = (long long)a.B - row0 - 4 * q;
                const int rows_left = real ? (int)(left < kRows ? left : kRows) : 0;
                const bool first = mi == 0;
#pragma unroll
                for (int i = 0; i < R; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool live = i * kTile + j < rows_left;
                        const size_t at = at0 + (size_t)((i * kTile + j) * a.out_dim);
                        const float mean = real ? cm[i][j] + bm : 0.f;
                        if (live && a.mean) a.mean[at] = mean;
                        if (gauss) {
                            float lv = hi - ens_softplus(hi - (cl[i][j] + bl));
                            lv = lo + ens_softplus(lv - lo);
                            if (live && a.logvar) a.logvar[at] = lv;
                            if (kStats) se[i][j] += real ? expf(lv) : 0.f;
                        }
                        if (kStats) {  // (the first requested member: m0 = its mean, S1 = 0, nothing to the squares)
                            m0[t][i][j] = first ? mean : m0[t][i][j];
                            const float delta = first ? 0.f : mean - m0[t][i][j];
                            s1[t][i][j] = first ? 0.f : s1[t][i][j] + delta;
                            sd[i][j] += delta * delta;
                        }
                    }
                }
            }
        }
        if (kStats) {
            // (the previous member's partials were read before the barriers of this member's hidden layers)
            ens_wide_put_partial<R>(P, se, wave, lane);
            ens_wide_put_partial<R>(P + kEnsWideWaves * kRows, sd, wave, lane);
            __syncthreads();
            if (tid < kRows) {
                const float e = ens_wide_get_sum<R>(P, tid), dd = ens_wide_get_sum<R>(P + kEnsWideWaves * kRows, tid);
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
    f32x4 sq[R];
#pragma unroll
    for (int i = 0; i < R; ++i) sq[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < (kStats ? T : 1); ++t) {
        if (t < ntm) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float u = s1[t][i][j] / n;
                    sq[i][j] += u * u;
                }
            }
        }
    }
    __syncthreads();  // the last member's partials are read
    ens_wide_put_partial<R>(P, sq, wave, lane);
    __syncthreads();
    const long long row = row0 + tid;
    if (tid < kRows && row < a.B) {
        float var = ssq / n - ens_wide_get_sum<R>(P, tid);  // sum_d Var_m(mean), population
        var = var < 0.f ? 0.f : var;                         // (rounding only; a NaN stays)
        float* s = a.stats + (size_t)row * 4;
        s[0] = max_std;
        s[1] = sqrtf(var);
        s[2] = sqrtf(var + sv / n);
        s[3] = max_dev;
    }
}

using EnsWideKernel = void (*)(EnsWideArgs);

// The instances the geometry rule can ask for (ens_wide_fits): with the statistics one per T, whose state costs T x R x 8 registers;
// without them one per (R, TH) at the largest T of that pair.
EnsWideKernel ens_wide_instance(const EnsWideGeo& g, const bool stats) {
    if (g.R == 4) {  // TH <= 2, T <= 3
        if (!stats) return ensemble_predict_wide_kernel<4, 3, 2, false>;
        return g.T == 1 ? ensemble_predict_wide_kernel<4, 1, 2, true> : g.T == 2 ? ensemble_predict_wide_kernel<4, 2, 2, true> : ensemble_predict_wide_kernel<4, 3, 2, true>;
    }
    if (g.TH > 2) {  // T <= 2
        if (!stats) return ensemble_predict_wide_kernel<2, 2, 8, false>;
        return g.T == 1 ? ensemble_predict_wide_kernel<2, 1, 8, true> : ensemble_predict_wide_kernel<2, 2, 8, true>;
    }
    if (!stats) return ensemble_predict_wide_kernel<2, 4, 2, false>;
    switch (g.T) {
        case 1: return ensemble_predict_wide_kernel<2, 1, 2, true>;
        case 2: return ensemble_predict_wide_kernel<2, 2, 2, true>;
        case 3: return ensemble_predict_wide_kernel<2, 3, 2, true>;
        default: return ensemble_predict_wide_kernel<2, 4, 2, true>;
    }
}

}  // namespace

hipError_t launch_ensemble_wide(const EnsWideArgs& a, size_t lds_max, hipStream_t st) {
    static LdsOptIn opted[2][2][kEnsWideMaxT + 1];  // [R == 4][TH > 2][T, 0: without statistics]
    const bool stats = a.stats != nullptr;
    const EnsWideKernel kernel = ens_wide_instance(a.g, stats);
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
