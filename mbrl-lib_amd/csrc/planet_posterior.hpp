// planet_posterior.hpp -- the kernels of PlaNetModel.update_posterior (mbrl/models/planet.py:592-641 -> :309-347) for n_env environments:
//
//   posterior_product_kernel   one layer of the encoder's product chain as an implicit GEMM on v_mfma_f32_16x16x4_f32:
//                              Conv2d + ReLU (mbrl/models/util.py:101-157), the encoder's Linear, the encoding half of posterior[0]
//   posterior_finish_kernel    the chain's last activations, finished, as a plain [n_env, width] array (hipets_planet_encode)
//   posterior_head_kernel      BeliefModel (planet.py:82-100), posterior_transition_model (:247-252, :103-114) and the sample (:289-306)
//                              on policy_layer.hpp's LDS-MLP scaffold, 16 environments per workgroup
//
// The product kernel.  Rows are the flattened (image, oh, ow) output positions, so images share and straddle row tiles; columns are
// C_out; k = (kh kw_n + kw) C_in + c, so a k-chunk is a run of channels and a gather of channels-last activations is coalesced.  The
// weights are policy_layer.hpp's W[k][n] image (Kp x Np, zero padded), read as that layer reads them: lane (r = lane & 15, q = lane >> 4)
// loads W[16 kb + 4 q + s][n0 + r] for MFMA s of k-block kb.  A workgroup (4 waves) owns one 16-row tile, FOUR column tiles -- one per
// wave -- and one K range; grid = (row tiles, column slices, K ranges).  Per stage of kStageK k it gathers the im2col A block into LDS
// [16][kStageK + 4] (row length = 4 mod 16: the ds_read_b128 of the 16 rows x 4 groups fall on distinct banks), then every wave runs
// the stage's k-blocks, four blocks' 16 weight loads ahead of their MFMAs.  Even MFMA steps add into c0, odd ones into c1; the result is
// c0 + c1.  With one K range the epilogue adds the bias, applies ReLU and stores; with S > 1 ranges it stores the raw partial sum of
// range z at out + z split_stride and the CONSUMER -- the next launch's gather -- forms ((p0 + p1) + ... + p(S-1)) + bias, then ReLU.
// So the summation order of an output element is fixed by (K, the ranges), i.e. by the layer's shape (planet_posterior.hip deal_layer).
//
// Activations between layers are channels-last, [image][position][channel]; the first layer reads the caller's [C, H, W] image (uint8
// or f32) and normalises it on the way into LDS; the last conv layer stores in flatten(C, H, W) order, which is what nn.Linear layers
// that follow it index.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "planet.hpp"
#include "policy_layer.hpp"

namespace hipets {

namespace {

constexpr int kProdThreads = 256;
constexpr int kProdWaves = kProdThreads / kWave;
constexpr int kStageK = 256;          // k of one LDS stage: 16 k-blocks
constexpr int kStageLd = kStageK + 4;  // = 4 (mod 16)
constexpr int kProdAhead = 4;         // k-blocks whose weight loads are issued ahead of their MFMAs

enum : int { SRC_F32_IMAGE = 0, SRC_U8_IMAGE = 1, SRC_ACT = 2 };

// Where a product's input lives, as its consumer indexes it -- element (image, position, channel) at image img_stride + position
// pos_stride + channel c_stride -- and what is still to be done to a value on the way in: the pixel normalisation, or the sum over the
// producer's S partial sums (split_stride apart), its bias (of channel / bias_div: a flattened (C, H, W) array carries one per H W run) and ReLU
struct ProdSrc {
    const void* p;
    const float* bias;
    long long img_stride, split_stride;
    int kind, S, relu, bias_div, pos_stride, c_stride;
};

__device__ __forceinline__ float prod_src_load(const ProdSrc& s, const long long img, const int pos, const int c) {
    const long long i = img * s.img_stride + (long long)pos * s.pos_stride + (long long)c * s.c_stride;
    if (s.kind == SRC_U8_IMAGE) return (float)static_cast<const uint8_t*>(s.p)[i] * (1.0f / 256.0f) - 0.5f;  // planet.py:274-275
    const float* f = static_cast<const float*>(s.p);
    if (s.kind == SRC_F32_IMAGE) return f[i] * (1.0f / 256.0f) - 0.5f;
    if (s.S == 1) return f[i];  // (finished by its producer's epilogue)
    float v = f[i];
    for (int z = 1; z < s.S; ++z) v += f[(long long)z * s.split_stride + i];
    v += s.bias[c / s.bias_div];
    return (s.relu && !(v > 0.f)) ? 0.f : v;
}

struct ProdArgs {
    ProdSrc src;
    const float* w;     // [Kp][Np]
    const float* bias;  // [Np]
    float* out;
    long long M;        // rows: n_env * OH * OW
    long long o_img, split_stride;  // the store: element (image, position, channel) at image o_img + position o_pos + channel o_c
    int o_pos, o_c;
    int C_in, C_out, ksz, stride, W, OW, P;  // P = OH * OW
    int K, Kp, Np, S, kb_per_split, relu;
};

__global__ __launch_bounds__(kProdThreads) void posterior_product_kernel(const ProdArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kTile * kStageLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const long long row0 = (long long)blockIdx.x * kTile;
    const int n0 = ((int)blockIdx.y * kProdWaves + wave) * kTile;
    const bool live = n0 < a.Np;  // (wave-uniform; a wave without a column tile still gathers)
    const int kb_first = (int)blockIdx.z * a.kb_per_split;
    const int kb_last = min(kb_first + a.kb_per_split, a.Kp / kKChunk);
    // the gather: 16 threads per row, consecutive threads consecutive k
    const int g_row = tid >> 4, g_k = tid & 15;
    const long long grow = row0 + g_row;
    const bool g_ok = grow < a.M;
    const long long g_img = g_ok ? grow / a.P : 0;
    const int g_pos = g_ok ? (int)(grow - g_img * a.P) : 0;
    const int g_oh = g_pos / a.OW, g_ow = g_pos - g_oh * a.OW;
    const int g_base = g_oh * a.stride * a.W + g_ow * a.stride;  // input position of tap (0, 0)

    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    for (int ks = kb_first * kKChunk; ks < kb_last * kKChunk; ks += kStageK) {
        const int kn = min(kStageK, kb_last * kKChunk - ks);  // a multiple of 16
        for (int kk = g_k; kk < kn; kk += 16) {
            const int k = ks + kk;
            float v = 0.f;
            if (g_ok && k < a.K) {
                const int tap = k / a.C_in, c = k - tap * a.C_in;
                const int kh = tap / a.ksz, kw = tap - kh * a.ksz;
                v = prod_src_load(a.src, g_img, g_base + kh * a.W + kw, c);
            }
            As[g_row * kStageLd + kk] = v;
        }
        __syncthreads();
        if (live) {
            const float* wp = a.w + (size_t)(ks + 4 * q) * a.Np + n0 + r;
            const float* ap = As + r * kStageLd + 4 * q;
            const int nkb = kn / kKChunk;
            int kb = 0;
            for (; kb + kProdAhead <= nkb; kb += kProdAhead) {
                float bv[kProdAhead][4];
#pragma unroll
                for (int u = 0; u < kProdAhead; ++u) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) bv[u][s] = wp[(size_t)(u * kKChunk + s) * a.Np];
                }
#pragma unroll
                for (int u = 0; u < kProdAhead; ++u) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + u * kKChunk);
                    c0 = mfma4(av[0], bv[u][0], c0);
                    c1 = mfma4(av[1], bv[u][1], c1);
                    c0 = mfma4(av[2], bv[u][2], c0);
                    c1 = mfma4(av[3], bv[u][3], c1);
                }
                wp += (size_t)(kProdAhead * kKChunk) * a.Np;
                ap += kProdAhead * kKChunk;
            }
            for (; kb < nkb; ++kb) {
                const float b0 = wp[0], b1 = wp[a.Np], b2 = wp[2 * (size_t)a.Np], b3 = wp[3 * (size_t)a.Np];
                const f32x4 av = *reinterpret_cast<const f32x4*>(ap);
                c0 = mfma4(av[0], b0, c0);
                c1 = mfma4(av[1], b1, c1);
                c0 = mfma4(av[2], b2, c0);
                c1 = mfma4(av[3], b3, c1);
                wp += (size_t)kKChunk * a.Np;
                ap += kKChunk;
            }
        }
        __syncthreads();
    }
    const int n = n0 + r;
    if (!live || n >= a.C_out) return;
    const f32x4 c = c0 + c1;
    const float bc = a.bias[n];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long row = row0 + 4 * q + j;
        if (row >= a.M) continue;
        const long long img = row / a.P;
        const int pos = (int)(row - img * a.P);
        const long long at = img * a.o_img + (long long)pos * a.o_pos + (long long)n * a.o_c;
        if (a.S > 1) {
            a.out[(long long)blockIdx.z * a.split_stride + at] = c[j];
        } else {
            const float v = c[j] + bc;
            a.out[at] = (a.relu && !(v > 0.f)) ? 0.f : v;
        }
    }
}

// out[image][i] = the finished element (image, 0, i) of `src`, i < width
__global__ void posterior_finish_kernel(const ProdSrc src, float* out, const int n_env, const int width) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n_env * width) return;
    const long long img = i / width;
    out[i] = prod_src_load(src, img, 0, (int)(i - img * width));
}

// nn.Linear / nn.Conv2d weights -> W[k][n] of a zeroed [Kp][np] image, k = (kh ksz + kw) C_in + c: element (n, c, kh, kw) is read at
// src[n src_ld + (c ksz + kh) ksz + kw] (a Linear: ksz = 1, src_ld its row length; a column block of one starts at src + its first column)
__global__ void posterior_pack_kernel(float* dst, const float* src, const int N, const int C_in, const int ksz, const long long src_ld, const int np) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = C_in * ksz * ksz;
    if (i >= (long long)N * K) return;
    const int n = (int)(i / K), k = (int)(i - (long long)n * K);
    const int tap = k / C_in, c = k - tap * C_in;
    const int kh = tap / ksz, kw = tap - kh * ksz;
    dst[(size_t)k * np + n] = src[(long long)n * src_ld + ((long long)c * ksz + kh) * ksz + kw];
}

// ---------------------------------------------------------------------------------------------
// The head.  A workgroup owns 16 environments; five LDS buffers of 16 rows each, row lengths = columns + 4 (policy_layer.hpp):
//   X  [latent | action], later posterior[0]'s hidden layer      E  the embedding, later posterior[2]'s [mean | raw std]
//   Hs the belief (old, then new)                                GI, GH  the GRU's input and hidden gates (r | z | n)
//   X -> E (embed, ReLU) and Hs -> GH (hidden gates) in one barrier interval | E -> GI | GRU into Hs and belief_inout |
//   Hs -> X (posterior[0], belief half, no bias) | X = relu(X + the encoding half, which carries the bias) | X -> E (posterior[2]) |
//   latent = mean + (softplus(raw) + min_std) eps
// ---------------------------------------------------------------------------------------------
constexpr int kHeadAhead = 4;

struct HeadArgs {
    const float *w, *b;          // the head's packed images and biases
    size_t w_off[5], b_off[5];   // embed, w_ih, w_hh, posterior[0] belief half, posterior[2]
    ProdSrc p1enc;               // the encoding half of posterior[0]: element (environment, 0, column)
    const float *action, *eps;   // [n_env, action] / [n_env, latent], or null
    const uint8_t* first;        // [n_env] or null
    float *latent, *belief;      // in place
    int n_env, L, A, Hb, F;
    int xp, hbp, g3p, fp, l2p;   // pad16 of L + A, Hb, 3 Hb, F, 2 L
    int ldX, ldE, ldH, ldG;
    float min_std;
};

__global__ __launch_bounds__(kPolicyThreads) void posterior_head_kernel(const HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float head_smem[];
    float* X = head_smem;
    float* E = X + kTile * a.ldX;
    float* Hs = E + kTile * a.ldE;
    float* GI = Hs + kTile * a.ldH;
    float* GH = GI + kTile * a.ldG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int env0 = (int)blockIdx.x * kTile;
    auto fresh = [&](const int env) { return a.first != nullptr && a.first[env] != 0; };
    for (int t = tid; t < kTile * a.xp; t += kPolicyThreads) {
        const int s = t / a.xp, k = t - s * a.xp, env = env0 + s;
        float v = 0.f;
        if (env < a.n_env && !fresh(env)) {
            if (k < a.L) v = a.latent[(size_t)env * a.L + k];
            else if (k < a.L + a.A && a.action) v = a.action[(size_t)env * a.A + (k - a.L)];
        }
        X[s * a.ldX + k] = v;
    }
    for (int t = tid; t < kTile * a.hbp; t += kPolicyThreads) {
        const int s = t / a.hbp, k = t - s * a.hbp, env = env0 + s;
        Hs[s * a.ldH + k] = (env < a.n_env && k < a.Hb && !fresh(env)) ? a.belief[(size_t)env * a.Hb + k] : 0.f;
    }
    __syncthreads();
    policy_layer<1, true, kHeadAhead>(X, a.ldX, a.xp, a.w + a.w_off[0], a.b + a.b_off[0], a.hbp, E, a.ldE, wave, lane);
    policy_layer<1, false, kHeadAhead>(Hs, a.ldH, a.hbp, a.w + a.w_off[2], a.b + a.b_off[2], a.g3p, GH, a.ldG, wave, lane);
    __syncthreads();
    policy_layer<1, false, kHeadAhead>(E, a.ldE, a.hbp, a.w + a.w_off[1], a.b + a.b_off[1], a.g3p, GI, a.ldG, wave, lane);
    __syncthreads();
    // GRUCell: r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h            planet.py:98-100
    for (int t = tid; t < kTile * a.Hb; t += kPolicyThreads) {
        const int s = t / a.Hb, j = t - s * a.Hb, env = env0 + s;
        const float* gi = GI + s * a.ldG;
        const float* gh = GH + s * a.ldG;
        const float rg = sigmoid_hw(gi[j] + gh[j]);
        const float zg = sigmoid_hw(gi[a.Hb + j] + gh[a.Hb + j]);
        const float ng = tanh_hw(gi[2 * a.Hb + j] + rg * gh[2 * a.Hb + j]);
        const float hn = (1.0f - zg) * ng + zg * Hs[s * a.ldH + j];
        Hs[s * a.ldH + j] = hn;
        if (env < a.n_env) a.belief[(size_t)env * a.Hb + j] = hn;
    }
    __syncthreads();
    policy_layer<1, false, kHeadAhead>(Hs, a.ldH, a.hbp, a.w + a.w_off[3], a.b + a.b_off[3], a.fp, X, a.ldX, wave, lane);
    __syncthreads();
    for (int t = tid; t < kTile * a.F; t += kPolicyThreads) {
        const int s = t / a.F, n = t - s * a.F, env = env0 + s;
        float v = X[s * a.ldX + n];
        if (env < a.n_env) v += prod_src_load(a.p1enc, env, 0, n);
        X[s * a.ldX + n] = v > 0.f ? v : 0.f;
    }
    __syncthreads();
    policy_layer<1, false, kHeadAhead>(X, a.ldX, a.fp, a.w + a.w_off[4], a.b + a.b_off[4], a.l2p, E, a.ldE, wave, lane);
    __syncthreads();
    // MeanStdCat and _sample_state_from_params                                                        planet.py:111-114, :295-306
    for (int t = tid; t < kTile * a.L; t += kPolicyThreads) {
        const int s = t / a.L, d = t - s * a.L, env = env0 + s;
        if (env >= a.n_env) continue;
        const float mean = E[s * a.ldE + d];
        float v = mean;
        if (a.eps) v = mean + (softplus_fast(E[s * a.ldE + a.L + d]) + a.min_std) * a.eps[(size_t)env * a.L + d];
        a.latent[(size_t)env * a.L + d] = v;
    }
}

}  // namespace

}  // namespace hipets
