// agent_forms.hpp -- the elementwise forms and geometries that the SAC actor kernel (policy.hip), the ensemble kernel (ensemble.hip) and
// the policy-rollout kernel (policy_rollout.hip), which runs the one inside the other, share: the actor's draws and its head
// arithmetic, one element of the ensemble's model input, the ensemble's activations, and the LDS geometry of either network.  One
// statement of each, so the fused kernel computes a step with the very operations of its two siblings.  Internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "closed_forms.hpp"
#include "common.hpp"
#include "engine.hpp"
#include "policy_layer.hpp"

namespace hipets {

namespace {

// ---- the actor (GaussianPolicy.forward / sample, third_party/pytorch_sac_pranz24/model.py:88-108) ----

// eps of (row, dims 4 blk .. 4 blk + 3): Philox4x32-10 with the counter word "POLI" where the rollouts' draws carry their step, under a
// key of its own -- no actor draw shares a (counter, key) with a model draw of the same (seed, stream)
__device__ __forceinline__ void policy_normals4(uint32_t row, uint32_t blk, unsigned long long seed, unsigned long long stream_id, float (&nrm)[4]) {
    const Philox4 r4 = philox4x32_10(row, 0x504F4C49u /* "POLI" */, blk, (uint32_t)stream_id, (uint32_t)seed,
                                     (uint32_t)(seed >> 32) ^ (uint32_t)(stream_id >> 32) ^ 0xAC7012ACu);
    box_muller(r4.x, r4.y, nrm[0], nrm[1]);
    box_muller(r4.z, r4.w, nrm[2], nrm[3]);
}

// one action dim from its two heads: tanh(mean + exp(clamped log_std) * e) * scale + bias with `sample` (Normal.rsample: loc + eps *
// scale), tanh(mean) * scale + bias without; `ls` returns the clamped log_std
__device__ __forceinline__ float policy_head_action(const float mean, const float raw_log_std, const bool sample, const float e, const float scale,
                                                    const float bias, float& ls) {
    ls = clamp_log_std(raw_log_std);
    float x = mean;
    if (sample) x = mean + expf(ls) * e;
    return tanhf(x) * scale + bias;
}

// (the actor's last layer is the two heads: columns [0, act) mean, [act, 2 act) log_std)
inline MlpGeo policy_geometry(const hipets_engine* e, long long batch) { return mlp_geometry(e->policy.obs, e->policy.hid, 2 * e->policy.act, e->lds_max, batch); }

// ---- the dynamics ensemble (OneDTransitionRewardModel._get_model_input, GaussianMLP's activation modules) ----

constexpr int kEnsAhead = 4;  // policy_layer's kAhead: k-blocks whose weight loads a wave issues ahead of their MFMAs (the critic's choice)

// element k < in_dim of the model input of (obs row, action row): obs_process including column tables, concatenation, the normaliser in
// its own dtype (util/math.py:129-143); f64 as the rollout kernel forms it: (x - mean) * (1 / std).  norm: [3][in_dim] mean, std, 1 / std
__device__ __forceinline__ float model_input_element(const float* obs_row, const float* act_row, const int k, const int obs_in, const int in_dim,
                                                     const int obs_process, const hipets_obs_column* cols, const int normalizer, const double* norm) {
    float v = k < obs_in ? processed_obs(obs_row, k, obs_process, cols) : act_row[k - obs_in];
    if (normalizer == HIPETS_NORM_F64) v = (float)(((double)v - norm[k]) * norm[2 * in_dim + k]);
    else if (normalizer == HIPETS_NORM_F32) v = (v - (float)norm[k]) / (float)norm[in_dim + k];
    return v;
}

// the activation modules of GaussianMLP (gaussian_mlp.py:88-96) on the four values a lane holds, as the rollout kernels state them
// (gemm_f32.hpp): SiLU and sigmoid through the hardware's exp2 and reciprocal, relu as a select (a NaN stays a NaN); `act` < 0: none
__device__ __forceinline__ f32x4 ens_activate(const int act, f32x4 z, const float slope) {
    constexpr float kNegLog2e = -1.44269504088896340736f;
    switch (act) {
        case HIPETS_ACT_RELU:
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = z[j] < 0.f ? 0.f : z[j];
            return z;
        case HIPETS_ACT_SILU:
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = z[j] * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(z[j] * kNegLog2e));
            return z;
        case HIPETS_ACT_LEAKY_RELU:
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = z[j] > 0.f ? z[j] : z[j] * slope;
            return z;
        case HIPETS_ACT_TANH:
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = tanhf(z[j]);
            return z;
        case HIPETS_ACT_SIGMOID:
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(z[j] * kNegLog2e));
            return z;
        default: return z;
    }
}

// one member's forward of the workgroup's rows: X -> buf0: h1 -> buf1: h2 -> buf0: h3 ... -> buf[(L - 1) & 1]: the last layer's np_last
// columns; returns that buffer and, through `ld_last`, its row length.  A barrier follows every layer; the caller's barrier precedes the
// first (X complete, the previous reader of the buffers done).  `w` / `b`: the member's images, layers in order.
template <int R>
__device__ __forceinline__ const float* ens_member_forward(const float* X, const int ld_x, const int kp0, const int hp, const int np_last, const int L,
                                                           const float* w, const float* b, float* buf0, const int ld0, float* buf1, const int ld1,
                                                           const int act, const float slope, const int wave, const int lane, int& ld_last) {
    const float* in = X;
    int ld_in = ld_x, kp = kp0;
    for (int l = 0; l < L; ++l) {
        float* out = (l & 1) ? buf1 : buf0;
        const int ld_out = (l & 1) ? ld1 : ld0;
        // (one call site for hidden and last layers: `act` < 0 is the last layer's identity)
        const bool last = l == L - 1;
        const int np = last ? np_last : hp, act_l = last ? -1 : act;
        mlp_layer_post<R, kEnsAhead>(in, ld_in, kp, w, b, np, out, ld_out, wave, lane, [act_l, slope](const f32x4 z) { return ens_activate(act_l, z, slope); });
        w += (size_t)kp * np;
        b += np;
        __syncthreads();
        in = out; ld_in = ld_out; kp = hp;
    }
    ld_last = ld_in;
    return in;
}

// LDS of the ensemble's shape: the kept input X and the two buffers (g.per_tile adds the ensemble kernel's two per-(row, column)
// accumulators: the g of hipets_ensemble_predict)
struct EnsGeo { int kp0, hp, npo, ld_x, ld0, ld1; MlpGeo g; };

inline EnsGeo ensemble_geo(int in_dim, int hid, int out_dim, int deterministic, int n_layers, size_t lds_max, long long batch) {
    EnsGeo x{};
    x.kp0 = pad16(in_dim); x.hp = pad16(hid); x.npo = pad16(deterministic ? out_dim : 2 * out_dim);
    x.ld_x = x.kp0 + 4;
    const int wide = std::max(x.hp, x.npo) + 4, narrow = x.hp + 4;
    x.ld0 = ((n_layers - 1) & 1) == 0 ? wide : narrow;  // (the last layer writes buffer (L - 1) & 1)
    x.ld1 = ((n_layers - 1) & 1) == 1 ? wide : narrow;
    x.g.kp0 = x.kp0; x.g.hp = x.hp; x.g.np_last = x.npo; x.g.ld_a = x.ld0; x.g.ld_b = x.ld1;
    x.g.per_tile = (size_t)kTile * 4 * (size_t)(x.ld_x + x.ld0 + x.ld1 + 2 * out_dim);
    x.g.R = policy_row_tiles(x.g.per_tile, lds_max, batch);
    x.g.lds = x.g.per_tile * x.g.R;
    return x;
}

inline EnsGeo ensemble_geo(const hipets_engine* e, long long batch) {
    const EnsembleSnapshot& s = e->ensemble;
    return ensemble_geo(s.in_dim, s.hid, s.out_dim, s.deterministic, s.n_layers, e->lds_max, batch);
}

}  // namespace

}  // namespace hipets
