// policy.hip -- the SAC Gaussian actor of an MBPO rollout (mbrl/algorithms/mbpo.py:40-47): its forward as one launch per call
// (hipets_policy_set / _act / _normals / _geometry).  The kernels, then the entry points.
//   policy_act_kernel          GaussianPolicy.forward / sample (third_party/pytorch_sac_pranz24/model.py:88-108)
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "engine.hpp"
#include "agent_forms.hpp"
#include "policy_layer.hpp"

namespace hipets {

namespace {

// The actor.  A workgroup owns 16 R consecutive rows; their activations live in two LDS buffers that the layers alternate between
// (A: obs, then h2; B: h1, then the heads), the packed weights stream from L2.  The layer, the LDS layout and the host scaffold --
// geometry, launch, packing -- are policy_layer.hpp's, shared with the critic kernel (value.hip); the draws and the head's arithmetic
// are agent_forms.hpp's, shared with the policy-rollout kernel (policy_rollout.hip).
struct PolicyArgs {
    const float* obs;      // [B, obs_dim]
    const float* eps;      // [B, act] or null
    float* actions;        // [B, act]
    float* mean_out;       // [B, act] or null
    float* log_std_out;    // [B, act] or null
    const float *w1, *w2, *wh;  // packed [kp0][hp], [hp][hp], [hp][nph]
    const float *b1, *b2, *bh;  // [hp], [hp], [nph] (zero padded)
    const float *scale, *bias;  // [act]
    int B, obs_dim, act;
    int kp0, hp, nph;  // obs_dim, hidden, 2 act rounded up to 16
    int ld_a, ld_b;
    int sample;
    unsigned long long seed, stream_id;
};

template <int R>
__global__ __launch_bounds__(kPolicyThreads) void policy_act_kernel(const PolicyArgs a) {
    extern __shared__ __attribute__((aligned(16))) float policy_smem[];
    constexpr int kRows = kTile * R;
    float* bufA = policy_smem;                  // [kRows][ld_a]
    float* bufB = policy_smem + kRows * a.ld_a;  // [kRows][ld_b]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kRows;
    mlp_stage_input<R, false>(bufA, a.ld_a, a.kp0, a.obs, a.obs_dim, nullptr, 0, a.B, row0, tid);
    __syncthreads();
    policy_layer<R, true>(bufA, a.ld_a, a.kp0, a.w1, a.b1, a.hp, bufB, a.ld_b, wave, lane);
    __syncthreads();
    policy_layer<R, true>(bufB, a.ld_b, a.hp, a.w2, a.b2, a.hp, bufA, a.ld_a, wave, lane);
    __syncthreads();
    policy_layer<R, false>(bufA, a.ld_a, a.hp, a.wh, a.bh, a.nph, bufB, a.ld_b, wave, lane);  // columns [0, act) mean, [act, 2 act) log_std
    __syncthreads();
    const int nblk = (a.act + 3) >> 2;
    for (int t = tid; t < kRows * nblk; t += kPolicyThreads) {
        const int r = t / nblk, blk = t - r * nblk;
        const long long row = row0 + r;
        if (row >= a.B) continue;
        float nrm[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.sample && !a.eps) policy_normals4((uint32_t)row, (uint32_t)blk, a.seed, a.stream_id, nrm);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int d = 4 * blk + s;
            if (d < a.act) {
                const float mean = bufB[r * a.ld_b + d];
                const long long o = row * a.act + d;
                float ls;
                a.actions[o] = policy_head_action(mean, bufB[r * a.ld_b + a.act + d], a.sample != 0, a.sample ? (a.eps ? a.eps[o] : nrm[s]) : 0.f, a.scale[d],
                                                  a.bias[d], ls);
                if (a.mean_out) a.mean_out[o] = mean;
                if (a.log_std_out) a.log_std_out[o] = ls;
            }
        }
    }
}

__global__ void policy_normals_kernel(float* out, int B, int act, unsigned long long seed, unsigned long long stream_id) {
    const int nblk = (act + 3) >> 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * nblk) return;
    const long long row = i / nblk;
    const int blk = (int)(i - row * nblk);
    float nrm[4];
    policy_normals4((uint32_t)row, (uint32_t)blk, seed, stream_id, nrm);
    for (int s = 0; s < 4; ++s) {
        const int d = 4 * blk + s;
        if (d < act) out[row * act + d] = nrm[s];
    }
}

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_policy_set(hipets_engine* e, int32_t obs_dim, int32_t hidden, int32_t act_dim, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* wm, const float* bm, const float* ws, const float* bs, const float* action_scale,
                      const float* action_bias, void* stream) {
    if (!e) return fail("null engine");
    if (!w1 || !b1 || !w2 || !b2 || !wm || !bm || !ws || !bs || !action_scale || !action_bias) return fail("null argument");
    if (check_mlp_dims("policy", obs_dim, hidden, act_dim)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    MlpSnapshot& p = e->policy;
    p.set = false; p.obs = obs_dim; p.hid = hidden; p.act = act_dim;
    const MlpGeo g = policy_geometry(e, 1);
    if (g.per_tile > e->lds_max) return fail("policy too wide for LDS");
    const size_t n1 = (size_t)g.kp0 * g.hp, n2 = (size_t)g.hp * g.hp, n3 = (size_t)g.hp * g.np_last;
    const size_t bh = (size_t)2 * g.hp, nb = bh + g.np_last + 2 * (size_t)act_dim;
    if (p.w.ensure((n1 + n2 + n3) * 4) || p.b.ensure(nb * 4)) return 1;
    const MlpLinear layers[4] = {{w1, b1, obs_dim, hidden, g.hp, 0, 0, 0},
                                 {w2, b2, hidden, hidden, g.hp, 0, n1, (size_t)g.hp},
                                 {wm, bm, hidden, act_dim, g.np_last, 0, n1 + n2, bh},
                                 {ws, bs, hidden, act_dim, g.np_last, act_dim, n1 + n2, bh + act_dim}};
    if (mlp_pack(st, p.w.as<float>(), n1 + n2 + n3, p.b.as<float>(), nb, layers, 4)) return 1;
    float* sc = p.b.as<float>() + bh + g.np_last;
    HCHECK(hipMemcpyAsync(sc, action_scale, (size_t)act_dim * 4, hipMemcpyDeviceToDevice, st));
    HCHECK(hipMemcpyAsync(sc + act_dim, action_bias, (size_t)act_dim * 4, hipMemcpyDeviceToDevice, st));
    p.set = true;
    return 0;
}

int hipets_policy_act(hipets_engine* e, const float* obs, int32_t batch, int32_t sample, uint64_t seed, uint64_t stream_id, const float* eps,
                      float* actions, float* mean_out, float* log_std_out, void* stream) {
    if (!e || !e->policy.set) return fail("engine has no policy (call hipets_policy_set)");
    if (!obs || !actions) return fail("null argument");
    if (batch < 1) return fail("bad batch");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const MlpSnapshot& p = e->policy;
    const MlpGeo g = policy_geometry(e, batch);
    const size_t n1 = (size_t)g.kp0 * g.hp, n2 = (size_t)g.hp * g.hp;
    PolicyArgs a{};
    a.obs = obs; a.eps = eps; a.actions = actions; a.mean_out = mean_out; a.log_std_out = log_std_out;
    a.w1 = p.w.as<float>(); a.w2 = a.w1 + n1; a.wh = a.w2 + n2;
    a.b1 = p.b.as<float>(); a.b2 = a.b1 + g.hp; a.bh = a.b2 + g.hp;
    a.scale = a.bh + g.np_last; a.bias = a.scale + p.act;
    a.B = batch; a.obs_dim = p.obs; a.act = p.act;
    a.kp0 = g.kp0; a.hp = g.hp; a.nph = g.np_last; a.ld_a = g.ld_a; a.ld_b = g.ld_b;
    a.sample = sample != 0;
    a.seed = seed; a.stream_id = stream_id;
    const hipError_t err = launch_mlp<policy_act_kernel<4>, policy_act_kernel<2>, policy_act_kernel<1>>(g, e->lds_max, batch, a, st);
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "policy kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

int hipets_policy_normals(hipets_engine* e, int32_t batch, int32_t act_dim, uint64_t seed, uint64_t stream_id, float* out, void* stream) {
    if (!e || !out) return fail("null argument");
    if (batch < 1) return fail("bad batch");
    if (act_dim < 1 || act_dim > HIPETS_POLICY_MAX_ACT) return fail("policy act_dim %d outside [1, %d]", act_dim, HIPETS_POLICY_MAX_ACT);
    HCHECK(hipSetDevice(e->device));
    const long long n = (long long)batch * ((act_dim + 3) / 4);
    hipLaunchKernelGGL(policy_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, batch, act_dim,
                       (unsigned long long)seed, (unsigned long long)stream_id);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_policy_geometry(hipets_engine* e, int32_t batch, int32_t* row_tiles, int32_t* lds_bytes) {
    if (!e || !e->policy.set) return fail("engine has no policy (call hipets_policy_set)");
    return mlp_geometry_query(batch, policy_geometry(e, batch), row_tiles, lds_bytes);
}

}  // extern "C"
