// value.hip -- value-bootstrapped planning objectives: the SAC critic's forward (hipets_critic_set / _q / _geometry) and the discounted,
// bootstrapped returns of a finished trajectory (hipets_discounted_returns).  The kernels, then the entry points.
//   critic_q_kernel             QNetwork.forward (third_party/pytorch_sac_pranz24/model.py:36-61), both networks in one launch
//   trajectory_returns_kernel<true> (returns_kernel.hpp)   sum_t gamma^t r_t + gamma^H v over rewards / dones [H, B], then the engine's
//                               particle reduction
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "engine.hpp"
#include "policy_layer.hpp"
#include "returns_kernel.hpp"

namespace hipets {

namespace {

// ---------------------------------------------------------------------------------------------
// The critic.  Built like the actor (policy.hip) on policy_layer.hpp's layer and host scaffold: a workgroup owns 16 R consecutive rows,
// two LDS buffers that the layers alternate between.  The input [s, a] exists in LDS only: buffer A is filled from the two source
// arrays, zero padded to pad16(obs + act) columns.  The two networks run ONE AFTER THE OTHER through the same two buffers:
//   A: [s, a]  -> B: h1 -> A: h2 -> B: column 0 = q      (Q1: linear1..3; then A is filled again and Q2 runs: linear4..6)
// so the LDS need is the actor's -- 16 R rows x (max(pad16(obs + act), hp) + 4 + hp + 4) floats -- and every shape inside the
// HIPETS_POLICY_MAX_* limits runs with R >= 1 (obs 512 + act 32, hidden 1024: 131 584 bytes).  A row's q1 waits in a register of the
// thread that writes the row's outputs while Q2 runs.  The last layer is one 16-column tile (column 0 real), i.e. one wave's work.
// ---------------------------------------------------------------------------------------------
// k-blocks whose weight loads a wave issues ahead of their MFMAs (policy_layer's kAhead).  At one workgroup per CU (the LDS) a CU holds 8
// waves; with the plain loop's 4 loads in flight per wave the launch is bound by L2 latency (hidden 1024: 4.28 ms at 10 000 rows).
constexpr int kCriticAhead = 4;

struct CriticArgs {
    const float* obs;      // [B, obs_dim]
    const float* actions;  // [B, act]
    float *q1, *q2, *qmin;  // [B] each, or null
    const float* w;        // packed, per network: [kp0][hp], [hp][hp], [hp][16]
    const float* b;        // per network: [hp], [hp], [16] (zero padded)
    int B, obs_dim, act;
    int kp0, hp;  // obs_dim + act, hidden rounded up to 16
    int ld_a, ld_b;
};

// q of this workgroup's row `tid` (threads tid < 16 R; the others return 0) through network `net` (0: linear1..3, 1: linear4..6)
template <int R>
__device__ __forceinline__ float critic_net(const CriticArgs& a, const int net, float* bufA, float* bufB, const long long row0, const int tid) {
    constexpr int kRows = kTile * R;
    const int lane = tid & 63, wave = tid >> 6;
    const size_t n1 = (size_t)a.kp0 * a.hp, n2 = (size_t)a.hp * a.hp, nw = n1 + n2 + (size_t)a.hp * kTile;
    const float* w = a.w + net * nw;
    const float* b = a.b + net * (2 * a.hp + kTile);
    // [s, a].  (The previous network's last layer read A before its closing barrier, and nothing reads B between that barrier and the
    // next one.)
    mlp_stage_input<R, true>(bufA, a.ld_a, a.kp0, a.obs, a.obs_dim, a.actions, a.act, a.B, row0, tid);
    __syncthreads();
    policy_layer<R, true, kCriticAhead>(bufA, a.ld_a, a.kp0, w, b, a.hp, bufB, a.ld_b, wave, lane);
    __syncthreads();
    policy_layer<R, true, kCriticAhead>(bufB, a.ld_b, a.hp, w + n1, b + a.hp, a.hp, bufA, a.ld_a, wave, lane);
    __syncthreads();
    policy_layer<R, false, kCriticAhead>(bufA, a.ld_a, a.hp, w + n1 + n2, b + 2 * a.hp, kTile, bufB, a.ld_b, wave, lane);
    __syncthreads();
    return tid < kRows ? bufB[tid * a.ld_b] : 0.f;  // (read before the next network's first barrier: B is written only behind it)
}

template <int R>
__global__ __launch_bounds__(kPolicyThreads) void critic_q_kernel(const CriticArgs a) {
    extern __shared__ __attribute__((aligned(16))) float critic_smem[];
    constexpr int kRows = kTile * R;
    float* bufA = critic_smem;                  // [kRows][ld_a]
    float* bufB = critic_smem + kRows * a.ld_a;  // [kRows][ld_b]
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * kRows;
    const float q1 = critic_net<R>(a, 0, bufA, bufB, row0, tid);
    const float q2 = critic_net<R>(a, 1, bufA, bufB, row0, tid);
    const long long row = row0 + tid;
    if (tid < kRows && row < a.B) {
        if (a.q1) a.q1[row] = q1;
        if (a.q2) a.q2[row] = q2;
        // torch.min(q1, q2) as a select: the smaller one, q2 on a tie, NaN when either is NaN
        if (a.qmin) a.qmin[row] = (q1 < q2 || q1 != q1) ? q1 : q2;
    }
}

// (the last layer is one 16-column tile, column 0 real)
MlpGeo critic_geometry(const hipets_engine* e, long long batch) { return mlp_geometry(e->critic.obs + e->critic.act, e->critic.hid, kTile, e->lds_max, batch); }

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_critic_set(hipets_engine* e, int32_t obs_dim, int32_t act_dim, int32_t hidden, const void* ptrs, int32_t n_ptrs, void* stream) {
    if (!e) return fail("null engine");
    e->critic.set = false;  // (a refused set leaves no critic behind)
    if (!ptrs) return fail("null argument");
    if (n_ptrs != HIPETS_CRITIC_N_PTRS) return fail("critic pointer table holds %d entries, expected %d", n_ptrs, HIPETS_CRITIC_N_PTRS);
    if (check_mlp_dims("critic", obs_dim, hidden, act_dim)) return 1;
    const float* const* p = static_cast<const float* const*>(ptrs);
    for (int i = 0; i < HIPETS_CRITIC_N_PTRS; ++i)
        if (!p[i]) return fail("critic pointer %d is null", i);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    MlpSnapshot& c = e->critic;
    c.obs = obs_dim; c.act = act_dim; c.hid = hidden;
    const MlpGeo g = critic_geometry(e, 1);
    if (g.per_tile > e->lds_max) return fail("critic too wide for LDS");
    const size_t n1 = (size_t)g.kp0 * g.hp, n2 = (size_t)g.hp * g.hp, n3 = (size_t)g.hp * kTile, nw = n1 + n2 + n3;
    const size_t nb = (size_t)2 * g.hp + kTile;
    if (c.w.ensure(2 * nw * 4) || c.b.ensure(2 * nb * 4)) return 1;
    const int K = obs_dim + act_dim;
    MlpLinear layers[6];
    for (int net = 0; net < 2; ++net) {
        const float* const* l = p + 6 * net;  // linear(3 net + 1..3): weight, bias each
        layers[3 * net + 0] = {l[0], l[1], K, hidden, g.hp, 0, net * nw, net * nb};
        layers[3 * net + 1] = {l[2], l[3], hidden, hidden, g.hp, 0, net * nw + n1, net * nb + g.hp};
        layers[3 * net + 2] = {l[4], l[5], hidden, 1, kTile, 0, net * nw + n1 + n2, net * nb + 2 * g.hp};
    }
    if (mlp_pack(st, c.w.as<float>(), 2 * nw, c.b.as<float>(), 2 * nb, layers, 6)) return 1;
    c.set = true;
    return 0;
}

int hipets_critic_q(hipets_engine* e, const float* obs, const float* actions, int32_t batch, float* q1, float* q2, float* qmin, void* stream) {
    if (!e || !e->critic.set) return fail("engine has no critic (call hipets_critic_set)");
    if (!obs || !actions) return fail("null argument");
    if (batch < 1) return fail("bad batch");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const MlpGeo g = critic_geometry(e, batch);
    CriticArgs a{};
    a.obs = obs; a.actions = actions; a.q1 = q1; a.q2 = q2; a.qmin = qmin;
    a.w = e->critic.w.as<float>(); a.b = e->critic.b.as<float>();
    a.B = batch; a.obs_dim = e->critic.obs; a.act = e->critic.act;
    a.kp0 = g.kp0; a.hp = g.hp; a.ld_a = g.ld_a; a.ld_b = g.ld_b;
    const hipError_t err = launch_mlp<critic_q_kernel<4>, critic_q_kernel<2>, critic_q_kernel<1>>(g, e->lds_max, batch, a, st);
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "critic kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

int hipets_critic_geometry(hipets_engine* e, int32_t batch, int32_t* row_tiles, int32_t* lds_bytes) {
    if (!e || !e->critic.set) return fail("engine has no critic (call hipets_critic_set)");
    return mlp_geometry_query(batch, critic_geometry(e, batch), row_tiles, lds_bytes);
}

int hipets_discounted_returns(hipets_engine* e, const float* rewards, const uint8_t* dones, const float* terminal_values, float gamma, int32_t pop,
                              int32_t H, int32_t P, float* returns, float* row_totals, int32_t* first_done, void* stream) {
    if (!e || !rewards || !dones || !returns) return fail("null argument");
    if (pop < 1 || H < 1 || P < 1) return fail("bad pop/horizon/particles");
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail("discount %g outside [0, 1]", (double)gamma);
    const long long B = (long long)pop * P;
    if (B > 0x7FFFFFFF) return fail("batch too large");
    if (check_reduce(e, P)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);  // (the two-pass form below may run on the engine's row totals)
    // (gamma == 1 without values IS hipets_trajectory_returns: the same instantiation of the same kernel, not an equal one)
    if (gamma == 1.0f && !terminal_values)
        return launch_trajectory_returns<false>(e, rewards, dones, nullptr, 1.0f, pop, H, P, returns, row_totals, first_done, st);
    return launch_trajectory_returns<true>(e, rewards, dones, terminal_values, gamma, pop, H, P, returns, row_totals, first_done, st);
}

}  // extern "C"
