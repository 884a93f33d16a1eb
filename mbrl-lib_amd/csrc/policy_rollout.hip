// policy_rollout.hip -- the SAC actor rolled through the dynamics ensemble, the action sequences that LOOP and TD-MPC put into every
// planning iteration's population: H steps of  a_t = GaussianPolicy(s_t),  s_{t+1} = the ensemble's expected next observation of (s_t,
// a_t)  (ModelEnv.step(..., sample=False) under propagation_method="expectation": gaussian_mlp.py:213-215, basic_ensemble.py:131-136,
// one_dim_tr_model.py:281-286) as ONE launch (hipets_policy_rollout / _geometry) over the snapshots hipets_policy_set and
// hipets_ensemble_set hold.  The kernel, then the entry points.
#include <hip/hip_runtime.h>

#include "agent_forms.hpp"
#include "common.hpp"
#include "engine.hpp"
#include "policy_layer.hpp"

namespace hipets {

namespace {

// A workgroup of kPolicyThreads owns 16 R consecutive rows for the whole horizon: no workgroup reads what another wrote, there is no
// poll and no hand-over, so the kernel cannot wait.  A step is policy_act_kernel's three layers and head, then ensemble_predict_kernel's
// input builder and member loop, each through the very functions of those kernels (policy_layer.hpp, agent_forms.hpp): a row's action
// has the bits hipets_policy_act gives for its state, a member's mean the bits hipets_ensemble_predict gives for (state, action).
//   LDS   S    [16 R][ld_s]     the state, zero padded to the actor's first k-blocks: the actor's input as it stands
//         ACT  [16 R][ld_act]   the step's action
//         U    the larger of    the actor's  A [16 R][ld_a] (h2), B [16 R][ld_b] (h1, then the heads)
//                               the model's  X [16 R][ld_x] (the kept input), buf0 [16 R][ld0], buf1 [16 R][ld1], ACC [16 R][out_dim]
// The two networks never run at once: the actor's buffers are dead once ACT is written, the model's once S is, so they share U.
// ACC: the requested members' means summed in requested order (acc = m_0; acc += m_i), divided once by their count.
struct PolicyRolloutArgs {
    const float* s0;     // [n, obs_dim]
    const float* eps;    // [H, n, act] or null
    float* actions;      // [n, H, act]
    float* states;       // [H + 1, n, obs_dim] or null
    // the actor (hipets_policy_set's images)
    const float *w1, *w2, *wh, *b1, *b2, *bh, *scale, *bias;
    int obs_dim, act, kp0a, hpa, nph, ld_s, ld_act, ld_a, ld_b;
    // the ensemble (hipets_ensemble_set's images)
    const float *w, *b;
    const double* norm;
    const hipets_obs_column* cols;
    const uint32_t* no_delta;  // bit d: observation dim d is predicted absolutely
    size_t wmember, bmember;
    int n_members, in_dim, out_dim, n_layers, kp0, hp, npo, ld_x, ld0, ld1, activation, obs_process, normalizer, target_is_delta;
    float slope;
    int members[HIPETS_ENSEMBLE_MAX_MEMBERS];
    int n, H, mean_rows;
    unsigned long long seed, stream_id;
};

template <int R>
__global__ __launch_bounds__(kPolicyThreads) void policy_rollout_kernel(const PolicyRolloutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rollout_smem[];
    constexpr int kRows = kTile * R;
    float* S = rollout_smem;
    float* ACT = S + kRows * a.ld_s;
    float* U = ACT + kRows * a.ld_act;
    float* bufA = U;
    float* bufB = bufA + kRows * a.ld_a;
    float* X = U;
    float* buf0 = X + kRows * a.ld_x;
    float* buf1 = buf0 + kRows * a.ld0;
    float* ACC = buf1 + kRows * a.ld1;
    const int tid0 = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * kRows;
    const int obs_in = a.in_dim - a.act;
    const float count = (float)a.n_members;

    // the start state: mlp_stage_input's form (zero padded columns, zero rows past the batch), also states[0]
    mlp_stage_input<R, false>(S, a.ld_s, a.kp0a, a.s0, a.obs_dim, nullptr, 0, a.n, row0, tid0);
    if (a.states) {
        for (int t = tid0; t < kRows * a.obs_dim; t += kPolicyThreads) {
            const int r = t / a.obs_dim, d = t - r * a.obs_dim;
            const long long row = row0 + r;
            if (row < a.n) a.states[(size_t)row * a.obs_dim + d] = a.s0[(size_t)row * a.obs_dim + d];
        }
    }
    __syncthreads();

    for (int step = 0; step < a.H; ++step) {
        // (the thread index is made opaque once per step: what a step's element loops derive from it -- quotients, LDS addresses -- is
        // then not hoisted out of the horizon loop and kept alive across the layers, which at R = 4 took the kernel past 256 VGPRs
        // into scratch memory)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = tid >> 6;
        // ---- the actor: policy_act_kernel with S as its input buffer ----
        // (the plain k loop, as there: issuing four k-blocks of weight loads ahead, policy_layer's kAhead = 4, was measured and changed
        // nothing -- 1.62 against 1.49 ms at n = 24, H = 5; 8.63 against 9.16 ms at H = 30)
        policy_layer<R, true>(S, a.ld_s, a.kp0a, a.w1, a.b1, a.hpa, bufB, a.ld_b, wave, lane);
        __syncthreads();
        policy_layer<R, true>(bufB, a.ld_b, a.hpa, a.w2, a.b2, a.hpa, bufA, a.ld_a, wave, lane);
        __syncthreads();
        policy_layer<R, false>(bufA, a.ld_a, a.hpa, a.wh, a.bh, a.nph, bufB, a.ld_b, wave, lane);  // columns [0, act) mean, [act, 2 act) log_std
        __syncthreads();
        const int nblk = (a.act + 3) >> 2;
        for (int t = tid; t < kRows * nblk; t += kPolicyThreads) {
            const int r = t / nblk, blk = t - r * nblk;
            const long long row = row0 + r;
            if (row >= a.n) continue;
            const bool sample = row >= a.mean_rows;
            const long long draw_row = (long long)step * a.n + row;  // the row of the [H, n, act] table
            float nrm[4] = {0.f, 0.f, 0.f, 0.f};
            if (sample && !a.eps) policy_normals4((uint32_t)draw_row, (uint32_t)blk, a.seed, a.stream_id, nrm);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int d = 4 * blk + s;
                if (d < a.act) {
                    float ls;
                    const float e = sample ? (a.eps ? a.eps[(size_t)draw_row * a.act + d] : nrm[s]) : 0.f;
                    const float action = policy_head_action(bufB[r * a.ld_b + d], bufB[r * a.ld_b + a.act + d], sample, e, a.scale[d], a.bias[d], ls);
                    ACT[r * a.ld_act + d] = action;
                    a.actions[((size_t)row * a.H + step) * a.act + d] = action;
                }
            }
        }
        __syncthreads();  // (the heads are read: U is the model's from here)

        // ---- the model input, as ensemble_predict_kernel builds it: padded columns and rows past the batch are zeros ----
        for (int t = tid; t < kRows * a.kp0; t += kPolicyThreads) {
            const int r = t / a.kp0, k = t - r * a.kp0;
            float v = 0.f;
            if (row0 + r < a.n && k < a.in_dim)
                v = model_input_element(S + r * a.ld_s, ACT + r * a.ld_act, k, obs_in, a.in_dim, a.obs_process, a.cols, a.normalizer, a.norm);
            X[r * a.ld_x + k] = v;
        }

        // ---- the requested members one after the other; their mean heads summed in requested order ----
        for (int mi = 0; mi < a.n_members; ++mi) {
            const int m = a.members[mi];
            // (X is complete; the previous member's means are summed, their buffer may be written again)
            __syncthreads();
            int ld_o;
            const float* o = ens_member_forward<R>(X, a.ld_x, a.kp0, a.hp, a.npo, a.n_layers, a.w + (size_t)m * a.wmember, a.b + (size_t)m * a.bmember, buf0,
                                                   a.ld0, buf1, a.ld1, a.activation, a.slope, wave, lane, ld_o);
            for (int t = tid; t < kRows * a.out_dim; t += kPolicyThreads) {
                const int r = t / a.out_dim, d = t - r * a.out_dim;
                const float mean = o[r * ld_o + d];
                ACC[t] = mi == 0 ? mean : ACC[t] + mean;
            }
        }
        __syncthreads();

        // ---- the next state (one_dim_tr_model.py:281-286): the learned-reward column, the last, is not read ----
        for (int t = tid; t < kRows * a.obs_dim; t += kPolicyThreads) {
            const int r = t / a.obs_dim, d = t - r * a.obs_dim;
            const long long row = row0 + r;
            if (row >= a.n) continue;  // (a row past the batch stays zeros)
            const float pred = ACC[r * a.out_dim + d] / count;
            const bool delta = a.target_is_delta && !((a.no_delta[d >> 5] >> (d & 31)) & 1u);
            const float next = delta ? S[r * a.ld_s + d] + pred : pred;
            S[r * a.ld_s + d] = next;
            if (a.states) a.states[((size_t)(step + 1) * a.n + (size_t)row) * a.obs_dim + d] = next;
        }
        __syncthreads();
    }
}

// LDS and row tiles of a rollout of `batch` rows over the two snapshots (g.R, g.lds, g.per_tile: what launch_mlp and the query read)
struct RolloutGeo { MlpGeo g, actor; EnsGeo x; int ld_s, ld_act, ld_a, ld_b; };

RolloutGeo rollout_geo(const hipets_engine* e, long long batch) {
    RolloutGeo r{};
    r.actor = policy_geometry(e, 1);
    r.x = ensemble_geo(e, 1);
    r.ld_s = r.actor.kp0 + 4;
    r.ld_act = (e->policy.act + 3) & ~3;
    r.ld_a = r.actor.hp + 4;                               // (h2 alone: the actor's input is S)
    r.ld_b = std::max(r.actor.hp, r.actor.np_last) + 4;
    const int actor_floats = r.ld_a + r.ld_b, model_floats = r.x.ld_x + r.x.ld0 + r.x.ld1 + e->ensemble.out_dim;
    r.g.per_tile = (size_t)kTile * 4 * (size_t)(r.ld_s + r.ld_act + std::max(actor_floats, model_floats));
    r.g.R = policy_row_tiles(r.g.per_tile, e->lds_max, batch);
    r.g.lds = r.g.per_tile * r.g.R;
    return r;
}

// what both entry points refuse about the two snapshots, before any argument of a call is looked at
int check_snapshots(const hipets_engine* e) {
    if (!e) return fail("null engine");
    if (!e->policy.set) return fail("engine has no policy (call hipets_policy_set)");
    if (!e->ensemble.set) return fail("engine has no ensemble (call hipets_ensemble_set)");
    const MlpSnapshot& p = e->policy;
    const EnsembleSnapshot& s = e->ensemble;
    if (p.obs != s.obs_dim || p.act != s.act_dim)
        return fail("the policy's (obs %d, act %d) differs from the ensemble's (obs_dim %d, act_dim %d)", p.obs, p.act, s.obs_dim, s.act_dim);
    if (s.out_dim != s.obs_dim + s.learned_rewards)
        return fail("the ensemble's out_dim %d is not obs_dim %d + learned_rewards %d: its prediction is no next observation", s.out_dim, s.obs_dim, s.learned_rewards);
    const RolloutGeo r = rollout_geo(e, 1);
    if (r.g.per_tile > e->lds_max)
        return fail("policy rollout too wide for LDS: one row tile needs %zu bytes (state, action, the larger of the actor's and the model's buffers), the limit is %zu",
                    r.g.per_tile, e->lds_max);
    return 0;
}

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_policy_rollout(hipets_engine* e, const float* s0, int32_t n, int32_t horizon, int32_t mean_rows, int32_t only_elite, uint64_t seed,
                          uint64_t stream_id, const float* eps, float* actions, float* states, void* stream) {
    if (check_snapshots(e)) return 1;
    if (!s0 || !actions) return fail("null argument");
    if (n < 1) return fail("bad n %d", n);
    if (horizon < 1) return fail("bad horizon %d", horizon);
    if ((long long)n * horizon > 0x7fffffffll) return fail("horizon %d x n %d rows of draws exceed 2^31 - 1", horizon, n);
    if (mean_rows < 0 || mean_rows > n) return fail("mean_rows %d outside [0, %d]", mean_rows, n);
    const MlpSnapshot& p = e->policy;
    const EnsembleSnapshot& s = e->ensemble;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const RolloutGeo r = rollout_geo(e, n);
    const size_t n1 = (size_t)r.actor.kp0 * r.actor.hp, n2 = (size_t)r.actor.hp * r.actor.hp;
    PolicyRolloutArgs a{};
    a.s0 = s0; a.eps = eps; a.actions = actions; a.states = states;
    a.w1 = p.w.as<float>(); a.w2 = a.w1 + n1; a.wh = a.w2 + n2;
    a.b1 = p.b.as<float>(); a.b2 = a.b1 + r.actor.hp; a.bh = a.b2 + r.actor.hp;
    a.scale = a.bh + r.actor.np_last; a.bias = a.scale + p.act;
    a.obs_dim = p.obs; a.act = p.act; a.kp0a = r.actor.kp0; a.hpa = r.actor.hp; a.nph = r.actor.np_last;
    a.ld_s = r.ld_s; a.ld_act = r.ld_act; a.ld_a = r.ld_a; a.ld_b = r.ld_b;
    a.w = s.w.as<float>(); a.b = s.b.as<float>(); a.norm = s.norm.as<double>(); a.cols = s.cols.as<hipets_obs_column>();
    a.no_delta = s.no_delta.as<uint32_t>();
    a.wmember = s.wmember; a.bmember = s.bmember;
    a.n_members = only_elite ? s.M : s.E;
    a.in_dim = s.in_dim; a.out_dim = s.out_dim; a.n_layers = s.n_layers;
    a.kp0 = r.x.kp0; a.hp = r.x.hp; a.npo = r.x.npo; a.ld_x = r.x.ld_x; a.ld0 = r.x.ld0; a.ld1 = r.x.ld1;
    a.activation = s.activation; a.obs_process = s.obs_process; a.normalizer = s.normalizer; a.target_is_delta = s.target_is_delta;
    a.slope = s.slope;
    for (int i = 0; i < a.n_members; ++i) a.members[i] = only_elite ? s.members[i] : i;
    a.n = n; a.H = horizon; a.mean_rows = mean_rows;
    a.seed = seed; a.stream_id = stream_id;
    const hipError_t err = launch_mlp<policy_rollout_kernel<4>, policy_rollout_kernel<2>, policy_rollout_kernel<1>>(r.g, e->lds_max, n, a, st);
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "policy rollout kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

int hipets_policy_rollout_geometry(hipets_engine* e, int32_t n, int32_t* row_tiles, int32_t* lds_bytes) {
    if (check_snapshots(e)) return 1;
    return mlp_geometry_query(n, rollout_geo(e, n).g, row_tiles, lds_bytes);
}

}  // extern "C"
