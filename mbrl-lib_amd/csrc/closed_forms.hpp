// closed_forms.hpp -- the elementwise closed forms around the MLP: observation preprocessing (ObsMap, processed_obs), termination
// and reward functions (term_eval, reward_eval, hopper_pair_bad), the standard normals of a (row, step, dim block)
// (rollout_normals4) and the hardware transcendentals behind the log-variance clamp (exp_hw, log_hw, softplus_fast).  Replaces
// mbrl/env/termination_fns.py, mbrl/env/reward_fns.py, the obs_process_fn of mbrl/env/pets_halfcheetah.py:91-113 and
// pets_cartpole.py:78-101, the torch.randn of Ensemble.sample_1d (mbrl/models/model.py:471-473) and F.softplus
// (gaussian_mlp.py:152-153).
#pragma once
#include "common.hpp"
#include "rollout_types.hpp"

namespace hipets {

// obs_process_fn seen from the PRODUCER of an observation dim (the fused tail, the straight form's collect phase: both hold a pair
// of raw dims in registers and write the next step's input image themselves): which input column does dim d feed, and which dim
// enters as sin / cos?  halfcheetah (env/pets_halfcheetah.py:91-113): [s1, sin s2, cos s2, s3:] -- dim 0 feeds nothing;
// cartpole_pets (env/pets_cartpole.py:78-101): [sin s1, cos s1, s0, s2:] -- one column more than dims.
template <int OBSP>
struct ObsMap {
    static constexpr int kTrigDim = OBSP == HIPETS_OBS_HALFCHEETAH ? 2 : (OBSP == HIPETS_OBS_CARTPOLE_PETS ? 1 : -1);  // enters as sin and cos
    static constexpr int kSinCol = OBSP == HIPETS_OBS_HALFCHEETAH ? 1 : 0;
    static constexpr int kCosCol = OBSP == HIPETS_OBS_HALFCHEETAH ? 2 : 1;
    // column of dim d (the sin column for the trig dim), -1 = the dim is not a model input
    __device__ static __forceinline__ int col(const int d) {
        if constexpr (OBSP == HIPETS_OBS_HALFCHEETAH) return d == 0 ? -1 : (d == 1 ? 0 : (d == 2 ? 1 : d));
        else if constexpr (OBSP == HIPETS_OBS_CARTPOLE_PETS) return d == 0 ? 2 : (d == 1 ? 0 : d + 1);
        else return d;
    }
};

// obs_process_fn(obs)[i] (mbrl/env/pets_halfcheetah.py:91-113, pets_cartpole.py:78-101)
// `cols`: the model's column table (HIPETS_OBS_COLUMNS: column i is fn_i(s[dim_i]), the same sinf / cosf as the enum forms -- a table that
// restates one of them gives its bits); the shape-specialised instances, whose mode is a compile-time enum, pass none
__device__ __forceinline__ float processed_obs(const float* s, int i, int mode, const hipets_obs_column* cols = nullptr) {
    if (mode == HIPETS_OBS_COLUMNS) {
        const hipets_obs_column col = cols[i];
        const float x = s[col.dim];
        if (col.fn == HIPETS_COL_SIN) return sinf(x);
        if (col.fn == HIPETS_COL_COS) return cosf(x);
        return x;
    }
    if (mode == HIPETS_OBS_HALFCHEETAH) {  // [s1, sin s2, cos s2, s3:]
        if (i == 0) return s[1];
        if (i == 1) return sinf(s[2]);
        if (i == 2) return cosf(s[2]);
        return s[i];
    }
    if (mode == HIPETS_OBS_CARTPOLE_PETS) {  // [sin s1, cos s1, s0, s2:]
        if (i == 0) return sinf(s[1]);
        if (i == 1) return cosf(s[1]);
        if (i == 2) return s[0];
        return s[i - 1];
    }
    return s[i];
}

// `forms`: the model's tables for the parametric forms (HIPETS_TERM_BOX here, HIPETS_REW_TERMS below); the shape-specialised instances,
// whose fn is a compile-time enum, pass none
__device__ __forceinline__ bool term_eval(const float* s, int obs_dim, int fn, const FormTables* forms = nullptr) {
    switch (fn) {
        case HIPETS_TERM_BOX: {  // include/hipets.h: every interval test holds, and (require_finite) every dim is finite; a NaN fails every test
            bool ok = true;
            if (forms->require_finite)
                for (int d = 0; d < obs_dim; ++d) ok = ok && isfinite(s[d]);
            const int n = forms->n_intervals;
            for (int k = 0; k < n; ++k) {  // (table address and k are wave-uniform)
                const hipets_term_interval iv = forms->intervals[k];
                const float x = s[iv.dim];
                ok = ok && ((iv.flags & HIPETS_BOX_LO_OPEN) ? x > iv.lo : x >= iv.lo) && ((iv.flags & HIPETS_BOX_HI_OPEN) ? x < iv.hi : x <= iv.hi);
            }
            return !ok;
        }
        case HIPETS_TERM_CARTPOLE: {  // termination_fns.py:29-44
            const float x = s[0], th = s[2], thr = (float)(12.0 * 2.0 * 3.14159265358979323846 / 360.0);
            return !((x > -2.4f) && (x < 2.4f) && (th > -thr) && (th < thr));
        }
        case HIPETS_TERM_INVERTED_PENDULUM: {  // :47-55
            bool fin = true;
            for (int d = 0; d < obs_dim; ++d) fin = fin && isfinite(s[d]);
            return !(fin && (fabsf(s[1]) <= 0.2f));
        }
        case HIPETS_TERM_HOPPER: {  // :12-26
            bool ok = true;
            for (int d = 0; d < obs_dim; ++d) ok = ok && isfinite(s[d]);
            for (int d = 1; d < obs_dim; ++d) ok = ok && (fabsf(s[d]) < 100.0f);
            return !(ok && (s[0] > 0.7f) && (fabsf(s[1]) < 0.2f));
        }
        case HIPETS_TERM_WALKER2D:  // :66-74
            return !((s[0] > 0.8f) && (s[0] < 2.0f) && (s[1] > -1.0f) && (s[1] < 1.0f));
        case HIPETS_TERM_ANT: {  // :77-85
            bool fin = true;
            for (int d = 0; d < obs_dim; ++d) fin = fin && isfinite(s[d]);
            return !(fin && (s[0] >= 0.2f) && (s[0] <= 1.0f));
        }
        case HIPETS_TERM_HUMANOID:  // :88-95
            return (s[0] < 1.0f) || (s[0] > 2.0f);
        default: return false;  // no_termination :58-63
    }
}

// (HIPETS_REW_TERMS: without the alive bonus, which needs the step's `done`: reward_alive_bonus below)
__device__ __forceinline__ float reward_eval(const float* s, const float* a, int obs_dim, int act_dim, int fn,
                                             float learned, const FormTables* forms = nullptr) {
    switch (fn) {
        case HIPETS_REW_TERMS: {  // include/hipets.h: the table's expression form, entry by entry in table order (fp32, no contraction)
            // three accumulators in three named registers (a run-time-indexed array would go to scratch).  The table address and k are
            // wave-uniform, but the entry arrives through a vector load (the kernel stores to global memory, so the compiler may not use
            // the scalar cache): the first lane's copy of every field goes to a scalar register, and fn / op / level / source select by
            // scalar branches.  A flat v9 table (every entry level 0, add, source OBS / ACT, fn <= abs: FormTables::grouped is 0) does not
            // enter the machine at all: it keeps its own short loop, so that it costs what it cost before the machine existed.
            if (!__builtin_amdgcn_readfirstlane(forms->grouped)) {  // a flat v9 table: bias + sum_k w_k f_k(e_k), the loop it always ran
                float r = forms->bias;
                const int n = forms->n_terms;
                for (int k = 0; k < n; ++k) {
                    const hipets_reward_term tm = forms->terms[k];
                    const float* v = tm.source == HIPETS_TERM_SRC_ACT ? a : s;
                    const float e = v[tm.i] - (tm.j >= 0 ? v[tm.j] : tm.c);
                    const float f = tm.fn == HIPETS_TERM_FN_SQUARE ? e * e : (tm.fn == HIPETS_TERM_FN_ABS ? fabsf(e) : e);
                    r = r + tm.w * f;
                }
                return r;
            }
            float a0 = forms->bias, a1 = 0.0f, a2 = 0.0f;
            const int n = __builtin_amdgcn_readfirstlane(forms->n_terms);
            for (int k = 0; k < n; ++k) {
                const hipets_reward_term tv = forms->terms[k];
                hipets_reward_term tm;
                tm.fn = __builtin_amdgcn_readfirstlane(tv.fn);
                tm.source = __builtin_amdgcn_readfirstlane(tv.source);
                tm.i = __builtin_amdgcn_readfirstlane(tv.i);
                tm.j = __builtin_amdgcn_readfirstlane(tv.j);
                tm.c = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tv.c)));
                tm.w = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, tv.w)));
                const int fn = HIPETS_TERM_WORD_FN(tm.fn), op = HIPETS_TERM_WORD_OP(tm.fn), level = HIPETS_TERM_WORD_LEVEL(tm.fn);
                float e;
                if (tm.source <= HIPETS_TERM_SRC_ACT) {
                    const float* v = tm.source == HIPETS_TERM_SRC_ACT ? a : s;
                    e = v[tm.i] - (tm.j >= 0 ? v[tm.j] : tm.c);
                } else if (tm.source == HIPETS_TERM_SRC_CONST) {
                    e = tm.c;
                } else if (level == 0) {  // HIPETS_TERM_SRC_GROUP: the finished deeper group, which starts over
                    e = a1 - tm.c;
                    a1 = 0.0f;
                } else {
                    e = a2 - tm.c;
                    a2 = 0.0f;
                }
                float f;
                if (fn <= HIPETS_TERM_FN_ABS) f = fn == HIPETS_TERM_FN_SQUARE ? e * e : (fn == HIPETS_TERM_FN_ABS ? fabsf(e) : e);
                else if (fn == HIPETS_TERM_FN_SIN) f = sinf(e);
                else if (fn == HIPETS_TERM_FN_COS) f = cosf(e);
                else if (fn == HIPETS_TERM_FN_EXP) f = expf(e);
                else f = sqrtf(e);
                const float t = tm.w * f;
                float acc = level == 0 ? a0 : (level == 1 ? a1 : a2);
                if (op == HIPETS_TERM_OP_ADD) acc = acc + t;
                else if (op == HIPETS_TERM_OP_MUL) acc = acc * t;
                else acc = acc / t;
                if (level == 0) a0 = acc;
                else if (level == 1) a1 = acc;
                else a2 = acc;
            }
            return a0;
        }
        case HIPETS_REW_CARTPOLE: return term_eval(s, obs_dim, HIPETS_TERM_CARTPOLE) ? 0.0f : 1.0f;  // reward_fns.py:10-13
        case HIPETS_REW_INVERTED_PENDULUM: return term_eval(s, obs_dim, HIPETS_TERM_INVERTED_PENDULUM) ? 0.0f : 1.0f;
        case HIPETS_REW_CARTPOLE_PETS: {  // :16-24
            const float e0 = (s[0] - 0.6f * sinf(s[1])) - 0.0f, e1 = (-0.6f * cosf(s[1])) - 0.6f;
            const float obs_cost = expf(-(e0 * e0 + e1 * e1) / (float)(0.6 * 0.6));
            float sq = 0.f;
            for (int i = 0; i < act_dim; ++i) sq += a[i] * a[i];
            return obs_cost + (-0.01f * sq);
        }
        case HIPETS_REW_HALFCHEETAH: {  // :33-38
            float sq = 0.f;
            for (int i = 0; i < act_dim; ++i) sq += a[i] * a[i];
            const float run = s[0] - 0.0f * (s[2] * s[2]);
            return run + (-0.1f * sq);
        }
        case HIPETS_REW_PUSHER: {  // :41-53
            const float g0 = 0.45f, g1 = -0.05f, g2 = -0.323f;
            const float tip_obj = fabsf(s[14] - s[17]) + fabsf(s[15] - s[18]) + fabsf(s[16] - s[19]);
            const float obj_goal = fabsf(g0 - s[17]) + fabsf(g1 - s[18]) + fabsf(g2 - s[19]);
            const float obs_cost = 0.5f * tip_obj + 1.25f * obj_goal;
            float sq = 0.f;
            for (int i = 0; i < act_dim; ++i) sq += a[i] * a[i];
            return -(obs_cost + 0.1f * sq);
        }
        case HIPETS_REW_NONE: return 0.0f;  // the caller evaluates its own reward_fn on the returned next_obs
        default: return learned;  // model_env.py:124-128 with reward_fn None
    }
}

// HIPETS_REW_TERMS, last op: + alive_bonus * (1 - done) with the step's own termination test (reward_fns.cartpole: (~termination_fn).float());
// a zero bonus adds nothing, so a non-finite sum keeps its bits
__device__ __forceinline__ float reward_alive_bonus(const float r, const bool done, const FormTables* forms) {
    const float bonus = forms->alive_bonus;
    return bonus != 0.0f ? r + bonus * (done ? 0.0f : 1.0f) : r;
}

// the 4 standard normals of (row, step, dim block): counter = (row, step, block, stream), key = seed
__device__ __forceinline__ void rollout_normals4(int rid, int t, int blk, unsigned long long seed,
                                                 unsigned long long stream_id, float (&nrm)[4]) {
    const Philox4 r4 = philox4x32_10((uint32_t)rid, (uint32_t)t, (uint32_t)blk, (uint32_t)stream_id, (uint32_t)seed,
                                     (uint32_t)(seed >> 32) ^ (uint32_t)(stream_id >> 32));
    box_muller(r4.x, r4.y, nrm[0], nrm[1]);
    box_muller(r4.z, r4.w, nrm[2], nrm[3]);
}

// termination_fns.hopper (:12-26) seen from ONE pair of state dims (d, d + 1): all finite, |dims 1..| < 100, height (dim 0) > 0.7,
// |angle (dim 1)| < 0.2.  The row is unhealthy iff any of its pairs says so (fused tail lanes / the collecting threads of the
// persistent DEVICE form, kspec.hpp KSpec).
__device__ __forceinline__ bool hopper_pair_bad(const int d, const float vA, const float vB, const bool hasA, const bool hasB) {
    bool bad = false;
    if (hasA) bad = !isfinite(vA) || (d >= 1 ? !(fabsf(vA) < 100.0f) : !(vA > 0.7f));
    if (hasB) bad = bad || !isfinite(vB) || !(fabsf(vB) < 100.0f) || (d == 0 && !(fabsf(vB) < 0.2f));
    return bad;
}

// Raw hardware transcendentals (v_exp_f32 / v_log_f32 are base 2, ~1 ulp, no denormal fix-up sequences).
__device__ __forceinline__ float exp_hw(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float log_hw(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994530942f; }
// log(1 + e^x) (abs error ~1e-7; F.softplus' threshold-20 branch kept as a select)
__device__ __forceinline__ float softplus_fast(float x) {
    const float y = log_hw(1.0f + exp_hw(fminf(x, 20.0f)));
    return x > 20.0f ? x : y;
}
// the log-variance clamp of GaussianMLP._default_forward (gaussian_mlp.py:152-153) between the bounds mn / mx
__device__ __forceinline__ float clamp_logvar(float lv, const float mn, const float mx) {
    lv = mx - softplus_fast(mx - lv);
    return mn + softplus_fast(lv - mn);
}

}  // namespace hipets
