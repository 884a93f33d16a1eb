// ensemble.hip -- what the dynamics ensemble PREDICTS, and how much its members disagree: GaussianMLP.forward(x, use_propagation=False)
// (mbrl/models/gaussian_mlp.py:140-154, 277-281; BasicEnsemble._default_forward, basic_ensemble.py:94-99) behind
// OneDTransitionRewardModel's model input (one_dim_tr_model.py:103-116), every member's mean and log-variance for a batch in one launch,
// with four uncertainty statistics reduced over the members inside it (hipets_ensemble_set / _predict / _geometry), and the elementwise
// reward penalty / halt built on one of them (hipets_uncertainty_penalty).  The kernels, then the entry points.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "agent_forms.hpp"
#include "closed_forms.hpp"
#include "common.hpp"
#include "engine.hpp"
#include "policy_layer.hpp"

namespace hipets {

namespace {

// ---------------------------------------------------------------------------------------------
// Built like the critic (value.hip) on policy_layer.hpp's scaffold: a workgroup of 512 threads owns 16 R consecutive rows, two LDS
// buffers that the layers alternate between, weights streamed from L2 as padded W[k][n] images.  The model input -- cat(obs_process(obs),
// act), normalised -- is built ONCE into a third LDS area X and kept: the members run ONE AFTER THE OTHER through the two buffers,
//   X -> buf0: h1 -> buf1: h2 -> buf0: h3 ... -> buf[(L - 1) & 1]: [mean | raw logvar]
// so the LDS need does not grow with the member count, every member reads the same input bits, and a member's weights pass through L2
// once per workgroup as the critic's do.  The buffer the last layer writes is max(hp, pad16(out_total)) wide, the other hp.
// The head -- the log-variance clamps, the outputs, the statistics -- runs on 8 consecutive lanes per row whatever R is (thread t:
// row t >> 3, columns (t & 7), (t & 7) + 8, ...): a sum over a row's columns is 8 partial sums in column order and a 3-step butterfly
// over those lanes, so a row's bits do not depend on R or on the batch it travelled in.
// Variance over the members is accumulated about the FIRST requested member's mean m0: per (row, column) LDS keeps m0 and S1 = sum_m
// (mean_m - m0); the squares' sum over the columns is one scalar per row.  sum_d Var_m = sum_m sum_d (mean_m - m0)^2 / n - sum_d (S1 / n)^2:
// the shifted values are of the size of the members' spread, so nothing cancels against the means' own size (the one-pass E[x^2] - E[x]^2
// of the raw means loses every digit the spread does not share with the mean).
// ---------------------------------------------------------------------------------------------
constexpr int kHeadLanes = 8;      // lanes of a row in the head
constexpr int kEnsMaxMembers = HIPETS_ENSEMBLE_MAX_MEMBERS, kEnsMaxIn = HIPETS_ENSEMBLE_MAX_IN, kEnsMaxOut = HIPETS_ENSEMBLE_MAX_OUT;

struct EnsArgs {
    const float *obs, *actions, *model_in;  // [B, obs_dim] and [B, act_dim], or [B, in_dim]
    float *mean, *logvar, *stats;           // [n, B, out_dim] x 2, [B, 4]; each may be null
    const float *w, *b;                     // member e at e * wmember / e * bmember; layers in order, [kp][np] each / [np] each
    const double* norm;                     // [3][in_dim]: mean, std, 1 / std
    const float* lv;                        // [lv_rows][out_dim] min, then [lv_rows][out_dim] max
    const hipets_obs_column* cols;
    size_t wmember, bmember;
    int B, n, obs_dim, act_dim, in_dim, out_dim, n_layers;
    int kp0, hp, npo;                       // in_dim, hid, out_total rounded up to 16
    int ld_x, ld0, ld1;
    int activation, obs_process, normalizer, deterministic, lv_per_member;
    float slope;
    int members[kEnsMaxMembers];            // the n requested members, in order
};

// torch.nn.functional.softplus (beta 1, threshold 20)
__device__ __forceinline__ float ens_softplus(const float x) { return x > 20.f ? x : log1pf(expf(x)); }

// sum over the 8 lanes of a row (aligned groups of 8 consecutive lanes): every lane gets the same bits
__device__ __forceinline__ float row_sum(float x) {
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 4);
    return x;
}

// torch.max's NaN rule: a NaN wins and stays
__device__ __forceinline__ float nan_max(const float acc, const float v) { return (v > acc || v != v) ? v : acc; }

template <int R>
__global__ __launch_bounds__(kPolicyThreads) void ensemble_predict_kernel(const EnsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ens_smem[];
    constexpr int kRows = kTile * R;
    float* X = ens_smem;                   // [kRows][ld_x]: the kept model input
    float* buf0 = X + kRows * a.ld_x;      // [kRows][ld0]
    float* buf1 = buf0 + kRows * a.ld0;    // [kRows][ld1]
    float* m0 = buf1 + kRows * a.ld1;      // [kRows][out_dim]: the first member's means
    float* s1 = m0 + kRows * a.out_dim;    // [kRows][out_dim]: sum_m (mean_m - m0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kRows;

    // ---- the model input, once: rows past the batch and columns past in_dim are zeros ----
    const int obs_in = a.in_dim - a.act_dim;
    for (int t = tid; t < kRows * a.kp0; t += kPolicyThreads) {
        const int r = t / a.kp0, k = t - r * a.kp0;
        const long long row = row0 + r;
        float v = 0.f;
        if (row < a.B && k < a.in_dim) {
            if (a.model_in) {
                v = a.model_in[row * a.in_dim + k];
            } else {
                v = model_input_element(a.obs + row * a.obs_dim, a.actions + row * a.act_dim, k, obs_in, a.in_dim, a.obs_process, a.cols, a.normalizer, a.norm);
            }
        }
        X[r * a.ld_x + k] = v;
    }

    // ---- the head's thread -> (row, column) map and its per-row running values ----
    const int hrow = tid / kHeadLanes, hj = tid % kHeadLanes;
    const bool head = tid < kRows * kHeadLanes;  // (whole waves: 128 R threads)
    const long long row = row0 + hrow;
    const bool live = head && row < a.B;
    const bool want_stats = a.stats != nullptr;
    float ssq = 0.f, sv = 0.f, max_std = 0.f, max_dev = 0.f;
    const int act = a.activation;
    const float slope = a.slope;
    const int L = a.n_layers;

    for (int mi = 0; mi < a.n; ++mi) {
        const int m = a.members[mi];
        const float* w = a.w + (size_t)m * a.wmember;
        const float* b = a.b + (size_t)m * a.bmember;
        // (X is complete; the previous member's head has read its buffer, which layer 0 or 1 writes again)
        __syncthreads();
        int ld_in;
        const float* in = ens_member_forward<R>(X, a.ld_x, a.kp0, a.hp, a.npo, L, w, b, buf0, a.ld0, buf1, a.ld1, act, slope, wave, lane, ld_in);
        if (!head) continue;
        // ---- the head: gaussian_mlp.py:150-153, the outputs, the member's share of the statistics ----
        const float* o = in + hrow * ld_in;
        const int lvrow = a.lv_per_member ? m : 0;
        const float* mn = a.lv + (size_t)lvrow * a.out_dim;
        const float* mx = mn + (size_t)(a.lv_per_member ? a.lv_per_member : 1) * a.out_dim;
        float se = 0.f, sd = 0.f;
        for (int d = hj; d < a.out_dim; d += kHeadLanes) {
            const float mean = o[d];
            const size_t at = ((size_t)mi * a.B + (size_t)row) * a.out_dim + d;
            if (live && a.mean) a.mean[at] = mean;
            if (!a.deterministic) {
                float lv = mx[d] - ens_softplus(mx[d] - o[a.out_dim + d]);
                lv = mn[d] + ens_softplus(lv - mn[d]);
                if (live && a.logvar) a.logvar[at] = lv;
                if (want_stats) se += expf(lv);
            }
            if (want_stats) {
                if (mi == 0) {
                    m0[hrow * a.out_dim + d] = mean;
                    s1[hrow * a.out_dim + d] = 0.f;
                } else {
                    const float delta = mean - m0[hrow * a.out_dim + d];
                    s1[hrow * a.out_dim + d] += delta;
                    sd += delta * delta;
                }
            }
        }
        if (want_stats) {
            se = row_sum(se);
            sd = row_sum(sd);
            sv += se;
            ssq += sd;
            max_std = nan_max(max_std, sqrtf(se));
            max_dev = nan_max(max_dev, sqrtf(sd));
        }
    }
    if (!head || !want_stats) return;
    // (m0 / s1 entries are read by the thread that wrote them)
    const float n = (float)a.n;
    float sq = 0.f;
    for (int d = hj; d < a.out_dim; d += kHeadLanes) {
        const float t = s1[hrow * a.out_dim + d] / n;
        sq += t * t;
    }
    sq = row_sum(sq);
    float var = ssq / n - sq;   // sum_d Var_m(mean), population
    var = var < 0.f ? 0.f : var;  // (rounding only; a NaN stays)
    if (live && hj == 0) {
        float* s = a.stats + (size_t)row * 4;
        s[0] = max_std;
        s[1] = sqrtf(var);
        s[2] = sqrtf(var + sv / n);
        s[3] = max_dev;
    }
}

// dst[e][k][n] of member images [Kp][np] at dst + e * member + off  <-  src [E, K, N]   (EnsembleLinearLayer's weight is W[k][n] already;
// a bias [E, 1, N] is K = 1).  The images were zeroed: padding stays zero.
__global__ void ensemble_pack_kernel(float* dst, const float* src, int E, int K, int N, int np, size_t member, size_t off) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)E * K * N) return;
    const int n = (int)(i % N);
    const long long ek = i / N;
    const int k = (int)(ek % K), e = (int)(ek / K);
    dst[(size_t)e * member + off + (size_t)k * np + n] = src[i];
}

// hipets_uncertainty_penalty (include/hipets.h): op by op in fp32 (the unit is compiled without contraction)
__global__ void uncertainty_penalty_kernel(const float* stats, int stat, float coef, int halt, float halt_threshold, int use_halt_reward,
                                           float halt_reward, int B, float* rewards, uint8_t* dones) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= B) return;
    const float u = stats[(size_t)row * 4 + stat];
    const float p = coef * u;
    float r = rewards[row] - p;
    if (halt && u > halt_threshold) {
        dones[row] = 1;
        if (use_halt_reward) r = halt_reward;
    }
    rewards[row] = r;
}

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_ensemble_set(hipets_engine* e, const hipets_model_desc* d, const hipets_obs_column* cols, int32_t n_cols, void* stream) {
    if (!e) return fail("null engine");
    EnsembleSnapshot& s = e->ensemble;
    s.set = false;  // (a refused set leaves no snapshot behind)
    if (!d) return fail("null argument");
    if (d->precision == HIPETS_PREC_BF16X3 || d->precision == HIPETS_PREC_BF16)
        return fail("ensemble predictions run in fp32 only: precision %s has no ensemble kernel", d->precision == HIPETS_PREC_BF16 ? "bf16" : "bf16x3");
    if (d->precision != HIPETS_PREC_F32) return fail("unknown precision %d", d->precision);
    if (d->n_layers < 2 || d->n_layers > HIPETS_MAX_LAYERS) return fail("n_layers %d outside [2, %d]", d->n_layers, HIPETS_MAX_LAYERS);
    if (d->ensemble_size < 1 || d->ensemble_size > kEnsMaxMembers) return fail("ensemble_size %d outside [1, %d]", d->ensemble_size, kEnsMaxMembers);
    if (d->n_members < 1 || d->n_members > d->ensemble_size || !d->members) return fail("n_members %d invalid for ensemble_size %d", d->n_members, d->ensemble_size);
    if (d->obs_dim < 1 || d->act_dim < 1 || d->in_dim < d->act_dim + 1 || d->hid < 1 || d->out_dim < 1) return fail("bad dimensions");
    if (d->in_dim > kEnsMaxIn) return fail("ensemble in_dim %d above %d", d->in_dim, kEnsMaxIn);
    if (d->out_dim > kEnsMaxOut) return fail("ensemble out_dim %d above %d", d->out_dim, kEnsMaxOut);
    if (d->hid > HIPETS_POLICY_MAX_HIDDEN) return fail("ensemble hidden width %d above %d", d->hid, HIPETS_POLICY_MAX_HIDDEN);
    if (d->activation < HIPETS_ACT_RELU || d->activation > HIPETS_ACT_SIGMOID) return fail("unknown activation %d", d->activation);
    if (d->normalizer < HIPETS_NORM_NONE || d->normalizer > HIPETS_NORM_F64) return fail("unknown normalizer %d", d->normalizer);
    if (d->normalizer != HIPETS_NORM_NONE && (!d->norm_mean || !d->norm_std)) return fail("normalizer stats missing");
    if (!d->deterministic && (!d->min_logvar || !d->max_logvar)) return fail("logvar bounds missing");
    if (d->ensemble_kind != HIPETS_ENSEMBLE_GAUSSIAN_MLP && d->ensemble_kind != HIPETS_ENSEMBLE_BASIC) return fail("unknown ensemble_kind %d", d->ensemble_kind);
    if (d->ensemble_kind == HIPETS_ENSEMBLE_BASIC && d->n_members != d->ensemble_size)
        return fail("BasicEnsemble has no elite subset (basic_ensemble.py:262-266): n_members %d != ensemble_size %d", d->n_members, d->ensemble_size);
    if (!d->weights || !d->biases) return fail("null argument");
    for (int l = 0; l < d->n_layers; ++l)
        if (!d->weights[l] || !d->biases[l]) return fail("layer %d: null weight or bias", l);
    for (int i = 0; i < d->n_members; ++i)
        if (d->members[i] < 0 || d->members[i] >= d->ensemble_size) return fail("member index %d out of range", d->members[i]);
    // the observation's route into the model input (what the raw-input form of hipets_ensemble_predict reads)
    const int obs_in = d->in_dim - d->act_dim;
    if (d->obs_process < HIPETS_OBS_NONE || d->obs_process > HIPETS_OBS_COLUMNS) return fail("unknown obs_process %d", d->obs_process);
    if (d->obs_process == HIPETS_OBS_COLUMNS) {
        if (!cols) return fail("obs_process COLUMNS: cols is null");
        if (n_cols < 1 || n_cols > HIPETS_MAX_OBS_COLUMNS) return fail("n_cols %d outside [1, %d]", n_cols, HIPETS_MAX_OBS_COLUMNS);
        if (obs_in != n_cols) return fail("in_dim %d != n_cols %d + act_dim %d", d->in_dim, n_cols, d->act_dim);
        for (int k = 0; k < n_cols; ++k) {
            if (cols[k].dim < 0 || cols[k].dim >= d->obs_dim) return fail("obs column %d: dim %d outside [0, %d)", k, cols[k].dim, d->obs_dim);
            if (cols[k].fn != HIPETS_COL_ID && cols[k].fn != HIPETS_COL_SIN && cols[k].fn != HIPETS_COL_COS) return fail("obs column %d: unknown fn %d", k, cols[k].fn);
        }
    } else {
        if (cols || n_cols) return fail("a column table comes with obs_process COLUMNS only (obs_process %d)", d->obs_process);
        if (obs_in != (d->obs_process == HIPETS_OBS_CARTPOLE_PETS ? d->obs_dim + 1 : d->obs_dim))
            return fail("in_dim %d inconsistent with obs_dim %d / obs_process %d / act_dim %d", d->in_dim, d->obs_dim, d->obs_process, d->act_dim);
        if (d->obs_process == HIPETS_OBS_HALFCHEETAH && d->obs_dim < 3) return fail("halfcheetah obs_process needs obs_dim >= 3");
        if (d->obs_process == HIPETS_OBS_CARTPOLE_PETS && d->obs_dim < 2) return fail("cartpole_pets obs_process needs obs_dim >= 2");
    }
    const EnsGeo x = ensemble_geo(d->in_dim, d->hid, d->out_dim, d->deterministic, d->n_layers, e->lds_max, 1);
    if (x.g.per_tile > e->lds_max)
        return fail("ensemble too wide for LDS: one row tile needs %zu bytes (input, two activation buffers, accumulators), the limit is %zu", x.g.per_tile, e->lds_max);

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const int E = d->ensemble_size, L = d->n_layers;
    size_t wmember = 0, bmember = 0;
    for (int l = 0; l < L; ++l) {
        wmember += (size_t)(l == 0 ? x.kp0 : x.hp) * (l == L - 1 ? x.npo : x.hp);
        bmember += (size_t)(l == L - 1 ? x.npo : x.hp);
    }
    if (s.w.ensure(wmember * E * 4) || s.b.ensure(bmember * E * 4)) return 1;
    HCHECK(hipMemsetAsync(s.w.p, 0, wmember * E * 4, st));
    HCHECK(hipMemsetAsync(s.b.p, 0, bmember * E * 4, st));
    size_t woff = 0, boff = 0;
    for (int l = 0; l < L; ++l) {
        const int K = l == 0 ? d->in_dim : d->hid, N = l == L - 1 ? (d->deterministic ? d->out_dim : 2 * d->out_dim) : d->hid;
        const int kp = l == 0 ? x.kp0 : x.hp, np = l == L - 1 ? x.npo : x.hp;
        const long long nw = (long long)E * K * N, nb = (long long)E * N;
        hipLaunchKernelGGL(ensemble_pack_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, s.w.as<float>(),
                           reinterpret_cast<const float*>(d->weights[l]), E, K, N, np, wmember, woff);
        hipLaunchKernelGGL(ensemble_pack_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, s.b.as<float>(),
                           reinterpret_cast<const float*>(d->biases[l]), E, 1, N, np, bmember, boff);
        woff += (size_t)kp * np;
        boff += np;
    }
    HCHECK(hipGetLastError());
    std::vector<double> norm;  // (host staging: alive until the synchronize below)
    if (d->normalizer != HIPETS_NORM_NONE) {
        norm.resize((size_t)3 * d->in_dim);
        for (int k = 0; k < d->in_dim; ++k) {
            norm[k] = d->norm_mean[k];
            norm[d->in_dim + k] = d->norm_std[k];
            norm[2 * d->in_dim + k] = 1.0 / d->norm_std[k];
        }
        if (s.norm.ensure(norm.size() * 8)) return 1;
        HCHECK(hipMemcpyAsync(s.norm.p, norm.data(), norm.size() * 8, hipMemcpyHostToDevice, st));
    }
    // the bounds by MEMBER where every member owns its own (the descriptor's rows follow its member list)
    const int lv_rows = (!d->deterministic && d->ensemble_kind == HIPETS_ENSEMBLE_BASIC) ? E : 1;
    std::vector<float> lv;
    if (!d->deterministic) {
        lv.assign((size_t)2 * lv_rows * d->out_dim, 0.f);
        for (int i = 0; i < (lv_rows > 1 ? d->n_members : 1); ++i) {
            const int at = lv_rows > 1 ? d->members[i] : 0;
            for (int c = 0; c < d->out_dim; ++c) {
                lv[(size_t)at * d->out_dim + c] = d->min_logvar[(size_t)i * d->out_dim + c];
                lv[(size_t)(lv_rows + at) * d->out_dim + c] = d->max_logvar[(size_t)i * d->out_dim + c];
            }
        }
        if (s.lv.ensure(lv.size() * 4)) return 1;
        HCHECK(hipMemcpyAsync(s.lv.p, lv.data(), lv.size() * 4, hipMemcpyHostToDevice, st));
    }
    if (d->obs_process == HIPETS_OBS_COLUMNS) {
        if (s.cols.ensure(sizeof(hipets_obs_column) * n_cols)) return 1;
        HCHECK(hipMemcpyAsync(s.cols.p, cols, sizeof(hipets_obs_column) * n_cols, hipMemcpyHostToDevice, st));
    }
    // the delta rule, for hipets_policy_rollout (a prediction itself does not read it): bit d = dim d is predicted absolutely
    uint32_t no_delta[kEnsMaxOut / 32] = {};
    for (int i = 0; d->no_delta && i < d->n_no_delta; ++i)
        if (d->no_delta[i] >= 0 && d->no_delta[i] < kEnsMaxOut) no_delta[d->no_delta[i] >> 5] |= 1u << (d->no_delta[i] & 31);
    if (s.no_delta.ensure(sizeof(no_delta))) return 1;
    HCHECK(hipMemcpyAsync(s.no_delta.p, no_delta, sizeof(no_delta), hipMemcpyHostToDevice, st));
    HCHECK(hipStreamSynchronize(st));  // the host staging and the caller's arrays may go away after return
    s.E = E; s.M = d->n_members; s.obs_dim = d->obs_dim; s.act_dim = d->act_dim; s.in_dim = d->in_dim; s.out_dim = d->out_dim;
    s.hid = d->hid; s.n_layers = L; s.activation = d->activation; s.slope = d->leaky_slope; s.obs_process = d->obs_process;
    s.normalizer = d->normalizer; s.deterministic = d->deterministic ? 1 : 0; s.lv_rows = lv_rows;
    for (int i = 0; i < d->n_members; ++i) s.members[i] = d->members[i];
    s.target_is_delta = d->target_is_delta ? 1 : 0; s.learned_rewards = d->learned_rewards ? 1 : 0;
    s.wmember = wmember; s.bmember = bmember;
    s.set = true;
    return 0;
}

int hipets_ensemble_predict(hipets_engine* e, const float* obs, const float* actions, const float* model_in, int32_t batch, int32_t only_elite,
                            float* mean, float* logvar, float* stats, void* stream) {
    if (!e || !e->ensemble.set) return fail("engine has no ensemble (call hipets_ensemble_set)");
    const EnsembleSnapshot& s = e->ensemble;
    if (model_in ? (obs || actions) : (!obs || !actions)) return fail("give either obs and actions, or model_in");
    if (batch < 1) return fail("bad batch");
    if (!mean && !logvar && !stats) return fail("no output requested");
    if (logvar && s.deterministic) return fail("a deterministic model has no log-variance head");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const EnsGeo x = ensemble_geo(e, batch);
    EnsArgs a{};
    a.obs = obs; a.actions = actions; a.model_in = model_in; a.mean = mean; a.logvar = logvar; a.stats = stats;
    a.w = s.w.as<float>(); a.b = s.b.as<float>(); a.norm = s.norm.as<double>(); a.lv = s.lv.as<float>(); a.cols = s.cols.as<hipets_obs_column>();
    a.wmember = s.wmember; a.bmember = s.bmember;
    a.B = batch; a.n = only_elite ? s.M : s.E;
    a.obs_dim = s.obs_dim; a.act_dim = s.act_dim; a.in_dim = s.in_dim; a.out_dim = s.out_dim; a.n_layers = s.n_layers;
    a.kp0 = x.kp0; a.hp = x.hp; a.npo = x.npo; a.ld_x = x.ld_x; a.ld0 = x.ld0; a.ld1 = x.ld1;
    a.activation = s.activation; a.obs_process = s.obs_process; a.normalizer = s.normalizer; a.deterministic = s.deterministic;
    a.lv_per_member = s.lv_rows > 1 ? s.lv_rows : 0;
    a.slope = s.slope;
    for (int i = 0; i < a.n; ++i) a.members[i] = only_elite ? s.members[i] : i;
    const hipError_t err = launch_mlp<ensemble_predict_kernel<4>, ensemble_predict_kernel<2>, ensemble_predict_kernel<1>>(x.g, e->lds_max, batch, a, st);
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "ensemble kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

int hipets_ensemble_geometry(hipets_engine* e, int32_t batch, int32_t* row_tiles, int32_t* lds_bytes) {
    if (!e || !e->ensemble.set) return fail("engine has no ensemble (call hipets_ensemble_set)");
    return mlp_geometry_query(batch, ensemble_geo(e, batch).g, row_tiles, lds_bytes);
}

int hipets_uncertainty_penalty(hipets_engine* e, const float* stats, int32_t stat, float coef, float halt_threshold, float halt_reward,
                               int32_t use_halt_reward, int32_t batch, float* rewards, uint8_t* dones, void* stream) {
    if (!e || !stats || !rewards) return fail("null argument");
    if (stat < 0 || stat > 3) return fail("statistic %d outside [0, 3]", stat);
    if (batch < 1) return fail("bad batch");
    const int halt = std::isnan(halt_threshold) ? 0 : 1;
    if (halt && !dones) return fail("a halt threshold needs dones");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    hipLaunchKernelGGL(uncertainty_penalty_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, stats, stat, coef, halt, halt_threshold,
                       use_halt_reward ? 1 : 0, halt_reward, batch, rewards, dones);
    HCHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
