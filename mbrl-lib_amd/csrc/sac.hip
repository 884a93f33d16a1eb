// sac.hip -- one SAC update (mbrl/third_party/pytorch_sac_pranz24/sac.py:76-173) as a fixed sequence of ordinary launches, in place on
// the live torch tensors (hipets_sac_bind / hipets_sac_update / hipets_sac_forward_taps, include/hipets.h).  The kernels, then the
// entry points.
//   sac_mm_kernel        up to kSacMaxProblems strided products C = A . B per launch, a 16 x 16 tile per wave, one epilogue per launch:
//                        bias (+ relu), relu mask (the dz chain), plain store, or torch-order Adam (+ the target's soft update)
//   sac_policy_tail_kernel / sac_policy_tail_bwd_kernel   GaussianPolicy.sample behind its heads (model.py:95-108) and its gradient
//   sac_q_tail_kernel    the N = 1 output layers of the Q-networks, fused with the TD target / the policy's min-Q and their gradients
//   sac_finish_kernel    the losses, the Adam step on log_alpha, the result slot
// Every product runs on v_mfma_f32_16x16x4_f32 through the compiler's builtin: sac_seg_acc is the k-loop, tile_walk.hpp the tiles'
// numbering and the lane-to-element map, adam.hpp the optimizers' rule (on the host and on the device).  Launch order is the only
// synchronisation: no kernel waits on another workgroup; no float atomics: every reduction has a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "adam.hpp"
#include "common.hpp"
#include "engine.hpp"
#include "policy_layer.hpp"
#include "tile_walk.hpp"
#include "transition_layout.hpp"

namespace hipets {

namespace {

constexpr int kSacThreads = 256;
constexpr int kSacWaves = kSacThreads / kWave;
constexpr int kSacMaxProblems = 12;

enum SacEpilogue { kEpiBiasRelu = 0, kEpiBias = 1, kEpiMask = 2, kEpiStore = 3, kEpiAdam = 4 };

// one contraction segment: element (i, k) of A at A[i * sam + k * sak], (k, j) of B at B[k * sbk + j * sbn], k < K
struct SacSeg {
    const float* A;
    const float* B;
    int sam, sak, sbk, sbn, K;
};

// C [M, N] = sum over the segments (a split k: [state, action] is never concatenated); C(i, j) at out[i * ldo + j]
struct SacProblem {
    SacSeg s[2];
    float* out;
    const float* aux;  // bias [N] (kEpiBias*), or the activations [M, ldo] whose sign masks the result (kEpiMask)
    float *m, *v;      // kEpiAdam: exp_avg / exp_avg_sq of `out`
    float* target;     // kEpiAdam: the target network's copy of `out`, or null
    int nseg, M, N, ldo, tiles_n;
};

struct SacMmArgs {
    SacProblem p[kSacMaxProblems];
    int tile_start[kSacMaxProblems + 1];
    int np, epilogue;
    AdamScalars adam;
    int soft;  // kEpiAdam: apply target = target * (1 - tau) + param * tau with the new parameter value
    float tau, one_minus_tau;
};

// the operands of k = k .. k + 3 of one row / column: one 16-byte load where k is the contiguous direction and the row is aligned
__device__ __forceinline__ f32x4 sac_ld4(const float* __restrict__ row, int sk, int k, int K, bool valid, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!valid) return v;
    if (vec && k + 4 <= K) return *reinterpret_cast<const f32x4*>(row + k);
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = k + s < K ? row[(int64_t)(k + s) * sk] : 0.f;
    return v;
}

// c0 / c1 += one segment's share of the 16 x 16 tile at (m0, n0).  Inside a k-block of 16 lane group q = lane >> 4 supplies
// k = 16 kb + 4 q + s to MFMA s, for A and B alike; the result lies as tile_walk.hpp says.
// (train.hip's mm_tile is the other k-loop of the learning kernels and stays apart: it gives lane group q the steps k0 + q, k0 + 4 + q,
// ... one float per load, so the two sum along k in different orders -- other bits -- and load differently -- other speed.)
__device__ __forceinline__ void sac_seg_acc(f32x4& c0, f32x4& c1, const SacSeg& s, int M, int N, int m0, int n0, int lane) {
    const int r = lane & 15, q = lane >> 4;
    const bool av = m0 + r < M, bv = n0 + r < N;
    const float* pa = s.A + (int64_t)(av ? m0 + r : 0) * s.sam;
    const float* pb = s.B + (int64_t)(bv ? n0 + r : 0) * s.sbn;
    const bool va = s.sak == 1 && (s.sam & 3) == 0 && (reinterpret_cast<uintptr_t>(s.A) & 15) == 0;
    const bool vb = s.sbk == 1 && (s.sbn & 3) == 0 && (reinterpret_cast<uintptr_t>(s.B) & 15) == 0;
    const int K = s.K;
#pragma unroll 2
    for (int k0 = 0; k0 < K; k0 += kKChunk) {
        const int k = k0 + 4 * q;
        const f32x4 a = sac_ld4(pa, s.sak, k, K, av, va);
        const f32x4 b = sac_ld4(pb, s.sbk, k, K, bv, vb);
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c1, 0, 0, 0);
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c1, 0, 0, 0);
    }
}

__global__ __launch_bounds__(kSacThreads) void sac_mm_kernel(const SacMmArgs a) {
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kSacWaves + ((int)threadIdx.x >> 6));
    if (t >= a.tile_start[a.np]) return;
    int pi = 0;
    while (pi + 1 < a.np && t >= a.tile_start[pi + 1]) ++pi;
    const SacProblem& p = a.p[pi];
    const int lt = t - a.tile_start[pi];
    const int m0 = tile_m0(lt, p.tiles_n), n0 = tile_n0(lt, p.tiles_n);
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    sac_seg_acc(c0, c1, p.s[0], p.M, p.N, m0, n0, lane);
    if (p.nseg > 1) sac_seg_acc(c0, c1, p.s[1], p.M, p.N, m0, n0, lane);
    const f32x4 c = c0 + c1;
    const int col = tile_col(n0, lane);
    if (col >= p.N) return;
    const int epi = a.epilogue;
    const float bc = (epi == kEpiBiasRelu || epi == kEpiBias) ? p.aux[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = tile_row(m0, lane, i);
        if (row >= p.M) continue;
        const int64_t o = (int64_t)row * p.ldo + col;
        if (epi == kEpiBiasRelu) {
            const float z = c[i] + bc;
            p.out[o] = z > 0.f ? z : 0.f;
        } else if (epi == kEpiBias) {
            p.out[o] = c[i] + bc;
        } else if (epi == kEpiMask) {
            p.out[o] = p.aux[o] > 0.f ? c[i] : 0.f;  // relu's backward: the gradient where the activation is positive
        } else if (epi == kEpiStore) {
            p.out[o] = c[i];
        } else {
            const float pn = adam_update(p.out[o], c[i], p.m + o, p.v + o, a.adam);
            p.out[o] = pn;
            if (a.soft && p.target) p.target[o] = p.target[o] * a.one_minus_tau + pn * a.tau;  // utils.soft_update
        }
    }
}

// GaussianPolicy.sample behind the heads, one thread per row of [s'; s]: Normal.rsample, tanh, the action, log_prob with the bound term
struct SacPolicyTailArgs {
    const float *mean, *raw_log_std;  // [2B, act]
    const float *eps_next, *eps_cur;  // [B, act]
    const float *scale, *bias;        // [act]
    float *action, *tanh_x, *sech2_x;  // [2B, act]
    float* log_pi;                    // [2B]
    int B, act;
};

__global__ __launch_bounds__(kSacThreads) void sac_policy_tail_kernel(const SacPolicyTailArgs a) {
    const int row = blockIdx.x * kSacThreads + threadIdx.x;
    if (row >= 2 * a.B) return;
    const float* eps = row < a.B ? a.eps_next + (int64_t)row * a.act : a.eps_cur + (int64_t)(row - a.B) * a.act;
    float lp = 0.f;
    for (int d = 0; d < a.act; ++d) {
        const int64_t o = (int64_t)row * a.act + d;
        const float mean = a.mean[o];
        const float ls = clamp_log_std(a.raw_log_std[o]);
        const float std = expf(ls);
        const float x = mean + eps[d] * std;  // Normal.rsample
        const float y = tanhf(x);
        // 1 - tanh(x)^2 as sech(x)^2 = 4 t / (1 + t)^2, t = exp(-2 |x|): no cancellation where |tanh| is near 1 (formed from the
        // rounded tanh, an error of half an ulp in y is an error of y / (1 - y^2) ulps in the bound term, and of one sign)
        const float t = expf(-2.f * fabsf(x));
        const float omy = 4.f * t / ((1.f + t) * (1.f + t));
        a.action[o] = y * a.scale[d] + a.bias[d];
        a.tanh_x[o] = y;
        a.sech2_x[o] = omy;
        const float dlt = x - mean;
        // Normal.log_prob.  log(std) is the clamped log_std itself: logf(expf(ls)) came out below ls by 3e-8 per action dim on average
        // (the device's expf rounds to one side more often than the other), a bias that a mean over the batch -- the logged entropy, the
        // gradient of alpha -- keeps in full
        float l = -(dlt * dlt) / (2.f * (std * std)) - ls - 0.91893853320467274178f;
        l -= logf(a.scale[d] * omy + kSacEpsilon);                                           // model.py:103
        lp += l;
    }
    a.log_pi[row] = lp;
}

// d(policy loss) / d(mean, log_std) of the s half, one thread per (row, dim): through the action (d_pi, from the updated critic), the
// bound term of log_prob, rsample and the clamp (zero outside [-20, 2]).  The quadratic term of Normal.log_prob at its own sample
// is -eps^2 / 2: its gradient is zero and is not formed.
struct SacPolicyBwdArgs {
    const float *raw_log_std, *tanh_x, *sech2_x;  // the s half: [B, act]
    const float *eps_cur, *scale, *d_pi;
    const float* alpha;
    float *d_mean, *d_log_std;
    int B, act;
};

__global__ __launch_bounds__(kSacThreads) void sac_policy_tail_bwd_kernel(const SacPolicyBwdArgs a) {
    const int i = blockIdx.x * kSacThreads + threadIdx.x;
    if (i >= a.B * a.act) return;
    const int d = i % a.act;
    const float gl = (1.f / (float)a.B) * *a.alpha;  // d loss / d log_pi of a row
    const float y = a.tanh_x[i], sc = a.scale[d];
    const float raw = a.raw_log_std[i];
    const float ls = clamp_log_std(raw);
    const float std = expf(ls);
    const float omy = a.sech2_x[i];  // 1 - y^2
    const float u = sc * omy + kSacEpsilon;
    const float dy = a.d_pi[i] * sc + gl * (2.f * sc * y / u);
    const float dx = dy * omy;
    a.d_mean[i] = dx;
    const bool inside = raw >= kLogSigMin && raw <= kLogSigMax;
    a.d_log_std[i] = inside ? dx * a.eps_cur[i] * std - gl : 0.f;
}

// The output layers (N = 1) of the Q-networks of 16 rows per workgroup, wave w the network w, then the row tail and dz of the last
// hidden layer.  td != 0: networks 0, 1 = the target on (s', a'), 2, 3 = the critic on (s, a); the TD target, the squared errors and
// dq_i = 2 (q_i - y) / B.  td == 0: networks 0, 1 = the updated critic on (s, pi); min with torch's tie rule (half each), the row's
// policy loss term and dq_i = -(1 / B) [q_i is the minimum].
struct SacQTailArgs {
    const float* h2;        // [nets][B][H]
    const float* w3[4];     // [H]
    const float* b3[4];     // [1]
    const float *batch;     // [B, width]
    const float *log_pi;    // [2B]
    const float* alpha;
    float *q, *y, *sq_err, *dq, *row_loss;  // q [2][B] (td: the critic's), y [B], sq_err [2][B], dq [2][B], row_loss [B]
    float* dz2;             // [2][B][H]
    int B, H, width, r_col, td;
    float gamma;
};

__global__ __launch_bounds__(kSacThreads) void sac_q_tail_kernel(const SacQTailArgs a) {
    __shared__ float qs[4][kTile];
    __shared__ float dqs[2][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * kTile;
    const int nets = a.td ? 4 : 2;
    if (wave < nets) {
        SacSeg s;
        s.A = a.h2 + (int64_t)wave * a.B * a.H;
        s.sam = a.H;
        s.sak = 1;
        s.B = a.w3[wave];
        s.sbk = 1;
        s.sbn = 0;
        s.K = a.H;
        f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
        sac_seg_acc(c0, c1, s, a.B, 1, m0, 0, lane);
        const f32x4 c = c0 + c1;
        if (tile_col(0, lane) == 0) {  // the one column of the tile
            const float b = *a.b3[wave];
#pragma unroll
            for (int i = 0; i < 4; ++i) qs[wave][tile_row(0, lane, i)] = c[i] + b;
        }
    }
    __syncthreads();
    if (tid < kTile && m0 + tid < a.B) {
        const int row = m0 + tid;
        const float alpha = *a.alpha;
        if (a.td) {
            const float q1t = qs[0][tid], q2t = qs[1][tid], q1 = qs[2][tid], q2 = qs[3][tid];
            const float* br = a.batch + (int64_t)row * a.width + a.r_col;
            const float mn = (q1t < q2t ? q1t : q2t) - alpha * a.log_pi[row];
            const float y = br[0] + br[1] * a.gamma * mn;
            const float norm = 2.f / (float)a.B;
            const float d1 = q1 - y, d2 = q2 - y;
            a.q[row] = q1;
            a.q[a.B + row] = q2;
            a.y[row] = y;
            a.sq_err[row] = d1 * d1;
            a.sq_err[a.B + row] = d2 * d2;
            dqs[0][tid] = a.dq[row] = norm * d1;
            dqs[1][tid] = a.dq[a.B + row] = norm * d2;
        } else {
            const float q1 = qs[0][tid], q2 = qs[1][tid];
            const float g = -(1.f / (float)a.B);
            a.row_loss[row] = alpha * a.log_pi[a.B + row] - (q1 < q2 ? q1 : q2);
            dqs[0][tid] = q1 == q2 ? g / 2.f : (q1 > q2 ? 0.f : g);
            dqs[1][tid] = q1 == q2 ? g / 2.f : (q1 < q2 ? 0.f : g);
        }
    }
    __syncthreads();
    const int first = a.td ? 2 : 0;  // the networks that are differentiated
    const int rows = min(kTile, a.B - m0);
    for (int i = 0; i < 2; ++i) {
        const float* h = a.h2 + ((int64_t)(first + i) * a.B + m0) * a.H;
        float* dz = a.dz2 + ((int64_t)i * a.B + m0) * a.H;
        const float* w = a.w3[first + i];
        for (int t = tid; t < rows * a.H; t += kSacThreads) {
            const int r = t / a.H, k = t - r * a.H;
            dz[t] = h[t] > 0.f ? dqs[i][r] * w[k] : 0.f;
        }
    }
}

// One workgroup: the sums of the update in a fixed order, the Adam step on log_alpha, the new alpha, the result slot
//   result = (qf1_loss, qf2_loss, policy_loss, alpha_loss, alpha, batch_reward, entropy, 0)
struct SacFinishArgs {
    const float *sq_err, *row_loss, *log_pi, *batch;
    float *log_alpha, *m, *v, *alpha;
    float* result;
    int B, width, r_col, tuning;
    float target_entropy;
    AdamScalars adam;
};

__device__ __forceinline__ double sac_block_sum(double x, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
    for (int s = kSacThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// (the sums over the batch run in double, in a fixed order, and are rounded once: they are the update's reported numbers)
__global__ __launch_bounds__(kSacThreads) void sac_finish_kernel(const SacFinishArgs a) {
    __shared__ double red[kSacThreads];
    const int tid = threadIdx.x;
    const float la = a.tuning ? *a.log_alpha : 0.f;
    double s1 = 0, s2 = 0, sp = 0, sl = 0, sr = 0, st = 0, sa = 0;
    for (int r = tid; r < a.B; r += kSacThreads) {
        s1 += (double)a.sq_err[r];
        s2 += (double)a.sq_err[a.B + r];
        sp += (double)a.row_loss[r];
        const float lp = a.log_pi[a.B + r];
        sl += (double)lp;
        const float t = lp + a.target_entropy;
        st += (double)t;
        sa += (double)(la * t);
        sr += (double)a.batch[(int64_t)r * a.width + a.r_col];
    }
    s1 = sac_block_sum(s1, red);
    s2 = sac_block_sum(s2, red);
    sp = sac_block_sum(sp, red);
    sl = sac_block_sum(sl, red);
    sr = sac_block_sum(sr, red);
    st = sac_block_sum(st, red);
    sa = sac_block_sum(sa, red);
    if (tid != 0) return;
    const double nb = (double)a.B;
    float alpha = *a.alpha, alpha_loss = 0.f;
    if (a.tuning) {
        alpha_loss = (float)(-(sa / nb));
        const float g = (float)(-(st / nb));  // d alpha_loss / d log_alpha
        const float ln = adam_update(la, g, a.m, a.v, a.adam);
        *a.log_alpha = ln;
        alpha = expf(ln);
        *a.alpha = alpha;
    }
    a.result[0] = (float)(s1 / nb);
    a.result[1] = (float)(s2 / nb);
    a.result[2] = (float)(sp / nb);
    a.result[3] = alpha_loss;
    a.result[4] = alpha;
    a.result[5] = (float)(sr / nb);
    a.result[6] = (float)(-(sl / nb));
    a.result[7] = 0.f;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

SacSeg seg(const float* A, int sam, int sak, const float* B, int sbk, int sbn, int K) {
    SacSeg s;
    s.A = A; s.B = B; s.sam = sam; s.sak = sak; s.sbk = sbk; s.sbn = sbn; s.K = K;
    return s;
}

struct SacLaunch {
    SacMmArgs a;
    SacLaunch(int epilogue) {
        std::memset(&a, 0, sizeof(a));
        a.epilogue = epilogue;
    }
    SacProblem& add(const SacSeg& s0, int M, int N, float* out, int ldo, const float* aux = nullptr) {
        SacProblem& p = a.p[a.np];
        p.s[0] = s0;
        p.nseg = 1;
        p.M = M; p.N = N; p.out = out; p.ldo = ldo; p.aux = aux;
        p.tiles_n = tiles_across(N);
        a.tile_start[a.np + 1] = a.tile_start[a.np] + tiles_across(M) * p.tiles_n;
        ++a.np;
        return p;
    }
    SacProblem& add2(const SacSeg& s0, const SacSeg& s1, int M, int N, float* out, int ldo, const float* aux = nullptr) {
        SacProblem& p = add(s0, M, N, out, ldo, aux);
        p.s[1] = s1;
        p.nseg = 2;
        return p;
    }
    // kEpiAdam: `out` [M, N] is the parameter, its gradient the product
    void adam(const SacSeg& s0, int M, int N, float* param, float* m, float* v, float* target) {
        SacProblem& p = add(s0, M, N, param, N);
        p.m = m; p.v = v; p.target = target;
    }
    void go(hipStream_t st) {
        const int tiles = a.tile_start[a.np];
        hipLaunchKernelGGL(sac_mm_kernel, dim3((unsigned)((tiles + kSacWaves - 1) / kSacWaves)), dim3(kSacThreads), 0, st, a);
    }
};

inline size_t up4(size_t n) { return (n + 3) & ~(size_t)3; }

// the engine's scratch activations of a batch of B rows, one behind the other (every section starts on 16 bytes)
struct SacWs {
    float *ph1, *ph2, *mean, *lstd, *act, *tanh_x, *sech2_x, *log_pi, *qh1, *qh2, *dz2, *dz1, *q, *y, *sq_err, *dq, *row_loss, *d_pi, *d_mean, *d_lstd,
        *pdh2, *pdh1;
    size_t floats;
    SacWs(float* base, size_t B, size_t H, size_t A) {
        size_t o = 0;
        auto take = [&](size_t n) { float* p = base ? base + o : nullptr; o += up4(n); return p; };
        ph1 = take(2 * B * H); ph2 = take(2 * B * H);
        mean = take(2 * B * A); lstd = take(2 * B * A); act = take(2 * B * A); tanh_x = take(2 * B * A); sech2_x = take(2 * B * A);
        log_pi = take(2 * B);
        qh1 = take(4 * B * H); qh2 = take(4 * B * H);
        dz2 = take(2 * B * H); dz1 = take(2 * B * H);
        q = take(2 * B); y = take(B); sq_err = take(2 * B); dq = take(2 * B); row_loss = take(B);
        d_pi = take(B * A); d_mean = take(B * A); d_lstd = take(B * A);
        pdh2 = take(B * H); pdh1 = take(B * H);
        floats = o;
    }
};

// the pointer table of hipets_sac_bind (include/hipets.h)
enum { kPol = 0, kPolM = 8, kPolV = 16, kCrit = 24, kCritM = 36, kCritV = 48, kTgt = 60, kLogAlpha = 72, kLogAlphaM = 73, kLogAlphaV = 74,
       kAlpha = 75, kScale = 76, kBias = 77 };

// the six tensors of Q-network j of the four a TD step runs: 0, 1 = the target's two, 2, 3 = the critic's two
inline float* const* q_net(float* const* P, int j) { return j < 2 ? P + kTgt + 6 * j : P + kCrit + 6 * (j - 2); }

}  // namespace

}  // namespace hipets

using namespace hipets;

extern "C" {

int hipets_sac_bind(hipets_engine* e, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t tuning, double gamma, double tau,
                    double target_entropy, int32_t target_update_interval, const double* adam, const void* ptrs, int32_t n_ptrs) {
    if (!e) return fail("null engine");
    e->has_sac = false;
    e->sac_last_batch = 0;
    if (!adam || !ptrs) return fail("null argument");
    if (check_mlp_dims("sac", obs_dim, hidden, act_dim)) return 1;
    if (n_ptrs != HIPETS_SAC_N_PTRS) return fail("sac pointer table holds %d entries, expected %d", n_ptrs, HIPETS_SAC_N_PTRS);
    if (target_update_interval < 1) return fail("sac target_update_interval %d < 1", target_update_interval);
    void* const* tab = reinterpret_cast<void* const*>(ptrs);
    for (int i = 0; i < HIPETS_SAC_N_PTRS; ++i) {
        const bool alpha_state = i >= kLogAlpha && i <= kLogAlphaV;
        if (!tab[i] && (tuning || !alpha_state)) return fail("sac pointer table entry %d is null", i);
    }
    for (int o = 0; o < 3; ++o) {
        const double b1 = adam[3 * o], b2 = adam[3 * o + 1], eps = adam[3 * o + 2];
        if (!(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0 && eps >= 0.0)) return fail("sac optimizer %d: betas / eps out of range", o);
    }
    HCHECK(hipSetDevice(e->device));
    if (e->sac_one.ensure(16)) return 1;
    const float one[4] = {1.f, 1.f, 1.f, 1.f};
    HCHECK(hipMemcpy(e->sac_one.p, one, sizeof(one), hipMemcpyHostToDevice));
    hipets::SacBind& b = e->sac;
    b.obs = obs_dim; b.act = act_dim; b.hid = hidden; b.tuning = tuning != 0; b.interval = target_update_interval;
    b.gamma = (float)gamma; b.tau = (float)tau; b.one_minus_tau = (float)(1.0 - tau); b.target_entropy = (float)target_entropy;
    for (int i = 0; i < 9; ++i) b.adam[i] = adam[i];
    for (int i = 0; i < HIPETS_SAC_N_PTRS; ++i) b.p[i] = reinterpret_cast<float*>(tab[i]);
    e->has_sac = true;
    return 0;
}

int hipets_sac_update(hipets_engine* e, const float* batch, int32_t batch_size, const float* eps_next, const float* eps_cur, int64_t update_index,
                      int64_t step_critic, int64_t step_policy, int64_t step_alpha, double lr_critic, double lr_policy, double lr_alpha,
                      float* result, void* stream) {
    if (!e || !e->has_sac) return fail("engine has no SAC agent (call hipets_sac_bind)");
    if (!batch || !eps_next || !eps_cur || !result) return fail("null argument");
    if (batch_size < 1 || batch_size > HIPETS_SAC_MAX_BATCH) return fail("sac batch %d outside [1, %d]", batch_size, HIPETS_SAC_MAX_BATCH);
    if (update_index < 0 || step_critic < 0 || step_policy < 0 || step_alpha < 0) return fail("negative update index or step count");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const hipets::SacBind& sb = e->sac;
    const TransitionLayout row(sb.obs, sb.act, 0);  // (the batch's rows: no area)
    const int B = batch_size, O = sb.obs, A = sb.act, H = sb.hid, K1 = O + A, W = row.width;
    const size_t BH = (size_t)B * H;
    if (e->sac_ws.ensure(SacWs(nullptr, B, H, A).floats * 4)) return 1;
    const SacWs ws(e->sac_ws.as<float>(), B, H, A);
    float* const* P = sb.p;
    const float* one = e->sac_one.as<float>();
    const float *s = batch, *s2 = batch + row.c_next;
    const int r_col = row.c_rew;
    // optimizer o's (beta1, beta2, eps) are sb.adam[3 o ..]: the critic's, the policy's, alpha's
    auto adam_of = [&](int o, double lr, long long steps_taken) { return adam_scalars(lr, sb.adam[3 * o], sb.adam[3 * o + 1], sb.adam[3 * o + 2], steps_taken + 1); };
    const AdamScalars ad_c = adam_of(0, lr_critic, step_critic), ad_p = adam_of(1, lr_policy, step_policy), ad_a = adam_of(2, lr_alpha, step_alpha);

    // ---- 1. the policy's forward over [s'; s] and the sample tail ----
    {
        SacLaunch l(kEpiBiasRelu);
        l.add(seg(s2, W, 1, P[kPol + 0], 1, O, O), B, H, ws.ph1, H, P[kPol + 1]);
        l.add(seg(s, W, 1, P[kPol + 0], 1, O, O), B, H, ws.ph1 + BH, H, P[kPol + 1]);
        l.go(st);
    }
    {
        SacLaunch l(kEpiBiasRelu);
        l.add(seg(ws.ph1, H, 1, P[kPol + 2], 1, H, H), 2 * B, H, ws.ph2, H, P[kPol + 3]);
        l.go(st);
    }
    {
        SacLaunch l(kEpiBias);
        l.add(seg(ws.ph2, H, 1, P[kPol + 4], 1, H, H), 2 * B, A, ws.mean, A, P[kPol + 5]);
        l.add(seg(ws.ph2, H, 1, P[kPol + 6], 1, H, H), 2 * B, A, ws.lstd, A, P[kPol + 7]);
        l.go(st);
    }
    {
        SacPolicyTailArgs t{ws.mean, ws.lstd, eps_next, eps_cur, P[kScale], P[kBias], ws.act, ws.tanh_x, ws.sech2_x, ws.log_pi, B, A};
        hipLaunchKernelGGL(sac_policy_tail_kernel, dim3((unsigned)((2 * B + kSacThreads - 1) / kSacThreads)), dim3(kSacThreads), 0, st, t);
    }
    // ---- 2. four Q-networks per layer: the target's two on (s', a'), the critic's two on (s, a) ----
    float* const pi = ws.act + (size_t)B * A;
    {
        SacLaunch l(kEpiBiasRelu);
        for (int j = 0; j < 4; ++j) {
            float* const* N = q_net(P, j);
            const SacSeg state = seg(j < 2 ? s2 : s, W, 1, N[0], 1, K1, O);
            const SacSeg action = j < 2 ? seg(ws.act, A, 1, N[0] + O, 1, K1, A) : seg(batch + row.c_act, W, 1, N[0] + O, 1, K1, A);
            l.add2(state, action, B, H, ws.qh1 + j * BH, H, N[1]);
        }
        l.go(st);
    }
    {
        SacLaunch l(kEpiBiasRelu);
        for (int j = 0; j < 4; ++j) {
            float* const* N = q_net(P, j);
            l.add(seg(ws.qh1 + j * BH, H, 1, N[2], 1, H, H), B, H, ws.qh2 + j * BH, H, N[3]);
        }
        l.go(st);
    }
    SacQTailArgs qt{};
    qt.h2 = ws.qh2; qt.batch = batch; qt.log_pi = ws.log_pi; qt.alpha = P[kAlpha];
    qt.q = ws.q; qt.y = ws.y; qt.sq_err = ws.sq_err; qt.dq = ws.dq; qt.row_loss = ws.row_loss; qt.dz2 = ws.dz2;
    qt.B = B; qt.H = H; qt.width = W; qt.r_col = r_col; qt.gamma = sb.gamma;
    const dim3 row_tiles((unsigned)((B + kTile - 1) / kTile));
    {
        for (int j = 0; j < 4; ++j) {
            float* const* N = q_net(P, j);
            qt.w3[j] = N[4];
            qt.b3[j] = N[5];
        }
        qt.td = 1;
        hipLaunchKernelGGL(sac_q_tail_kernel, row_tiles, dim3(kSacThreads), 0, st, qt);
    }
    // ---- 3. the critic's backward: the dz chain through the old weights, then all dW / db products with Adam (+ soft update) ----
    {
        SacLaunch l(kEpiMask);
        for (int i = 0; i < 2; ++i)
            l.add(seg(ws.dz2 + i * BH, H, 1, P[kCrit + 6 * i + 2], H, 1, H), B, H, ws.dz1 + i * BH, H, ws.qh1 + (2 + i) * BH);
        l.go(st);
    }
    {
        SacLaunch l(kEpiAdam);
        l.a.adam = ad_c;
        l.a.soft = update_index % sb.interval == 0;
        l.a.tau = sb.tau;
        l.a.one_minus_tau = sb.one_minus_tau;
        for (int i = 0; i < 2; ++i) {
            float* const* N = P + kCrit + 6 * i;
            float* const* M = P + kCritM + 6 * i;
            float* const* V = P + kCritV + 6 * i;
            float* const* T = P + kTgt + 6 * i;
            const float *dz1 = ws.dz1 + i * BH, *dz2 = ws.dz2 + i * BH, *dq = ws.dq + (size_t)i * B;
            l.adam(seg(dz1, 1, H, batch, W, 1, B), H, K1, N[0], M[0], V[0], T[0]);
            l.adam(seg(dz1, 1, H, one, 0, 0, B), H, 1, N[1], M[1], V[1], T[1]);
            l.adam(seg(dz2, 1, H, ws.qh1 + (2 + i) * BH, H, 1, B), H, H, N[2], M[2], V[2], T[2]);
            l.adam(seg(dz2, 1, H, one, 0, 0, B), H, 1, N[3], M[3], V[3], T[3]);
            l.adam(seg(dq, 0, 1, ws.qh2 + (2 + i) * BH, H, 1, B), 1, H, N[4], M[4], V[4], T[4]);
            l.adam(seg(dq, 0, 1, one, 0, 0, B), 1, 1, N[5], M[5], V[5], T[5]);
        }
        l.go(st);
    }
    // ---- 4. the policy's gradient through the updated critic ----
    {
        SacLaunch l(kEpiBiasRelu);
        for (int j = 0; j < 2; ++j) {
            float* const* N = P + kCrit + 6 * j;
            l.add2(seg(s, W, 1, N[0], 1, K1, O), seg(pi, A, 1, N[0] + O, 1, K1, A), B, H, ws.qh1 + j * BH, H, N[1]);
        }
        l.go(st);
    }
    {
        SacLaunch l(kEpiBiasRelu);
        for (int j = 0; j < 2; ++j) l.add(seg(ws.qh1 + j * BH, H, 1, P[kCrit + 6 * j + 2], 1, H, H), B, H, ws.qh2 + j * BH, H, P[kCrit + 6 * j + 3]);
        l.go(st);
    }
    {
        for (int j = 0; j < 2; ++j) {
            qt.w3[j] = P[kCrit + 6 * j + 4];
            qt.b3[j] = P[kCrit + 6 * j + 5];
        }
        qt.td = 0;
        hipLaunchKernelGGL(sac_q_tail_kernel, row_tiles, dim3(kSacThreads), 0, st, qt);
    }
    {
        SacLaunch l(kEpiMask);
        for (int i = 0; i < 2; ++i) l.add(seg(ws.dz2 + i * BH, H, 1, P[kCrit + 6 * i + 2], H, 1, H), B, H, ws.dz1 + i * BH, H, ws.qh1 + i * BH);
        l.go(st);
    }
    {
        SacLaunch l(kEpiStore);  // d pi = dz1_1 W1_1[:, obs:] + dz1_2 W1_2[:, obs:]: no weight gradients in this pass
        l.add2(seg(ws.dz1, H, 1, P[kCrit + 0] + O, K1, 1, H), seg(ws.dz1 + BH, H, 1, P[kCrit + 6] + O, K1, 1, H), B, A, ws.d_pi, A);
        l.go(st);
    }
    {
        SacPolicyBwdArgs t{ws.lstd + (size_t)B * A, ws.tanh_x + (size_t)B * A, ws.sech2_x + (size_t)B * A, eps_cur, P[kScale], ws.d_pi, P[kAlpha], ws.d_mean, ws.d_lstd, B, A};
        hipLaunchKernelGGL(sac_policy_tail_bwd_kernel, dim3((unsigned)((B * A + kSacThreads - 1) / kSacThreads)), dim3(kSacThreads), 0, st, t);
    }
    const float *ph1s = ws.ph1 + BH, *ph2s = ws.ph2 + BH;
    {
        SacLaunch l(kEpiMask);
        l.add2(seg(ws.d_mean, A, 1, P[kPol + 4], H, 1, A), seg(ws.d_lstd, A, 1, P[kPol + 6], H, 1, A), B, H, ws.pdh2, H, ph2s);
        l.go(st);
    }
    {
        SacLaunch l(kEpiMask);
        l.add(seg(ws.pdh2, H, 1, P[kPol + 2], H, 1, H), B, H, ws.pdh1, H, ph1s);
        l.go(st);
    }
    {
        SacLaunch l(kEpiAdam);
        l.a.adam = ad_p;
        float* const* N = P + kPol;
        float* const* M = P + kPolM;
        float* const* V = P + kPolV;
        l.adam(seg(ws.pdh1, 1, H, s, W, 1, B), H, O, N[0], M[0], V[0], nullptr);
        l.adam(seg(ws.pdh1, 1, H, one, 0, 0, B), H, 1, N[1], M[1], V[1], nullptr);
        l.adam(seg(ws.pdh2, 1, H, ph1s, H, 1, B), H, H, N[2], M[2], V[2], nullptr);
        l.adam(seg(ws.pdh2, 1, H, one, 0, 0, B), H, 1, N[3], M[3], V[3], nullptr);
        l.adam(seg(ws.d_mean, 1, A, ph2s, H, 1, B), A, H, N[4], M[4], V[4], nullptr);
        l.adam(seg(ws.d_mean, 1, A, one, 0, 0, B), A, 1, N[5], M[5], V[5], nullptr);
        l.adam(seg(ws.d_lstd, 1, A, ph2s, H, 1, B), A, H, N[6], M[6], V[6], nullptr);
        l.adam(seg(ws.d_lstd, 1, A, one, 0, 0, B), A, 1, N[7], M[7], V[7], nullptr);
        l.go(st);
    }
    // ---- 5. the alpha step and the result slot ----
    {
        SacFinishArgs f{};
        f.sq_err = ws.sq_err; f.row_loss = ws.row_loss; f.log_pi = ws.log_pi; f.batch = batch;
        f.log_alpha = P[kLogAlpha]; f.m = P[kLogAlphaM]; f.v = P[kLogAlphaV]; f.alpha = P[kAlpha];
        f.result = result;
        f.B = B; f.width = W; f.r_col = r_col; f.tuning = sb.tuning;
        f.target_entropy = sb.target_entropy;
        f.adam = ad_a;
        hipLaunchKernelGGL(sac_finish_kernel, dim3(1), dim3(kSacThreads), 0, st, f);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "sac kernel launch failed: %s", hipGetErrorString(err));
    e->sac_last_batch = B;
    return 0;
}

int hipets_sac_forward_taps(hipets_engine* e, int32_t batch_size, float* q1, float* q2, float* y, float* log_pi_next, float* log_pi,
                            void* stream) {
    if (!e || !e->has_sac) return fail("engine has no SAC agent (call hipets_sac_bind)");
    if (batch_size < 1 || batch_size != e->sac_last_batch) return fail("sac taps: batch %d is not the last update's (%d)", batch_size, e->sac_last_batch);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const size_t B = (size_t)batch_size;
    const SacWs ws(e->sac_ws.as<float>(), B, e->sac.hid, e->sac.act);
    const size_t n = B * 4;
    if (q1) HCHECK(hipMemcpyAsync(q1, ws.q, n, hipMemcpyDeviceToDevice, st));
    if (q2) HCHECK(hipMemcpyAsync(q2, ws.q + B, n, hipMemcpyDeviceToDevice, st));
    if (y) HCHECK(hipMemcpyAsync(y, ws.y, n, hipMemcpyDeviceToDevice, st));
    if (log_pi_next) HCHECK(hipMemcpyAsync(log_pi_next, ws.log_pi, n, hipMemcpyDeviceToDevice, st));
    if (log_pi) HCHECK(hipMemcpyAsync(log_pi, ws.log_pi + B, n, hipMemcpyDeviceToDevice, st));
    return 0;
}

}  // extern "C"
