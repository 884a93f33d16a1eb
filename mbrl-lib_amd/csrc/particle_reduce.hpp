// particle_reduce.hpp -- the ONE rule that collapses a candidate's P particle totals into its value (model_env.py:190-191 is the
// MEAN; the other kinds rank candidates by the spread the particles carry: DESIGN.md section 20).  Included by rollout_helpers.hpp
// (particle_mean_kernel, the LDS tail of trajectory_returns_kernel) and cem.hpp (the refit prologue): every site calls
// particle_value, so the rule exists once and all sites give the same bits.  fp32 op by op (the build has -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/hipets.h"

namespace hipets {

constexpr int kWorstKMaxP = 256;  // WORST_K counts ranks over the P totals (P^2 reads per candidate): refused beyond

struct ParticleReduce {
    int kind = HIPETS_REDUCE_MEAN;
    float kappa = 0.f;  // MEAN_STD: value = mean - kappa * std (kappa > 0 risk-averse, < 0 optimistic)
    int k = 0;          // WORST_K: mean of the k lowest totals, 1 <= k <= P
};

// s = 0; for p: s += t[p], strictly in particle order; the totals are fetched eight at a time (every load of a batch unconditional, its
// index clamped: the round trips overlap, the additions and their order are those of the plain loop)
__device__ __forceinline__ float particle_sum(const float* t, const int stride, const int P) {
    float s = 0.f;
    for (int q0 = 0; q0 < P; q0 += 8) {
        float tv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) tv[u] = t[(size_t)min(q0 + u, P - 1) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (q0 + u < P) s += tv[u];
    }
    return s;
}

// The value of the candidate whose particle totals are t[0], t[stride], ..., t[(P - 1) * stride] (row order: particle p of candidate
// c is row c * P + p), global memory or LDS.
//   MEAN      s / P
//   MEAN_STD  m = s / P;  q = sum (t[p] - m)^2 in particle order;  m - kappa * sqrtf(q / P)
//   MIN, MAX  the lowest / highest total; NaN if any total is NaN
//   WORST_K   NaN if any total is NaN; else rank_p = #{q < p : t[q] <= t[p]} + #{q > p : t[q] < t[p]} (ties go to the lower particle),
//             the totals of rank < k summed in particle order, / k.  k = P: every rank is below k -- MEAN's sum, MEAN's bits.
// No per-thread array is indexed at run time (no kernel of the library uses scratch memory): the ranks are counted by reading again.
__device__ __forceinline__ float particle_value(const float* t, const int stride, const int P, const ParticleReduce r) {
    if (r.kind == HIPETS_REDUCE_MEAN) return particle_sum(t, stride, P) / (float)P;
    if (r.kind == HIPETS_REDUCE_MEAN_STD) {
        const float m = particle_sum(t, stride, P) / (float)P;
        float q = 0.f;
        for (int p = 0; p < P; ++p) {
            const float d = t[(size_t)p * stride] - m;
            q += d * d;
        }
        const float sd = sqrtf(q / (float)P);
        return m - r.kappa * sd;
    }
    if (r.kind == HIPETS_REDUCE_MIN || r.kind == HIPETS_REDUCE_MAX) {
        const bool lowest = r.kind == HIPETS_REDUCE_MIN;
        float v = t[0];
        for (int p = 1; p < P; ++p) {
            const float tp = t[(size_t)p * stride];
            v = ((lowest ? tp < v : tp > v) || tp != tp) ? tp : v;
        }
        return v;
    }
    // WORST_K
    bool any_nan = false;
    float s = 0.f;
    for (int p = 0; p < P; ++p) {
        const float tp = t[(size_t)p * stride];
        any_nan = any_nan || tp != tp;
        int rank = 0;
        for (int q = 0; q < p; ++q) rank += t[(size_t)q * stride] <= tp;
        for (int q = p + 1; q < P; ++q) rank += t[(size_t)q * stride] < tp;
        if (rank < r.k) s += tp;
    }
    return any_nan ? NAN : s / (float)r.k;
}

}  // namespace hipets
