// returns_kernel.hpp -- the masked returns of a finished trajectory: ONE kernel and ONE launcher behind hipets_trajectory_returns
// (rollout.hip) and hipets_discounted_returns (value.hip), so the two entry points cannot drift apart.  Host units only.
#pragma once
#include <hip/hip_runtime.h>

#include "engine.hpp"
#include "particle_reduce.hpp"

#pragma GCC visibility push(hidden)

namespace hipets {

namespace {  // (internal linkage: each of the two units gets its own copy, like policy_layer.hpp's pack kernel)

// model_env.py:186-191 over a finished trajectory: rewards / dones [H, B] of rollouts whose reward and termination were evaluated
// OUTSIDE the rollout kernel (Python callables over the traced states).  One thread per row, so the loads of a step are coalesced
// over B; per row, in step order, the chain of rollout.hpp's end_step_for_row:
//     r = term ? 0 : rewards[t][row];  term |= dones[t][row] != 0;  tot += r
// (a select, like the reference's rewards[terminated] = 0: whatever a terminated row's reward holds, NaN included, adds exactly 0).
// kDiscount: the same chain with a discount and an optional bootstrap, one float32 operation per line:
//     tot = tot + disc * r;  disc = disc * gamma          and, with values:  tot = tot + (term ? 0 : disc * values[row])
// cand_per_block > 0: the workgroup owns candidates [blockIdx.x * cand_per_block, + cand_per_block) = cand_per_block * P consecutive
// rows (<= kReturnsThreads); their totals go through LDS to the thread that runs candidate c's particle_value, as particle_mean_kernel
// does (the same rule: the same bits).  cand_per_block == 0 (P > kReturnsThreads): rows only, blockDim.x per workgroup,
// into row_totals (never null then); the launcher runs the particle reduction behind it.
constexpr int kReturnsThreads = 256;
template <bool kDiscount>
__global__ __launch_bounds__(kReturnsThreads) void trajectory_returns_kernel(const float* __restrict__ rewards, const unsigned char* __restrict__ dones,
                                                                             const float* __restrict__ values, const float gamma, int pop, int H, int P,
                                                                             int cand_per_block, const ParticleReduce r, float* __restrict__ returns,
                                                                             float* __restrict__ row_totals, int* __restrict__ first_done) {
    __shared__ float tot_s[kReturnsThreads];
    const long long B = (long long)pop * P;
    const int tid = threadIdx.x;
    const int rows_here = cand_per_block > 0 ? cand_per_block * P : (int)blockDim.x;
    const long long row = (long long)blockIdx.x * rows_here + tid;
    if (tid < rows_here && row < B) {
        float tot = 0.0f;
        [[maybe_unused]] float disc = 1.0f;
        bool term = false;
        int first = H;
#pragma unroll 4
        for (int t = 0; t < H; ++t) {
            const size_t i = (size_t)t * (size_t)B + (size_t)row;
            const float rw = rewards[i];
            const bool d = dones[i] != 0;
            const float rr = term ? 0.0f : rw;
            if (d && !term) first = t;
            term = term || d;
            if constexpr (kDiscount) {
                const float dr = disc * rr;
                tot = tot + dr;
                disc = disc * gamma;
            } else {
                tot += rr;
            }
        }
        if constexpr (kDiscount) {
            if (values) {
                const float dv = disc * values[row];
                tot = tot + (term ? 0.0f : dv);
            }
        }
        tot_s[tid] = tot;
        if (row_totals) row_totals[row] = tot;
        if (first_done) first_done[row] = first;
    }
    if (cand_per_block == 0) return;
    __syncthreads();
    const long long c = (long long)blockIdx.x * cand_per_block + tid;
    if (tid < cand_per_block && c < pop) returns[c] = particle_value(tot_s + tid * P, 1, P, r);
}

// The launch of both entry points; the caller has checked its arguments and check_reduce, and holds the StreamScope (the two-pass
// form may run on the engine's row totals).  values / gamma are read under kDiscount only.
template <bool kDiscount>
inline int launch_trajectory_returns(hipets_engine* e, const float* rewards, const uint8_t* dones, const float* values, float gamma, int pop, int H,
                                     int P, float* returns, float* row_totals, int32_t* first_done, hipStream_t st) {
    const long long B = (long long)pop * P;
    if (P <= kReturnsThreads) {
        const int cpb = kReturnsThreads / P;  // whole candidates per workgroup
        hipLaunchKernelGGL(trajectory_returns_kernel<kDiscount>, dim3((unsigned)((pop + cpb - 1) / cpb)), dim3(kReturnsThreads), 0, st, rewards, dones,
                           values, gamma, pop, H, P, cpb, e->reduce, returns, row_totals, first_done);
        HCHECK(hipGetLastError());
        return 0;
    }
    // a candidate's particles do not fit one workgroup: the row pass, then the particle reduction
    if (!row_totals) {
        if (e->totals.ensure((size_t)B * 4)) return 1;
        row_totals = e->totals.as<float>();
    }
    hipLaunchKernelGGL(trajectory_returns_kernel<kDiscount>, dim3((unsigned)((B + kReturnsThreads - 1) / kReturnsThreads)), dim3(kReturnsThreads), 0, st,
                       rewards, dones, values, gamma, pop, H, P, 0, e->reduce, static_cast<float*>(nullptr), row_totals, first_done);
    HCHECK(hipGetLastError());
    return launch_particle_reduce(e, row_totals, returns, pop, P, st);
}

}  // namespace

}  // namespace hipets

#pragma GCC visibility pop
