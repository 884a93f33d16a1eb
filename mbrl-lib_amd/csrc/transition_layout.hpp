// transition_layout.hpp -- where a SAC transition's floats live (include/hipets.h), for replay.hip's kernels and
// hipets_sac_update: an area of `cap` rows is five arrays one behind the other, a batch row is state, action, next state, reward, mask
#pragma once
#include <hip/hip_runtime.h>

namespace hipets {

struct TransitionLayout {
    int width;                           // floats of a batch row, and of an area per row
    long long o_act, o_nobs, o_rew, o_done;  // where the area's arrays start, in floats (obs at 0; 64-bit: a 2 M-row ring passes 2^31 bytes)
    int c_act, c_next, c_rew, c_mask;    // columns of a batch row (the state at 0)
    __host__ __device__ TransitionLayout(int od, int ad, long long cap)
        : width(2 * od + ad + 2), o_act(cap * od), o_nobs(cap * (od + ad)), o_rew(cap * (2 * od + ad)), o_done(o_rew + cap), c_act(od),
          c_next(od + ad), c_rew(2 * od + ad), c_mask(c_rew + 1) {}
};

}  // namespace hipets
