// adam.hpp -- torch.optim.Adam's non-fused single-tensor rule (torch/optim/adam.py _single_tensor_adam; no amsgrad, no maximize),
// once for the model trainer (train.hip) and the three SAC optimizers (sac.hip): the host's scalars of one step, the device's update
// of one element.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace hipets {

// One optimizer: what no step changes, and with it what step t does.  torch computes all six as python floats (double) and hands them
// to float32 tensor ops: one rounding each.
struct AdamConstants {
    float one_minus_beta1, beta2, one_minus_beta2, eps;
};
struct AdamScalars : AdamConstants {
    float neg_step_size, bc2_sqrt;  // -(lr / (1 - beta1^t)), (1 - beta2^t)^0.5
};

// step = t, the optimizer's step count after this update (>= 1)
inline AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, long long step) {
    const double t = (double)step;
    const double bc1 = 1.0 - std::pow(beta1, t), bc2 = 1.0 - std::pow(beta2, t);
    AdamScalars a;
    a.one_minus_beta1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.one_minus_beta2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.neg_step_size = (float)(-(lr / bc1));
    a.bc2_sqrt = (float)std::pow(bc2, 0.5);
    return a;
}

// The moment update of one element with gradient g (weight decay, where there is any, is already coupled into g); returns the new
// parameter.  exp_avg.lerp_(g, 1 - beta1) with Tensor.lerp_'s branch at weight 0.5; denom = sqrt(v) / bc2_sqrt + eps, in that order.
// The step's two values travel apart from the constants for train_step_kernel, whose argument block holds them in per-step arrays:
// it reads the constants in place (assembling an AdamScalars per step inside that kernel moved its instructions about and changed
// its SGPR spills; this way it compiles as it did with its own copy of this function).
__device__ __forceinline__ float adam_update(float p, float g, float* m, float* v, const AdamConstants& a, float neg_step_size, float bc2_sqrt) {
    const float mo = *m, w = a.one_minus_beta1;
    const float mn = w < 0.5f ? mo + w * (g - mo) : g - (g - mo) * (1.f - w);
    const float vn = *v * a.beta2 + a.one_minus_beta2 * g * g;
    *m = mn;
    *v = vn;
    const float denom = sqrtf(vn) / bc2_sqrt + a.eps;
    return p + neg_step_size * (mn / denom);
}

__device__ __forceinline__ float adam_update(float p, float g, float* m, float* v, const AdamScalars& a) {
    return adam_update(p, g, m, v, a, a.neg_step_size, a.bc2_sqrt);
}

}  // namespace hipets
