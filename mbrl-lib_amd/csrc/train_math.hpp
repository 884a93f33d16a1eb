// train_math.hpp -- the elementwise device functions both training paths share (train.hip: one workgroup per member; train_split.hip:
// the row-split step): GaussianMLP's activations and their derivatives, torch's softplus, the MSE tail of one output element with its
// gradient (mse_tail), a wave's sum.  Plain functions, like tile_walk.hpp's and for its reason.  Not here, although both kernels of
// either path hold the same lines: the NLL tail and the compensated (Kahan) sum of the MSE bias gradients.  As functions (value,
// reference and pointer parameters were tried) they compiled to the same registers but to another instruction order in
// train_step_kernel<NLL>, train_rows_kernel<NLL> and train_dw_kernel<MSE>, so each kernel keeps its copy and names the other
// (DESIGN.md section 29).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hipets.h"

namespace hipets {

// the activation modules of GaussianMLP (gaussian_mlp.py:88-96) and their derivatives in terms of the pre-activation z
__device__ __forceinline__ float act_fwd(int act, float z, float slope) {
    switch (act) {
        case HIPETS_ACT_RELU: return z > 0.f ? z : 0.f;
        case HIPETS_ACT_SILU: return z / (1.f + expf(-z));
        case HIPETS_ACT_LEAKY_RELU: return z > 0.f ? z : z * slope;
        case HIPETS_ACT_TANH: return tanhf(z);
        default: return 1.f / (1.f + expf(-z));
    }
}

__device__ __forceinline__ float act_grad(int act, float z, float slope) {
    switch (act) {
        case HIPETS_ACT_RELU: return z > 0.f ? 1.f : 0.f;
        case HIPETS_ACT_SILU: {
            const float s = 1.f / (1.f + expf(-z));
            return s * (1.f + z * (1.f - s));
        }
        case HIPETS_ACT_LEAKY_RELU: return z > 0.f ? 1.f : slope;
        case HIPETS_ACT_TANH: {
            const float t = tanhf(z);
            return 1.f - t * t;
        }
        default: {
            const float s = 1.f / (1.f + expf(-z));
            return s * (1.f - s);
        }
    }
}

// torch.nn.functional.softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float softplus_grad(float x) {
    if (x > 20.f) return 1.f;
    const float z = expf(x);
    return z / (z + 1.f);
}

// GaussianMLP._mse_loss on one output element (gaussian_mlp.py:283-289): the loss is a plain sum of squared errors, accumulated in
// double (and rounded once per step)
__device__ __forceinline__ void mse_tail(float o, float target, float grad_scale, double& loss_sum, float& d_out) {
    const float d = o - target;
    loss_sum += (double)d * (double)d;
    d_out = 2.f * d * grad_scale;
}

template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

}  // namespace hipets
