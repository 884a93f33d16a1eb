// train.hpp -- GaussianMLP ensemble training (ModelTrainer.train / evaluate, mbrl/models/model_trainer.py:70-262): the limits, the
// slab's layout and the kernel argument blocks of train.hip (its kernels and launchers, and its entry points of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hipets.h"
#include "adam.hpp"

namespace hipets {

constexpr int kTrainThreads = 512;        // 8 waves: two per SIMD, so one wave's MFMA chain hides the other's latency
constexpr int kTrainMaxSteps = 256;       // steps per launch: the per-step Adam scalars travel in the kernel arguments
constexpr int kTrainMaxMembers = HIPETS_TRAIN_MAX_MEMBERS;  // the shape limits of the C ABI (include/hipets.h)
constexpr int kTrainMaxHid = HIPETS_TRAIN_MAX_HID;
constexpr int kTrainMaxIn = HIPETS_TRAIN_MAX_IN;
constexpr int kTrainMaxOut = HIPETS_TRAIN_MAX_OUT;  // target columns; the output layer is 2 x this wide (mean | logvar)
constexpr int kTrainMaxBatch = HIPETS_TRAIN_MAX_BATCH;
constexpr int kEvalRows = 32;             // rows per evaluate workgroup
constexpr int kEvalThreads = 256;
constexpr int kTrainLossNLL = HIPETS_TRAIN_LOSS_NLL;  // the loss tail train_step_kernel is instantiated for
constexpr int kTrainLossMSE = HIPETS_TRAIN_LOSS_MSE;

// The member's slab of a step launch, in floats: per layer its input A_l and (hidden layers) its pre-activation Z_l, the raw output
// O, the gathered targets T and two gradient ping-pong buffers D0 / D1, one behind the other, every section a multiple of 64 floats.
struct TrainSlab {
    int64_t stride;  // floats per member
    int64_t off_a[HIPETS_MAX_LAYERS];
    int64_t off_z[HIPETS_MAX_LAYERS];
    int64_t off_o, off_t, off_d0, off_d1;
};

// the layout for dims = (in, hid ... hid, output columns) and minibatches of at most max_batch rows
inline TrainSlab train_slab(const int32_t* dims, int n_layers, int out_dim, int max_batch) {
    TrainSlab s{};
    int64_t off = 0, widest = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += (n + 63) / 64 * 64; return o; };
    for (int l = 0; l < n_layers; ++l) s.off_a[l] = take((int64_t)max_batch * dims[l]);
    for (int l = 0; l + 1 < n_layers; ++l) s.off_z[l] = take((int64_t)max_batch * dims[l + 1]);
    for (int l = 1; l <= n_layers; ++l) widest = widest > dims[l] ? widest : dims[l];
    s.off_o = take((int64_t)max_batch * dims[n_layers]);
    s.off_t = take((int64_t)max_batch * out_dim);
    s.off_d0 = take((int64_t)max_batch * widest);
    s.off_d1 = take((int64_t)max_batch * widest);
    s.stride = off;
    return s;
}

// One launch = n_steps consecutive minibatch steps, one workgroup per member (members never communicate: the loss is a sum
// over members, Adam is elementwise, the logvar bounds are constants).  Everything a step keeps for its backward pass lives
// in the member's slab (global, L2-resident; TrainSlab above).
// Loss kinds: NLL (GaussianMLP._nll_loss: the output layer is 2 out wide, mean | raw logvar) and MSE (GaussianMLP._mse_loss of a
// deterministic model: the output layer is out wide, the loss a plain sum of squared errors, no logvar columns anywhere).
// A BasicEnsemble of one-member GaussianMLPs is the same launch with per-member bounds (bounds_stride = out) and grad_scale = 1 / E.
struct TrainStepArgs {
    float* w[HIPETS_MAX_LAYERS];   // [E, d_l, d_{l+1}]  (torch's EnsembleLinearLayer layout)
    float* b[HIPETS_MAX_LAYERS];   // [E, 1, d_{l+1}]
    float* mw[HIPETS_MAX_LAYERS];  // Adam exp_avg, same layouts
    float* mb[HIPETS_MAX_LAYERS];
    float* vw[HIPETS_MAX_LAYERS];  // Adam exp_avg_sq
    float* vb[HIPETS_MAX_LAYERS];
    const float* x;                // [n_rows, in]  model inputs of the whole dataset
    const float* y;                // [n_rows, out] targets
    const int32_t* idx;            // [n_steps, E, max_batch] dataset rows of every (step, member)
    const int32_t* rows;           // [n_steps] rows of every step (the last minibatch of an epoch is ragged)
    const float* min_logvar;       // [out], or [E, out] with bounds_stride = out; not read under MSE
    const float* max_logvar;
    float* slab;                   // [E, at.stride]
    float* loss;                   // [n_steps, E] mean NLL (MSE: sum of squared errors) of every member, without grad_scale
    float* grad_sq;                // [n_steps, E] sum of squares of the raw gradient (before weight decay; grad_scale included)
    TrainSlab at;                  // where the sections of a member's slab are
    int64_t n_rows;
    int32_t dims[HIPETS_MAX_LAYERS + 1];  // in, hid ... hid, 2 out (MSE: out)
    int32_t n_layers, out_dim, ensemble_size, max_batch, n_steps, activation;
    int32_t bounds_stride;         // member stride of min_logvar / max_logvar: 0 = shared [out], out = per member [E, out]
    float leaky_slope;
    float grad_scale;              // multiplied into the loss gradient (1 / E of BasicEnsemble.loss); 1.0f is exact
    float weight_decay;            // coupled into the gradient ahead of Adam (torch.optim.Adam's weight_decay)
    AdamConstants adam;            // the optimizer (adam.hpp), and AdamScalars' two per-step values of every step of the launch:
    float neg_step_size[kTrainMaxSteps];
    float bc2_sqrt[kTrainMaxSteps];
};

// evaluate: the mean columns only (the first out_dim of the dims[n_layers] the output layer has), many workgroups over (row tile, member); partial sums [E, tiles] reduced in a fixed order
struct TrainEvalArgs {
    const float* w[HIPETS_MAX_LAYERS];
    const float* b[HIPETS_MAX_LAYERS];
    const float* x;
    const float* y;
    const int32_t* order;   // [n_rows] or NULL: row r of the pass is dataset row order[r]
    float* partial;         // [E, tiles]
    float* row_score;       // [E, n_rows] or NULL: sum over output dims of the squared error of every row
    float* score;           // [E]
    int64_t n_rows;
    int32_t dims[HIPETS_MAX_LAYERS + 1];
    int32_t n_layers, out_dim, ensemble_size, activation, max_width, tiles;
    float leaky_slope;
};

hipError_t launch_train_steps(const TrainStepArgs& a, int loss_kind, hipStream_t st);
hipError_t launch_train_eval(const TrainEvalArgs& a, hipStream_t st);

}  // namespace hipets
