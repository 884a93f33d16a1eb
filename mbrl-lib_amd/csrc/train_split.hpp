// train_split.hpp -- the row-split training step (train_split.hip; HIPETS_TRAIN_KERNEL_SPLIT of include/hipets.h): its limits, the
// slab's layout, the LDS need of the rows kernel and the argument block its three kernels share (filled by train.hpp's train_fill and
// train_fill_step).  The dW kernel's 64 x 64 blocks and their waves' corners are tile_walk.hpp's.
//   train_rows_kernel          grid (row block, member): 32 rows through forward, loss tail and the dA chain, activations LDS-resident
//   train_dw_kernel            grid (64 x 64 block of W, layer, member): dW = A_l^T dZ_l over all rows, Adam fused; first row of blocks: db
//   train_split_finish_kernel  grid (member): the step's loss and grad_sq partials, summed in a fixed order
// One step = these three launches in stream order; no workgroup waits on another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_walk.hpp"
#include "train.hpp"

namespace hipets {

constexpr int kSplitMaxBatch = HIPETS_TRAIN_SPLIT_MAX_BATCH;
constexpr int kSplitRows = 32;           // rows of a row block: two 16-row MFMA tiles that share every weight fragment
constexpr int kSplitRowsThreads = 512;   // 8 waves, each a block of kSplitRows x 32 result columns at a time
constexpr int kSplitDwThreads = 256;     // 4 waves, each a 2 x 2 block of 16 x 16 tiles of a kBlock x kBlock block of W (tile_walk.hpp: 64)
constexpr int kSplitDwChunk = 32;        // minibatch rows per staged K-chunk of the dW product
constexpr int kSplitDwStride = 80;       // floats per LDS row of a chunk: kBlock + 16, so k-steps q and q + 1 lie 16 banks apart
static_assert(kSplitDwStride == kBlock + 16 && kSplitDwThreads == 4 * 64, "the dW kernel's staging and its four waves are written for 64 x 64 blocks");

// floats per row of a slab section / of an LDS panel that is `width` wide: rows start 16-byte aligned (the panel: plus one float4,
// so the rows of a 32 k wide panel do not all start in one bank)
__host__ __device__ constexpr int split_ld(int width) { return (width + 3) & ~3; }
__host__ __device__ constexpr int split_panel_stride(int width) { return split_ld(width) + 4; }

// the rows kernel's two activation panels: P0 holds the inputs of the even layers (A_0 is in wide), P1 those of the odd ones; the
// dZ chain runs back through the same two.  The output layer's panel (up to 2 x 512 columns) goes through the slab instead.
__host__ __device__ constexpr int split_panel0_floats(int in, int hid) { return kSplitRows * split_panel_stride(in > hid ? in : hid); }
__host__ __device__ constexpr int split_panel1_floats(int hid) { return kSplitRows * split_panel_stride(hid); }
__host__ __device__ constexpr int split_rows_lds_bytes(int in, int hid) {
    return (split_panel0_floats(in, hid) + split_panel1_floats(hid)) * (int)sizeof(float);
}
static_assert(split_rows_lds_bytes(kTrainMaxIn, kTrainMaxHid) <= 160 * 1024, "the widest shape of the ABI fits the LDS of a CU");

// The member's slab of a split step, in floats: per layer its input A_l [max_batch, ld(d_l)], per hidden layer its pre-activation
// Z_l [max_batch, ld(d_{l+1})], per layer its gradient dZ_l [max_batch, ld(d_{l+1})] (the rows kernel writes them, the dW kernel reads
// A_l and dZ_l; dZ of the output layer holds the raw output until the loss tail has turned it into the gradient).  ld = split_ld.
struct TrainSplitSlab {
    int64_t stride;  // floats per member
    int64_t off_a[HIPETS_MAX_LAYERS];
    int64_t off_z[HIPETS_MAX_LAYERS];
    int64_t off_d[HIPETS_MAX_LAYERS];
};

inline TrainSplitSlab train_split_slab(const int32_t* dims, int n_layers, int max_batch) {
    TrainSplitSlab s{};
    int64_t off = 0;
    auto take = [&](int width) { const int64_t o = off; off += ((int64_t)max_batch * split_ld(width) + 63) / 64 * 64; return o; };
    for (int l = 0; l < n_layers; ++l) s.off_a[l] = take(dims[l]);
    for (int l = 0; l + 1 < n_layers; ++l) s.off_z[l] = take(dims[l + 1]);
    for (int l = 0; l < n_layers; ++l) s.off_d[l] = take(dims[l + 1]);
    s.stride = off;
    return s;
}

// blocks of W_l the dW kernel cuts a din x dout layer into, in tile_walk.hpp's row-major block order
__host__ __device__ __forceinline__ int split_dw_blocks(int din, int dout) { return blocks_across(din) * blocks_across(dout); }

// One minibatch step.  The fields train_fill sets carry TrainStepArgs' names; idx / rows / loss / grad_sq point at THIS step's entries,
// and the step's two Adam values travel as plain members (no per-launch table: steps_per_launch has no meaning here).
struct TrainSplitArgs {
    float* w[HIPETS_MAX_LAYERS];
    float* b[HIPETS_MAX_LAYERS];
    float* mw[HIPETS_MAX_LAYERS];
    float* mb[HIPETS_MAX_LAYERS];
    float* vw[HIPETS_MAX_LAYERS];
    float* vb[HIPETS_MAX_LAYERS];
    const float* x;
    const float* y;
    const int32_t* idx;        // [E, max_batch] of the step
    const int32_t* rows;       // [1] of the step
    const float* min_logvar;
    const float* max_logvar;
    float* slab;               // [E, at.stride]
    double* loss_part;         // [E, row blocks of max_batch] the row blocks' loss sums
    double* gsq_part;          // [E, n_layers, dw_blocks] the dW workgroups' sums of squared raw gradients
    float* loss;               // [E] of the step
    float* grad_sq;
    TrainSplitSlab at;
    int64_t n_rows;
    int32_t dims[HIPETS_MAX_LAYERS + 1];
    int32_t n_layers, out_dim, ensemble_size, max_batch, activation;
    int32_t row_blocks;        // of max_batch
    int32_t dw_blocks;         // the widest layer's split_dw_blocks: the dW grid's x extent
    int32_t bounds_stride;
    float leaky_slope, grad_scale, weight_decay;
    AdamScalars adam;          // of this step
};

#pragma GCC visibility push(hidden)
// hipets_train_steps_loss under HIPETS_TRAIN_KERNEL_SPLIT, after its argument checks and stream entry (train.hip); wide: under
// HIPETS_TRAIN_WIDTH_WIDE, the same step with train_wide.hip's rows kernel in place of train_rows_kernel
int train_split_steps(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows, const int32_t* idx,
                      const int32_t* rows, int32_t n_steps, int64_t step0, float* loss, float* grad_sq, hipStream_t st, int32_t loss_kind,
                      int32_t bounds_per_member, float grad_scale, bool wide);
#pragma GCC visibility pop

}  // namespace hipets
