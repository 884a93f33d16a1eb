// train_wide.hpp -- the WIDE training step and evaluate pass (train_wide.hip; hipets_set_train_width(HIPETS_TRAIN_WIDTH_WIDE) of
// include/hipets.h): hidden widths up to 1024, where two activation panels of 32 rows no longer fit the LDS of a CU.
//   train_wide_rows_kernel  grid (row block, member): 32 rows through forward, loss tail and the dA chain on ONE panel that every layer
//                           overwrites in place -- a layer's whole 32 x dout result waits in the accumulators of the waves that own its
//                           columns until every wave has read the panel for the last time
//   train_wide_eval_kernel  grid (row tile, member): the same forward chain, the mean columns of the output layer, train_eval_kernel's tail
// A wide step = train_wide_rows_kernel, then train_split.hip's train_dw_kernel and train_split_finish_kernel on the same slab and the same
// argument block (train_split.hpp: neither is sized by a hidden width); a wide evaluate = train_wide_eval_kernel, then train.hip's
// train_eval_reduce_kernel.  No workgroup waits on another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train.hpp"
#include "train_split.hpp"

namespace hipets {

constexpr int kTrainWideMaxHid = HIPETS_TRAIN_WIDE_MAX_HID;
constexpr int kWideThreads = kSplitRowsThreads;  // 8 waves over the column tiles of a layer; kSplitRows rows per workgroup, as the slab's row blocks are
constexpr int kWideWaves = kWideThreads / 64;
static_assert(kEvalRows == kSplitRows, "one panel shape for the step and the evaluate pass");

// The kernels are instantiated on kT, the 16-column tiles of a layer's result one wave may own (two row tiles each: 8 kT accumulator
// registers): 4 serves results up to 512 columns wide, 8 up to 1024.
constexpr int kWideTilesNarrow = 4, kWideTilesFull = 8;
__host__ __device__ constexpr int wide_columns(int tiles_per_wave) { return kWideWaves * tiles_per_wave * 16; }
static_assert(wide_columns(kWideTilesFull) >= kTrainWideMaxHid && wide_columns(kWideTilesFull) >= 2 * kTrainMaxOut, "the full instance owns every column of the widest layer");

// the one panel: kSplitRows rows of the widest layer input or result, train_split.hpp's row stride
__host__ __device__ constexpr int wide_lds_bytes(int widest) { return kSplitRows * split_panel_stride(widest) * (int)sizeof(float); }
static_assert(wide_lds_bytes(kTrainWideMaxHid) <= 160 * 1024 && kTrainMaxIn <= kTrainWideMaxHid && 2 * kTrainMaxOut <= kTrainWideMaxHid,
              "the widest shape of the ABI fits the LDS of a CU");

#pragma GCC visibility push(hidden)
// the rows kernel of one wide step (train_split.hip's step loop launches it in place of train_rows_kernel)
hipError_t launch_train_wide_rows(const TrainSplitArgs& a, int loss_kind, hipStream_t st);
// the wide evaluate kernel (train.hip's launch_train_eval launches it in place of train_eval_kernel)
hipError_t launch_train_wide_eval(const TrainEvalArgs& a, hipStream_t st);
#pragma GCC visibility pop

}  // namespace hipets
