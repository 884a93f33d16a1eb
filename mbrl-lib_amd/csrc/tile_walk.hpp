// tile_walk.hpp -- what every 16 x 16 fp32 result tile of v_mfma_f32_16x16x4_f32 in train.hip and sac.hip shares: how the tiles of
// an M x N result are numbered and which elements of a tile a lane holds; and the 64 x 64 block geometry of the two blocked kernels
// (sac_mm_blocked_kernel in sac.hip, train_dw_kernel in train_split.hip).  The k-loops that fill a tile (mm_tile in train.hip,
// sac_seg_acc in sac.hip, mm_rows_step in train_split.hip) are not here: they walk k in different orders and stay apart.
// A site deals tiles t = wave, wave + waves, ... < tiles_across(M) * tiles_across(N) to its waves and, under col < N and row < M, walks
// the lane's four elements.  These are plain functions on purpose.  Forceinline templates that take the two loop bodies as lambdas
// compute the same values, but the compiler orders the kernel's instructions differently around a closure: train_step_kernel then
// took 2 more VGPRs and spilt 6 to 7 more SGPRs.
#pragma once
#include <hip/hip_runtime.h>

namespace hipets {

// tiles along an extent of n rows or columns
__host__ __device__ __forceinline__ int tiles_across(int n) { return (n + 15) >> 4; }

// tile t of a result that is tn tiles wide, in row-major tile order: its first row and column
__device__ __forceinline__ int tile_m0(int t, int tn) { return (t / tn) << 4; }
__device__ __forceinline__ int tile_n0(int t, int tn) { return (t % tn) << 4; }

// The lane-to-element map: element i of lane l's f32x4 result is C[m0 + 4 (l >> 4) + i][n0 + (l & 15)].
__device__ __forceinline__ int tile_col(int n0, int lane) { return n0 + (lane & 15); }
__device__ __forceinline__ int tile_row(int m0, int lane, int i) { return m0 + 4 * (lane >> 4) + i; }

// The blocked product of sac.hip (sac_mm_blocked_kernel) and the dW kernel of the row-split trainer (train_dw_kernel) deal 64 x 64
// blocks of 4 x 4 tiles to workgroups, numbered like the tiles: block b of a result that is bn blocks wide, in row-major block order.
// Wave w of the workgroup owns the 2 x 2 tiles at rows 32 (w >> 1), columns 32 (w & 1) of the block.  (What the two kernels stage in
// LDS differs and is theirs: kSacPanelStride, row-major; kSplitDwStride, k-major.)  Int = the type the kernel numbers its blocks in:
// sac.hip in int, train_dw_kernel by its unsigned blockIdx.x, and the division is that type's, as it was in either kernel.
constexpr int kBlock = 64;
__host__ __device__ __forceinline__ int blocks_across(int n) { return (n + kBlock - 1) / kBlock; }
template <class Int> __device__ __forceinline__ int block_m0(Int b, Int bn) { return (int)(b / bn) * kBlock; }
template <class Int> __device__ __forceinline__ int block_n0(Int b, Int bn) { return (int)(b % bn) * kBlock; }
__device__ __forceinline__ int block_wave_m0(int wave) { return (wave >> 1) << 5; }
__device__ __forceinline__ int block_wave_n0(int wave) { return (wave & 1) << 5; }

}  // namespace hipets
