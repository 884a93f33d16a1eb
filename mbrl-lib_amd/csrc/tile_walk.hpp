// tile_walk.hpp -- what every 16 x 16 fp32 result tile of v_mfma_f32_16x16x4_f32 in train.hip and sac.hip shares: how the tiles of
// an M x N result are numbered and which elements of a tile a lane holds.  The k-loops that fill a tile (mm_tile in train.hip,
// sac_seg_acc in sac.hip) are not here: they walk k in different orders and stay apart.
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

}  // namespace hipets
