// ensemble_wide.hpp -- the WIDE form of the dynamics ensemble's forward (hipets_set_ensemble_kernel(HIPETS_ENSEMBLE_KERNEL_WIDE);
// ensemble_wide.hip): what ensemble.hip needs to dispatch to it -- the geometry rule, the argument block, the launch.
// The tile form (ensemble.hip) keeps per row the model input, two full-width activation buffers (one as wide as the output layer) and
// two per-(row, column) variance accumulators in LDS, so a Humanoid-sized model (393-200x4-754) gets one 16-row tile per workgroup
// and every 16 rows stream all members' images from L2.  The wide form keeps the input and ONE hidden buffer: the hidden layers run
// in place, the output layer and the statistics' per-(row, column) state never leave registers, and a workgroup owns 64 rows (32
// where the input is too wide for 64).  No HIP in this header's rule: plain C++.
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

#include "../../include/hipets.h"

namespace hipets {

constexpr int kEnsWideWaves = 8;     // waves of a workgroup; wave w owns hidden and mean column tiles w, w + 8, ...
constexpr int kEnsWideMaxT = 4;      // mean column tiles of one wave at out_dim 512
constexpr int kEnsWideSums = 2;      // row sums reduced through LDS at a time: sum_d exp(logvar) and sum_d delta^2 (then sum_d (S1/n)^2)

// kp0 / hp / npo: in_dim, hid and the output layer's columns rounded up to 16.  R: row tiles of a workgroup (16 R rows).  T / TH: the
// mean / hidden column tiles of the busiest wave.  lds: the dynamic LDS of a launch, bytes.
struct EnsWideGeo { int kp0, hp, npo, R, T, TH, lds; };

// What the 256 registers of a lane hold at R row tiles: TH x R x 4 hidden accumulators beside T x R x 8 registers of statistics state and
// R x 8 of row sums.  The instances that the compiler fits without scratch (DESIGN.md section 33 has the table), which are the ones built:
// at R = 4 two hidden tiles (hid <= 256) and three mean tiles (out_dim <= 384) per wave; at R = 2 two hidden tiles with any T, or up to
// eight (hid <= 1024) with two mean tiles (out_dim <= 256).
constexpr bool ens_wide_fits(int R, int T, int TH) { return R == 4 ? (TH <= 2 && T <= 3) : (TH <= 2 ? T <= kEnsWideMaxT : (TH <= 8 && T <= 2)); }

// THE geometry rule of the wide form (the launch and hipets_ensemble_geometry read it; hipets.ensemble.ensemble_wide_geometry restates
// it for the host tests).  LDS holds X [16 R][kp0 + 4], the kept input, H [16 R][hp + 4], the one hidden buffer, and the waves' partial
// row sums [kEnsWideSums][8][16 R].  R = 4 where that fits `lds_max` and the registers (ens_wide_fits), else 2 -- by the SHAPE alone,
// never the batch or the outputs requested, so a row's bits do not move with the call it arrives in.  False: R = 2 does not fit
// either, and the wide setting runs the tile form for this model.
inline bool ensemble_wide_geometry(int in_dim, int hid, int out_dim, int deterministic, size_t lds_max, EnsWideGeo& g) {
    auto pad = [](int x) { return (x + 15) & ~15; };
    g.kp0 = pad(in_dim); g.hp = pad(hid); g.npo = pad(deterministic ? out_dim : 2 * out_dim);
    g.T = (pad(out_dim) / 16 + kEnsWideWaves - 1) / kEnsWideWaves;
    g.TH = (g.hp / 16 + kEnsWideWaves - 1) / kEnsWideWaves;
    for (g.R = 4; g.R >= 2; g.R >>= 1) {
        const size_t lds = (size_t)16 * g.R * 4 * (size_t)(g.kp0 + 4 + g.hp + 4 + kEnsWideSums * kEnsWideWaves);
        g.lds = (int)lds;
        if (lds <= lds_max && ens_wide_fits(g.R, g.T, g.TH)) return true;
    }
    return false;
}

// hipets_ensemble_predict's arguments behind its checks; the images are those hipets_ensemble_set packed for the tile form
struct EnsWideArgs {
    const float *obs, *actions, *model_in;  // [B, obs_dim] and [B, act_dim], or [B, in_dim]
    float *mean, *logvar, *stats;           // [n, B, out_dim] x 2, [B, 4]; each may be null
    const float *w, *b;                     // member e at e * wmember / e * bmember; layers in order, [kp][np] each / [np] each
    const double* norm;                     // [3][in_dim]: mean, std, 1 / std
    const float* lv;                        // [lv_rows][out_dim] min, then [lv_rows][out_dim] max
    const hipets_obs_column* cols;
    size_t wmember, bmember;
    int B, n, obs_dim, act_dim, in_dim, out_dim, n_layers;
    int activation, obs_process, normalizer, deterministic, lv_per_member;
    float slope;
    int members[HIPETS_ENSEMBLE_MAX_MEMBERS];  // the n requested members, in order
    EnsWideGeo g;
};

// One launch on `st`, ceil(B / 16 R) workgroups (ensemble_wide.hip).  LDS past the 64 KiB window is opted in to once per instance and device.
hipError_t launch_ensemble_wide(const EnsWideArgs& a, size_t lds_max, hipStream_t st);

}  // namespace hipets
