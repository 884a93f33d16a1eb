// ensemble_bf16.hpp -- the BF16 form of the dynamics ensemble's forward (hipets_set_ensemble_kernel(HIPETS_ENSEMBLE_KERNEL_BF16);
// ensemble_bf16.hip): what ensemble.hip needs to dispatch to it -- the geometry rule, the weight images' sizes, the argument block, the
// pack and the launch.  The wide form's outline (ensemble_wide.hpp: the kept input and ONE hidden buffer in LDS, in-place hidden layers,
// the output layer and the statistics' state in registers) on v_mfma_f32_16x16x32_bf16: both operands of every linear layer rounded to
// bf16 nearest-even, exact products, fp32 accumulation, everything else fp32.  No HIP in this header's rules: plain C++.
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

#include "../../include/hipets.h"

namespace hipets {

constexpr int kEnsBf16Waves = 8;     // waves of a workgroup; wave w owns hidden and mean column tiles w, w + 8, ...
constexpr int kEnsBf16MaxT = 4;      // mean column tiles of one wave at out_dim 512
constexpr int kEnsBf16MaxTH = 8;     // hidden column tiles of one wave at hid 1024
constexpr int kEnsBf16RowPad = 16;   // bytes behind a row's chunks: 16 consecutive rows of a fragment read start 4 banks apart
constexpr int kEnsBf16Sums = 2;      // row sums reduced through LDS at a time (sum_d exp(logvar) and sum_d delta^2, then sum_d (S1/n)^2)

// kc0 / kch: 32-wide k chunks of the input and of a hidden layer.  tm: mean column tiles of the output layer.  th: hidden column tiles.
// R: row tiles of a workgroup (16 R rows).  T / TH: the mean / hidden column tiles of the busiest wave.  lds: dynamic LDS, bytes.
struct EnsBf16Geo { int kc0, kch, tm, th, R, T, TH, lds; };

// What a lane's 256 registers hold at R row tiles: TH x R x 4 hidden accumulators, T x R x 8 of statistics state, a ring of weight
// fragments (4 registers each, ens_bf16_ahead sets deep), R activation fragments and the head's working set.  The instances built are
// those the compiler fits without scratch (DESIGN.md section 35 has the table): at R = 4 two hidden tiles (hid <= 256) and two mean tiles
// (out_dim <= 256) per wave; at R = 2 two hidden tiles with any T, or up to eight (hid <= 1024) with one mean tile (out_dim <= 128).
constexpr bool ens_bf16_fits(int R, int T, int TH) { return R == 4 ? (TH <= 2 && T <= 2) : (TH <= 2 ? T <= kEnsBf16MaxT : (TH <= kEnsBf16MaxTH && T <= 1)); }
// weight fragment sets a wave keeps in flight ahead of its MFMAs (gemm_bf16.hpp, kBf16Ahead: the k loop is paced by these loads)
constexpr int ens_bf16_ahead(int TH) { return TH <= 2 ? 4 : 2; }

// THE geometry rule of the bf16 form (the launch and hipets_ensemble_geometry read it; hipets.ensemble.ensemble_bf16_geometry restates it).
// LDS holds X [16 R][64 kc0 + 16 bytes], the kept input, H [16 R][64 kch + 16 bytes], the one hidden buffer -- both bf16 in
// gemm_bf16.hpp's fragment row format -- and the waves' partial row sums [2][8][16 R] floats.  R = 4 where that fits `lds_max` and the
// registers (ens_bf16_fits), else 2: by the SHAPE alone.  False: R = 2 does not fit either, and the predict call refuses the model.
inline bool ensemble_bf16_geometry(int in_dim, int hid, int out_dim, size_t lds_max, EnsBf16Geo& g) {
    g.kc0 = (in_dim + 31) / 32; g.kch = (hid + 31) / 32;
    g.tm = (out_dim + 15) / 16; g.th = (hid + 15) / 16;
    g.T = (g.tm + kEnsBf16Waves - 1) / kEnsBf16Waves;
    g.TH = (g.th + kEnsBf16Waves - 1) / kEnsBf16Waves;
    for (g.R = 4; g.R >= 2; g.R >>= 1) {
        const size_t lds = (size_t)16 * g.R * (size_t)(64 * g.kc0 + kEnsBf16RowPad + 64 * g.kch + kEnsBf16RowPad + 4 * kEnsBf16Sums * kEnsBf16Waves);
        g.lds = (int)lds;
        if (lds <= lds_max && ens_bf16_fits(g.R, g.T, g.TH)) return true;
    }
    return false;
}

// The weight images: per member the layers in order, per layer [column tile][k chunk][lane] entries of 16 bytes -- lane l's A-operand
// fragment, output column 16 tile + (l & 15), k = 32 chunk + 8 (l >> 4) .. + 7.  Hidden layers have th tiles; the output layer has tm mean
// tiles and, for a Gaussian model, tm log-variance tiles behind them (tile tm + c: columns out_dim + 16 c ..), so a wave finds the
// log-variance columns of its mean tile tile-aligned.  Entries past K or N are zeros.  Sizes in 16-byte entries:
inline size_t ens_bf16_layer_entries(const EnsBf16Geo& g, int l, int n_layers, int deterministic) {
    const size_t tiles = l == n_layers - 1 ? (size_t)g.tm * (deterministic ? 1 : 2) : (size_t)g.th;
    return tiles * (size_t)(l == 0 ? g.kc0 : g.kch) * 64;
}
inline size_t ens_bf16_member_entries(const EnsBf16Geo& g, int n_layers, int deterministic) {
    size_t n = 0;
    for (int l = 0; l < n_layers; ++l) n += ens_bf16_layer_entries(g, l, n_layers, deterministic);
    return n;
}

// hipets_ensemble_predict's arguments behind its checks; `wb`: the bf16 images (above), `b` / `lv` / `norm` / `cols`: the snapshot's own
struct EnsBf16Args {
    const float *obs, *actions, *model_in;  // [B, obs_dim] and [B, act_dim], or [B, in_dim]
    float *mean, *logvar, *stats;           // [n, B, out_dim] x 2, [B, 4]; each may be null
    const uint4* wb;                        // member e at e * wbmember entries
    const float* b;                         // member e at e * bmember; layers in order, [pad16(N)] each
    const double* norm;                     // [3][in_dim]: mean, std, 1 / std
    const float* lv;                        // [lv_rows][out_dim] min, then [lv_rows][out_dim] max
    const hipets_obs_column* cols;
    size_t wbmember, bmember;
    int B, n, obs_dim, act_dim, in_dim, out_dim, n_layers;
    int activation, obs_process, normalizer, deterministic, lv_per_member;
    float slope;
    int members[HIPETS_ENSEMBLE_MAX_MEMBERS];  // the n requested members, in order
    EnsBf16Geo g;
};

// The images of all E members from the snapshot's padded fp32 images `w` (member e at e * wmember floats; layer l [pad16(K)][pad16(N)]),
// on `st`: one launch per layer.  `wb` holds E * ens_bf16_member_entries entries.
hipError_t pack_ensemble_bf16(uint4* wb, const float* w, size_t wmember, int E, int in_dim, int hid, int out_dim, int n_layers, int deterministic,
                              const EnsBf16Geo& g, hipStream_t st);

// One launch on `st`, ceil(B / 16 R) workgroups (ensemble_bf16.hip).  LDS past the 64 KiB window is opted in to once per instance and device.
hipError_t launch_ensemble_bf16(const EnsBf16Args& a, size_t lds_max, hipStream_t st);

}  // namespace hipets
