// agent_wide.hpp -- the WIDE form of the SAC actor's and critic's forward (hipets_set_agent_kernel(HIPETS_AGENT_KERNEL_WIDE);
// agent_wide.hip): what policy.hip and value.hip need to dispatch to it -- the geometry rule, the argument blocks, the two launches.
// The tile form (policy_layer.hpp) keeps a row's full-width activations in LDS, so its rows per workgroup shrink as the agent widens
// (64 / 32 / 16 at hidden <= 256 / 512 / 1024); the wide form keeps 64 rows at every width by never holding a full-width activation in
// LDS: h1 exists one column chunk at a time, h2 in registers only.  No HIP in this header's rule: plain C++.
#pragma once
#include <algorithm>
#include <cstddef>

#include <hip/hip_runtime.h>

namespace hipets {

constexpr int kWideRows = 64;   // rows of a workgroup: 4 row tiles, at every width
constexpr int kWideWaves = 8;   // its waves; wave w owns the h2 column tiles w, w + 8, ...
constexpr int kWideMaxTiles = 8;  // h2 column tiles of one wave at hidden 1024: 8 x 4 row tiles = 32 accumulators = 128 registers

// kp0 / hp / np_last: the first layer's K, the hidden width, the last layer's columns, rounded up to 16.  wc: the chunk width, columns of
// h1 that exist in LDS at a time.  tiles: the h2 column tiles of the busiest wave.  lds: the dynamic LDS of a launch, bytes.
struct WideGeo { int kp0, hp, np_last, wc, tiles, lds; };

// THE geometry rule of the wide form (the launches and the geometry queries read it; hipets/sac.py restates it for the host tests).
// LDS holds the 64 input rows [64][kp0 + 4] and one h1 chunk [64][wc + 4]; wc = the widest of 256, 128, 64 that fits `lds_max` beside
// the input, no wider than the hidden layer needs.  Behind the last chunk the same bytes hold the 8 waves' partial sums of the last
// layer, [8][64][np_last + 4].  False: the input rows and a 64-column chunk do not fit (no shape inside HIPETS_POLICY_MAX_* at 160 KB).
inline bool agent_wide_geometry(int k0, int hidden, int last_cols, size_t lds_max, WideGeo& g) {
    auto pad = [](int x) { return (x + 15) & ~15; };
    g.kp0 = pad(k0); g.hp = pad(hidden); g.np_last = pad(last_cols);
    auto chain_bytes = [&](int wc) { return (size_t)kWideRows * 4 * (size_t)(g.kp0 + 4 + wc + 4); };
    g.wc = 256;
    while (g.wc > 64 && (chain_bytes(g.wc) > lds_max || g.wc / 2 >= g.hp)) g.wc >>= 1;
    const size_t lds = std::max(chain_bytes(g.wc), (size_t)kWideWaves * kWideRows * 4 * (size_t)(g.np_last + 4));
    g.tiles = (g.hp / 16 + kWideWaves - 1) / kWideWaves;
    g.lds = (int)lds;
    return lds <= lds_max && g.tiles <= kWideMaxTiles;
}

// the body of hipets_policy_geometry / hipets_critic_geometry under the wide form: 4 row tiles whatever the batch, the rule's LDS
int wide_geometry_query(int batch, int k0, int hidden, int last_cols, size_t lds_max, int* row_tiles, int* lds_bytes);

// one packed network as hipets_policy_set / hipets_critic_set leave it: W[k][n] images [kp0][hp], [hp][hp], [hp][np_last], zero-padded biases
struct WideNet { const float *w1, *w2, *wl, *b1, *b2, *bl; };

struct WideActorArgs {
    const float *obs, *eps;                   // [B, obs_dim]; [B, act] or null
    float *actions, *mean_out, *log_std_out;  // [B, act]; the taps or null
    WideNet net;
    const float *scale, *bias;  // [act]
    int B, obs_dim, act, sample;
    unsigned long long seed, stream_id;
    WideGeo g;
};

struct WideCriticArgs {
    const float *obs, *actions;  // [B, obs_dim], [B, act]
    float *q1, *q2, *qmin;       // [B] each, or null
    WideNet net[2];              // Q1 (linear1..3), Q2 (linear4..6)
    int B, obs_dim, act;
    WideGeo g;
};

// One launch each on `st`, ceil(B / 64) workgroups (agent_wide.hip).  LDS past the 64 KiB window is opted in to once per instance and device.
hipError_t launch_actor_wide(const WideActorArgs& a, size_t lds_max, hipStream_t st);
hipError_t launch_critic_wide(const WideCriticArgs& a, size_t lds_max, hipStream_t st);

}  // namespace hipets
