// engine.hpp -- private to the host units of the C ABI (include/hipets.h): engine.hip, model.hip, rollout.hip, plan.hip, comm.hip,
// train.hip, policy.hip, replay.hip, sac.hip, value.hip, ensemble.hip and policy_rollout.hip.  The engine struct, the thread's error state, stream entry, host staging, and the few functions one unit offers another.
// Host code only; nothing declared here is part of the ABI (hidden visibility).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hipets.h"
#include "particle_reduce.hpp"
#include "planet_types.hpp"
#include "rollout_types.hpp"

namespace hipets {

// message and class of the last failure of this thread (hipets_last_error, hipets_last_error_kind); defined in engine.hip.
// (Default visibility on purpose: a unit that reads a thread_local of another unit calls its TLS init function through a WEAK
// reference, and g_err_kind -- constant-initialised -- has none.  A hidden weak reference is bound PC-relative in PIC code and
// comes out non-null: the first read from another unit jumped into nowhere.  Through the GOT it is null and skipped.)
extern thread_local std::string g_err;
extern thread_local int g_err_kind;

}  // namespace hipets

#pragma GCC visibility push(hidden)

namespace hipets {

// an argument / configuration the library rejects: deterministic, the same on every rank that passes the same arguments
int fail(const char* fmt, ...);
// something the machine did (a HIP / RCCL call, an allocation, a launch, a hand-over time-out): may hit one rank only
int fail_kind(int kind, const char* fmt, ...);

#define HCHECK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        cap = bytes;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// a network's weights as hipets_policy_set / hipets_critic_set packed them (policy_layer.hpp): is one set, its sizes, image and biases
struct MlpSnapshot { bool set = false; int obs = 0, hid = 0, act = 0; DevBuf w, b; };

// what hipets_ensemble_set keeps (ensemble.hip): the dynamics ensemble's shape, every member's padded W[k][n] images and biases (member e, layer
// l at e * wmember + its layer offset), the normaliser (mean, std, 1 / std: [3][in_dim] doubles), the log-variance bounds (min rows, then
// max rows: lv_rows each, indexed by member where every member owns its own), the elite list, the column table and the delta rule
struct EnsembleSnapshot {
    bool set = false;
    int E = 0, M = 0, obs_dim = 0, act_dim = 0, in_dim = 0, out_dim = 0, hid = 0, n_layers = 0;
    int activation = 0, obs_process = 0, normalizer = 0, deterministic = 0, lv_rows = 1;
    // how a prediction becomes the next observation (one_dim_tr_model.py:281-286; read by hipets_policy_rollout alone): bit d of
    // no_delta (HIPETS_ENSEMBLE_MAX_OUT bits, on the device) = observation dim d is predicted absolutely
    int target_is_delta = 0, learned_rewards = 0;
    float slope = 0.f;
    int members[HIPETS_ENSEMBLE_MAX_MEMBERS] = {};
    size_t wmember = 0, bmember = 0;
    DevBuf w, b, norm, lv, cols, no_delta;
};

// what hipets_sac_bind keeps: the agent's sizes and hyper-parameters, its optimizers' (beta1, beta2, eps) [critic, policy, alpha], and the
// pointer table (the live torch tensors, include/hipets.h)
struct SacBind {
    int obs = 0, act = 0, hid = 0, interval = 1;
    bool tuning = false;
    float gamma = 0.f, tau = 0.f, one_minus_tau = 1.f, target_entropy = 0.f;
    double adam[9] = {};
    float* p[HIPETS_SAC_N_PTRS] = {};
};

}  // namespace hipets

#pragma GCC visibility pop  // (the ABI's own opaque type keeps the default)

struct hipets_engine {
    using DevBuf = hipets::DevBuf;
    int device = 0;
    int num_cu = 256;
    size_t lds_max = 160 * 1024;
    bool has_model = false;
    hipets::ModelDev md{};
    int ensemble_size = 0;
    DevBuf w3pack;  // bf16x3 / bf16 precision modes: weight pieces (three bf16 planes / one)
    DevBuf wpack, bpack, layer_meta, norm_mean, norm_std, min_lv, max_lv, no_delta, members;
    // rollout workspace
    DevBuf s0, state, totals, term;
    // DEVICE mode, persistent form: row exchange table, per-step permutation keys, timeout flag (host-mapped)
    DevBuf exchange, step_keys, plan_keys;
    // host -> device staging of the caller's observations: a small ring of pinned buffers owned by the engine, so the async
    // copy never reads caller memory after the call returned (hipets.h: HOST arrays are consumed during the call)
    struct HostStage { void* p = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool used = false; };
    HostStage stage[4];
    int stage_next = 0;
    uint32_t tag_base = 0;  // hand-over tags handed out so far (exchange granules hold tags <= tag_base)
    // the key tables a fused plan generated up front: rollouts (plan_keys_seed, stream in [first, first + count), H) read them
    uint64_t plan_keys_seed = 0, plan_keys_first = 0;
    int plan_keys_count = 0, plan_keys_H = 0;
    int* error_flag = nullptr;
    bool persistent_ok = true;
    long long poll_ticks = 20000000ll;  // bound of one hand-over poll, 100 MHz ticks (hipets_set_handover_timeout; default 0.2 s)
    DevBuf census;                      // [2] ints of the co-residency self-test (residency.hpp census_ok)
    // The workspace (state / totals / schedules / plan buffers), the hand-over table, its tags and the key tables are
    // engine-global: the work of two calls must execute in the order the calls were made.  A call on another stream than the
    // previous call's first makes its stream wait for that one (an event, device side only), so "any stream per call"
    // (hipets.h) stays true without two launches ever sharing a buffer.
    hipStream_t last_stream = nullptr;
    bool last_stream_set = false;
    hipEvent_t last_done = nullptr;
    // plan workspace
    DevBuf mu, disp, population, values, best_value, best_solution, past_action, kept, elite_idx, keep_idx;
    // RCCL communicator (lazy-loaded librccl)
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    DevBuf shard_values, gathered;
    // PlaNet latent model
    bool has_planet = false;
    bool planet_static = false;  // the PlaNet model has conf/dynamics_model/planet.yaml's shapes: the STATIC kernel instance (planet_types.hpp)
    hipets::PlanetDev pd{};
    DevBuf planet_w, planet_b, planet_member, planet_ops;
    // fused plans: randomness mode of their rollouts, optional per-iteration trace
    int plan_mode = HIPETS_MODE_FAST;
    // how every entry point that reduces a candidate's particles forms its value (hipets_set_particle_reduce; particle_reduce.hpp)
    hipets::ParticleReduce reduce{};
    bool has_trace = false;
    hipets_plan_trace trace{};
    // timing: every timing_stride-th rollout-kernel launch carries a start / stop event pair on its dispatch packet
    bool timing = false;
    int timing_stride = 1;
    unsigned long long launch_counter = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> event_pool;
    // model training (hipets_train_steps / hipets_train_eval): per-member activation slabs, evaluate's partial sums
    DevBuf train_slab, train_partial;
    // the packed layers of the SAC actor (hipets_policy_set / _act, policy.hip) and of the SAC critic, Q1 and Q2 (hipets_critic_set / _q, value.hip)
    hipets::MlpSnapshot policy, critic;
    // the block counts of hipets_compact_transitions / hipets_ring_compact_transitions (replay.hip)
    DevBuf compact_counts;
    // SAC updates (hipets_sac_bind / hipets_sac_update, sac.hip): the bound agent, the scratch activations (grown on demand), a device 1.0f
    bool has_sac = false;
    hipets::SacBind sac{};
    int sac_last_batch = 0;
    DevBuf sac_ws, sac_one;
    // the dynamics ensemble as hipets_ensemble_set packed it (hipets_ensemble_predict, ensemble.hip); apart from the rollout model slot above
    hipets::EnsembleSnapshot ensemble;
};

#pragma GCC visibility push(hidden)

namespace hipets {

// ---- engine.hip ----

// copy `bytes` of caller HOST memory to `dst` on `st`: memcpy into the next pinned slot of the engine's ring, async copy from
// there.  A slot is reused only after the copy that last read it has executed (its event; normally long complete).
int stage_h2d(hipets_engine* e, void* dst, const void* src, size_t bytes, hipStream_t st);

// Every entry point that enqueues work on the engine's workspace calls this first: if `st` is not the stream of the previous
// call, `st` waits (device side) for what that call enqueued.  Same stream: nothing to do.  The event it waits for was recorded at
// the END of the previous call, on that call's own stream, while the caller was still inside the library -- i.e. while the stream
// was certainly alive (StreamScope below); nothing is ever recorded on a stream the caller may have destroyed since.
int enter_stream(hipets_engine* e, hipStream_t st);
// ... and holds one of these until it returns: marks the end of the call's work on its stream
struct StreamScope {
    hipets_engine* e;
    hipStream_t st;
    ~StreamScope();
};
#define ENTER_STREAM(e, st)                \
    if (enter_stream((e), (st))) return 1; \
    StreamScope stream_scope_ { (e), (st) }

// First local failure of a sharded plan on this rank (message + class).  A rank on which something cannot be enqueued must NOT
// leave the plan: its peers are, or will be, waiting in this and the remaining iterations' collectives.  It keeps contributing
// (stale) shards to every ncclAllGather and reports its own error at the end; the peers' plans are then built on garbage, which is
// why hipets.dist agrees on the outcome over all ranks (an all-reduce of the status) before anybody uses a plan.
struct LocalErr {
    std::string msg;
    int kind = HIPETS_ERR_NONE;
    bool ok() const { return kind == HIPETS_ERR_NONE; }
    void note(const int rc) {  // rc of a call that has just set g_err / g_err_kind
        if (rc && ok()) { msg = g_err; kind = g_err_kind == HIPETS_ERR_NONE ? HIPETS_ERR_RUNTIME : g_err_kind; }
    }
    int report() const {
        if (ok()) return 0;
        g_err = msg;
        g_err_kind = kind;
        return 1;
    }
};

// the engine's reduction against the particle count of a call (WORST_K: worst_k <= P <= 256); every call that reduces particles asks
// before it enqueues anything, a sharded plan on every rank alike
int check_reduce(const hipets_engine* e, int P);

// ---- rollout.hip (the one unit that includes rollout_helpers.hpp: its small kernels are launched from there) ----

// returns [pop] = the engine's reduction of totals [pop * P] (particle_mean_kernel); the caller has passed check_reduce
int launch_particle_reduce(const hipets_engine* e, const float* totals, float* returns, int pop, int P, hipStream_t st);

// hipets_rollout with a plan-level shortcut: s0 == nullptr means the initial state(s) are already staged in e->s0 (the observation
// is the same for every iteration of a plan); returns == nullptr: the caller reduces e->totals over the particles itself (the CEM /
// iCEM plans: inside the refit kernel, CemDev::totals).  The public entry point that led here holds the StreamScope.
int rollout_impl(hipets_engine* e, const float* actions, const float* s0, int32_t pop, int32_t H, int32_t P, const hipets_rollout_opts* o,
                 float* returns, void* stream);
// hipets_planet_rollout, `returns` as above.  o->n_env > 1: pop is n_env groups of pop / n_env candidates, group g starts from
// latent0[g] / belief0[g].
int planet_rollout_impl(hipets_engine* e, const float* actions, const float* latent0, const float* belief0, int32_t pop, int32_t H, int32_t P,
                        const hipets_planet_opts* o, float* returns, hipStream_t st);
// DEVICE-mode plans: the per-step permutation keys of ALL `iters` rollouts of a plan (stream ids first_stream, +1, ...) in one launch;
// rollout_impl finds them by seed / stream id.  Nothing to do for the other modes and forms.
int plan_step_keys(hipets_engine* e, int H, int iters, uint64_t seed, uint64_t first_stream, hipStream_t st);
// weight / bias packing of hipets_set_model and hipets_planet_set_model (rollout_helpers.hpp pack_*_kernel, one thread per element)
int pack_weights(hipStream_t st, float* dst, const float* src, const int* members, int M, int K, int N, int Kp, int Np, long long member_stride,
                 long long layer_off, int permute_cols, int src_nk, int head_dim = 0);
int pack_weights_b3(hipStream_t st, uint4* dst, const float* src, const int* members, int M, int K, int N, int Kp32, int Np, long long member_stride,
                    long long layer_off, int src_nk, int pieces);
int pack_bias(hipStream_t st, float* dst, const float* src, const int* members, int M, int N, int Np, int member_stride, int layer_off,
              int permute_cols, int head_dim = 0);

// ---- comm.hip ----

// ONE ncclAllGather of every rank's padded shard of `width` returns: e->shard_values -> e->gathered [world, width]
int comm_all_gather(hipets_engine* e, size_t width, hipStream_t st);
// e->gathered [world, width] (rank r's shard in row r, padded) -> e->values [rows]
int comm_unpad_shards(hipets_engine* e, int rows, int width, hipStream_t st);
// hipets_destroy: the engine's communicator, if it has one
void comm_release(hipets_engine* e);

}  // namespace hipets

#pragma GCC visibility pop
