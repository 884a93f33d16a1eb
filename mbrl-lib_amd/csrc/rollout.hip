// rollout.hip -- rollouts of the C ABI (include/hipets.h): launch geometry, the binding from a call's mode to the kernel's arguments,
// hipets_rollout / hipets_step / hipets_planet_rollout / hipets_trajectory_returns / hipets_particle_reduce, the geometry queries and the exports of the device-side randomness.  The one
// unit that includes residency.hpp (the launcher of every rollout kernel instance) and rollout_helpers.hpp (the small kernels around it).
#include <hip/hip_ext.h>

#include <algorithm>

#include "engine.hpp"
#include "launch.hpp"
#include "residency.hpp"
#include "returns_kernel.hpp"
#include "rollout_helpers.hpp"
#include "rollout_smem.hpp"

using namespace hipets;

namespace {

// the kernel instance a call with R row tiles runs (launch.hpp pick_rollout_instance); nullptr: there is none, and fail() has said why
KernelRec* rollout_instance(const hipets_engine* e, int R, const RolloutArgs& ra) {
    static constexpr decltype(&rollout_instance_r1) resolvers[kMaxR] = {rollout_instance_r1, rollout_instance_r2, rollout_instance_r3, rollout_instance_r4};
    if (R < 1 || R > kMaxR) return fail("unsupported rows_per_group %d (1..%d)", R, kMaxR), nullptr;
    hipError_t why = hipSuccess;
    KernelRec* k = resolvers[R - 1](e->md, ra, &why);
    const bool b3 = e->md.precision == HIPETS_PREC_BF16X3;
    if (!k && why == hipErrorNotSupported && (b3 || e->md.precision == HIPETS_PREC_BF16))
        fail("precision %s: no shape-specialised kernel instance for this model / call (SiLU, f64 normaliser, no obs preprocessing, in-kernel "
             "sampling, one of the %s layer shapes, R = %d); use precision f32", b3 ? "bf16x3" : "bf16", b3 ? "BASELINE" : "two bf16", R);
    else if (!k) fail_kind(HIPETS_ERR_RUNTIME, "rollout kernel launch failed: %s", hipGetErrorString(why));
    return k;
}

int launch_rollout(hipets_engine* e, int R, int grid, size_t lds, const RolloutArgs& ra, hipStream_t st) {
    RolloutArgs rl = ra;
    rl.lds_bytes = (unsigned)lds;  // (debug builds check every LDS section against it)
    KernelRec* k = rollout_instance(e, R, rl);
    if (!k) return 1;
    hipEvent_t a = nullptr, b = nullptr;
    const bool timed = e->timing && (e->launch_counter++ % (unsigned long long)e->timing_stride) == 0;
    if (timed) {
        if (!e->event_pool.empty()) {
            a = e->event_pool.back().first;
            b = e->event_pool.back().second;
            e->event_pool.pop_back();
        } else {
            HCHECK(hipEventCreate(&a));
            HCHECK(hipEventCreate(&b));
        }
    }
    const hipError_t err = launch_rollout_kernel(*k, grid, (unsigned)lds, (int)e->lds_max, e->md, rl, st, a, b);
    if (timed) e->events.emplace_back(a, b);  // recorded (or leaked to the pool) either way
    if (err != hipSuccess) return fail_kind(HIPETS_ERR_RUNTIME, "rollout kernel launch failed: %s", hipGetErrorString(err));
    return 0;
}

// persistent form or one launch per step, for a DEVICE rollout of `logical` workgroups (residency.hpp decide_launch_form)
int launch_form(hipets_engine* e, int R, int logical, size_t lds, RolloutArgs ra, hipStream_t st, bool* persistent, int* capacity = nullptr) {
    ra.lds_bytes = (unsigned)lds;
    KernelRec* k = rollout_instance(e, R, ra);
    if (!k) return 1;
    HCHECK(decide_launch_form(*k, logical, (unsigned)lds, (int)e->lds_max, e->num_cu, e->md, ra, e->census.as<int>(), e->poll_ticks, st, &e->persistent_ok, persistent, capacity));
    return 0;
}

// wide: the call will run a KSpec::WIDE instance (launch.hpp wide_model + lean_call): hidden-width activation buffers, the input
// image with its own stride in buf0
size_t lds_for(const hipets_engine* e, int R, int horizon, bool wide = false) {
    const ModelDev& md = e->md;
    if (wide)
        return rollout_smem_bytes(kTile * R, lean_ld(md.hidC, md.hidC), md.obs_dim, md.act_dim, md.in_dim, md.out_dim, md.out_total, horizon, false,
                                  md.lv_rows, md.ld_in);
    return rollout_smem_bytes(kTile * R, md.ld, md.obs_dim, md.act_dim, md.in_dim, md.out_dim, md.out_total, horizon,
                              md.propagation == HIPETS_PROP_EXPECTATION, md.lv_rows);
}

// Cost model for the row-tile count R of a workgroup (DESIGN.md "Choosing R"), in units of "one MFMA unit through a layer's k loop"
// (~2.7 us per step at hid 200).  A workgroup's step costs a + units(R): `units` = MFMA units per k-chunk of its busiest wave
// (hid 200: 4, 7, 10, 13 for R = 1..4), a ~ 1.8 = what a step spends outside the k loops (epilogues, tail, set-up, barriers).
// A CU holds two workgroups of an R <= 2 instance at once (256 registers each) and their fixed parts hide behind each other's MFMAs:
// a pair costs a + 2 units; R >= 3 instances own the CU (512 registers) and their workgroups run one after the other.  A (shape, R)
// pair without a shape-specialised instance (launch.hpp lean_shape_exists) runs the hidden-static or the generic kernel: + 8 %.
// `drift`: the workgroups of the launch do not wait for each other (FAST mode: one launch for the horizon, no hand-over).  Two of them
// on a CU then drift apart and their heavy waves stop meeting on a SIMD: a pair costs a + 2 x the AVERAGE units per SIMD (C R / 4: 3.25
// instead of 4 per row tile at hid 200).  Step-synchronous launches (DEVICE / EXACT: hand-over or one launch per step) pay the busiest one.
// Calibrated on MI355X (profiles/r4_stock_workloads.json, r4_learned_reward_workloads.json, r4_device_r_sweep.json: every R forced, 12
// workloads, both modes -- the rule picks the fastest R in 23 of the 24 cases and loses 0.3 % in the other).

int wave_units(int C, int R) {  // MFMA units per k-chunk of the busiest SIMD (waves w and w + 4 share SIMD w % 4)
    const int full = C / kWaves, rem = C % kWaves, nu = rem * R;
    int simd[4] = {0, 0, 0, 0};
    for (int w = 0; w < kWaves; ++w) simd[w % 4] += full * R + (w < nu ? (nu - w + kWaves - 1) / kWaves : 0);
    return std::max(std::max(simd[0], simd[1]), std::max(simd[2], simd[3]));
}

int choose_R(const hipets_engine* e, long long tiles_total_per_slice, int slices, int forced, int horizon, bool wide, bool drift) {
    if (forced > 0) return forced;
    const int C = e->md.hidC;
    // the fixed part scales with the layer width like the units do.  WIDE instances (Humanoid-v4: 47 output column tiles, one workgroup per
    // CU) carry their output layer and its tail in it: a round of two-tile workgroups costs 1.29 x a round of one-tile ones in FAST mode,
    // 1.45 x in the turn-based DEVICE form (profiles/r5_cfg4p_iterations.json: the five population sizes of the cfg4' iCEM plan, both R)
    const double a = (wide ? (drift ? 6.45 : 2.67) : 1.77) * (double)C / 13.0;
    int best = 1;
    double best_cost = 1e300;
    // bf16x3 / bf16 arithmetic exists in shape-specialised instances only: among the R that have one (if any has: else the launch reports it)
    bool b3_only = false;
    if (e->md.precision != HIPETS_PREC_F32)
        for (int R = 1; R <= kMaxR; ++R) b3_only = b3_only || b3_shape_exists(e->md, R);
    for (int R = 1; R <= kMaxR; ++R) {
        if (lds_for(e, R, horizon, wide) > e->lds_max) break;
        if (wide && R > 2) break;  // WIDE instances exist for R = 1, 2 (rollout_inst.inc)
        if (b3_only && !b3_shape_exists(e->md, R)) continue;
        const long long groups = (tiles_total_per_slice + R - 1) / R;
        const long long nwg = groups * slices;
        const long long n = (nwg + e->num_cu - 1) / e->num_cu;  // workgroups the busiest CU serves
        const int co = (R <= 2 && !wide) ? 2 : 1;               // ... of which it holds this many at once
        const double u = wave_units(C, R);
        const double u_pair = (co == 2 && drift) ? (double)C * R / 4.0 : u;
        const long long full = n / co, rem = n % co;
        double cost = (double)full * (a + co * u_pair) + (rem ? a + (double)rem * u : 0.0);
        if (!lean_shape_exists(e->md, R)) cost *= 1.08;
        if (cost < best_cost - 1e-9) {
            best_cost = cost;
            best = R;
        }
    }
    return best;
}

// The launch geometry of one rollout / step call: everything the launch of the rollout kernel is sized by.
enum class GeoCall { rollout, step, query };  // hipets_rollout, hipets_step, or a query of hipets_rollout's geometry (no launch)
struct Geometry {
    int domains;         // member domains: M for EXACT / DEVICE (1 under expectation propagation), 1 for FAST
    long long rpd;       // rows per domain: B / domains, or opts.rows_per_member (EXACT with per-row member maps)
    long long tiles;     // row tiles per domain
    bool wide;           // the KSpec::WIDE layout (RolloutArgs::wide_lds)
    bool whole_horizon;  // the FAST form: one launch for the horizon (RolloutArgs::whole_horizon); else step-synchronous, state in HBM
    int R;               // row tiles per workgroup
    int groups;          // workgroups per domain
    size_t lds;          // dynamic LDS bytes
};

// `probe`: the RolloutArgs the launcher's lean_call will see (in-kernel draws / injected eps, traces, generic_only); `rows_per_member`:
// opts.rows_per_member (0 for queries).  hipets_step runs the step-synchronous form in every mode (for ONE step it is the FAST form too,
// and every shape-specialised instance has it) and never the WIDE layout.
int rollout_geometry(const hipets_engine* e, int mode, long long B, int rows_per_member, int H, int rows_per_group, GeoCall call,
                     const RolloutArgs& probe, Geometry* g) {
    const ModelDev& md = e->md;
    const bool fast = mode == HIPETS_MODE_FAST;
    const bool expectation = md.propagation == HIPETS_PROP_EXPECTATION;
    g->domains = (fast || expectation) ? 1 : md.M;
    const bool slots = mode == HIPETS_MODE_EXACT && !expectation && rows_per_member > 0;
    g->rpd = slots ? rows_per_member : B / g->domains;
    g->tiles = (g->rpd + kTile - 1) / kTile;
    g->whole_horizon = fast && call != GeoCall::step;
    g->wide = call != GeoCall::step && rows_per_group <= 2 && wide_model(md) && lean_call(md, probe);
    // (a caller-sized member schedule follows hipets_fast_geometry: the default call's geometry -- the WIDE instance's where one will run;
    // rows_per_group = -1 asks for the general layout's, which is what calls with injected eps / traces run)
    if (g->whole_horizon && !g->wide && wide_model(md) && probe.schedule && rows_per_group == 0)
        return fail("this call runs the general kernel layout (injected eps / traces / generic_kernel) on a model whose default geometry is "
                    "the wide-output instance's: size member_schedule with hipets_fast_geometry(rows_per_group = -1) and pass its row-tile "
                    "count as opts->rows_per_group");
    // Only a whole-horizon launch of more than one step drifts apart.
    const bool drift = g->whole_horizon && H > 1;
    g->R = choose_R(e, g->tiles, g->domains, rows_per_group, H, g->wide, drift);
    g->lds = lds_for(e, g->R, H, g->wide);
    if (g->lds > e->lds_max) return fail("rows_per_group %d does not fit LDS", g->R);
    g->groups = (int)((g->tiles + g->R - 1) / g->R);
    if (fast && call != GeoCall::query && g->groups > 8000)
        return fail("FAST mode supports at most 8000 workgroups per launch (got %d)%s", g->groups, call == GeoCall::rollout ? "; shard the population" : "");
    return 0;
}

// The member maps of an EXACT / DEVICE call (hipets_rollout, hipets_step): per step ONE balanced permutation of all B rows, slot j ->
// member j / (B / M) (gaussian_mlp.py:164-166, 203-205), or explicit per-row member maps (padded member slots, opts.rows_per_member):
// what BasicEnsemble draws with randint (basic_ensemble.py:122-129) and mbrl.util.math.propagate_from_indices expresses (util/math.py:
// 180-196), accepted for GaussianMLP models too (any batch size, members may own unequal row counts).
int check_member_maps(const hipets_engine* e, const hipets_rollout_opts* o, long long B, bool one_step) {
    const ModelDev& md = e->md;
    const bool device = o->mode == HIPETS_MODE_DEVICE;
    const bool expectation = md.propagation == HIPETS_PROP_EXPECTATION;
    const bool slots = o->mode == HIPETS_MODE_EXACT && !expectation && o->rows_per_member > 0;
    // the reference's ValueError (gaussian_mlp.py:195-200), raised for every propagation method.  hipets_step raises it in every mode and
    // exempts every EXACT call with rows_per_member
    const bool exempt = one_step ? o->mode == HIPETS_MODE_EXACT && o->rows_per_member > 0 : slots;
    if (!md.iid_members && !exempt && B % md.M != 0)
        return fail("GaussianMLP ensemble requires batch size to be a multiple of the number of models. "
                    "Current batch size is %lld for %d models.", B, md.M);
    if ((o->mode != HIPETS_MODE_EXACT && !device) || expectation) return 0;
    if (device && md.iid_members) return fail("DEVICE mode has no BasicEnsemble (iid member map) variant: use FAST, or EXACT with injected maps");
    if (!device && !o->perms) return fail("EXACT mode with random_model/fixed_model propagation needs opts.perms");
    if ((md.iid_members && !device && !slots) || (slots && o->rows_per_member > B))
        return fail("EXACT mode with per-row member maps needs opts.rows_per_member in [1, B] (padded member slots)");
    return 0;
}

// The binding from a call's mode to the kernel's arguments, for hipets_rollout and hipets_step alike: where the randomness comes from,
// then the geometry (which looks at those fields: rollout_geometry's `probe`), then what the kernel takes from the geometry.
//   DEVICE  a keyed bijection and Philox normals in-kernel (no input tensors, no host work); the permutation is keyed by
//           (o->seed, perm_stream, perm_step)
//   EXACT   the permutations and eps come from the caller (the reference's own draws)
//   FAST    workgroup w runs the member the FAST rule gives it: the caller's schedule, or (null) every workgroup draws its own entries in
//           its prologue (common.hpp fast_member).  One step (hipets_step): B independent rows, workgroup w owns rows [w * 16 R,
//           (w + 1) * 16 R) -- the step-synchronous form with the identity permutation (one domain of B rows) and RolloutArgs::fast_members
int bind_mode(const hipets_engine* e, const hipets_rollout_opts* o, long long B, int H, GeoCall call, uint64_t perm_stream, uint32_t perm_step,
              RolloutArgs* ra, Geometry* g) {
    const bool expectation = e->md.propagation == HIPETS_PROP_EXPECTATION;
    const bool fast = o->mode == HIPETS_MODE_FAST;
    if (o->mode == HIPETS_MODE_DEVICE) {
        ra->use_philox = o->no_sample ? 0 : 1;
        if (!expectation) {
            ra->perm_n = (unsigned)B;
            perm_radices((uint32_t)B, &ra->perm_a, &ra->perm_b);
            ra->perm_keys = perm_round_keys(perm_key(o->seed, perm_stream, perm_step));
        }
    } else if (o->mode == HIPETS_MODE_EXACT) {
        ra->perm = expectation ? nullptr : reinterpret_cast<const long long*>(o->perms);
        ra->eps = o->eps;
    } else if (fast) {
        ra->eps = o->fast_eps;
        ra->use_philox = (o->fast_eps || o->no_sample) ? 0 : 1;
        ra->schedule = expectation ? nullptr : o->member_schedule;
        ra->fast_members = call == GeoCall::step ? 1 : 0;
    } else {
        return fail("unknown rollout mode %d", o->mode);
    }
    if (rollout_geometry(e, o->mode, B, o->rows_per_member, H, o->rows_per_group, call, *ra, g)) return 1;
    ra->whole_horizon = g->whole_horizon ? 1 : 0;
    ra->wide_lds = g->wide ? 1 : 0;
    ra->groups = g->groups;
    if (!g->whole_horizon) ra->rows_per_domain = (int)g->rpd;
    if (fast) perm_radices((uint32_t)g->groups, &ra->fm_a, &ra->fm_b);
    return 0;
}

}  // namespace

namespace hipets {

int pack_weights(hipStream_t st, float* dst, const float* src, const int* members, int M, int K, int N, int Kp, int Np, long long member_stride,
                 long long layer_off, int permute_cols, int src_nk, int head_dim) {
    const long long n = (long long)Kp * Np * M;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, members, M, K, N, Kp, Np, member_stride, layer_off,
                       permute_cols, src_nk, head_dim);
    HCHECK(hipGetLastError());
    return 0;
}

int pack_weights_b3(hipStream_t st, uint4* dst, const float* src, const int* members, int M, int K, int N, int Kp32, int Np, long long member_stride,
                    long long layer_off, int src_nk, int pieces) {
    const long long n3 = (long long)(Np / 16) * (Kp32 / 32) * pieces * 64 * M;
    hipLaunchKernelGGL(pack_weights_b3_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, dst, src, members, M, K, N, Kp32, Np, member_stride,
                       layer_off, src_nk, pieces);
    HCHECK(hipGetLastError());
    return 0;
}

int pack_bias(hipStream_t st, float* dst, const float* src, const int* members, int M, int N, int Np, int member_stride, int layer_off, int permute_cols,
              int head_dim) {
    const int nb = M * Np;
    hipLaunchKernelGGL(pack_bias_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, dst, src, members, M, N, Np, member_stride, layer_off, permute_cols, head_dim);
    HCHECK(hipGetLastError());
    return 0;
}

int launch_particle_reduce(const hipets_engine* e, const float* totals, float* returns, int pop, int P, hipStream_t st) {
    hipLaunchKernelGGL(particle_mean_kernel, dim3((pop + 255) / 256), dim3(256), 0, st, totals, returns, pop, P, e->reduce);
    HCHECK(hipGetLastError());
    return 0;
}

int plan_step_keys(hipets_engine* e, int H, int iters, uint64_t seed, uint64_t first_stream, hipStream_t st) {
    if (e->md.propagation != HIPETS_PROP_RANDOM_MODEL || iters < 1 || e->plan_mode != HIPETS_MODE_DEVICE || !e->persistent_ok) return 0;
    if (e->plan_keys.ensure((size_t)iters * H * sizeof(PermKeys))) return 1;
    hipLaunchKernelGGL(step_keys_kernel, dim3((H + 63) / 64, iters), dim3(64), 0, st, e->plan_keys.as<PermKeys>(), H, (unsigned long long)seed,
                       (unsigned long long)first_stream);
    HCHECK(hipGetLastError());
    e->plan_keys_seed = seed; e->plan_keys_first = first_stream; e->plan_keys_count = iters; e->plan_keys_H = H;
    return 0;
}

int rollout_impl(hipets_engine* e, const float* actions, const float* s0, int32_t pop, int32_t H, int32_t P,
                 const hipets_rollout_opts* o, float* returns, void* stream) {
    if (!e || !e->has_model) return fail("engine has no model (call hipets_set_model)");
    if (!actions || !o) return fail("null argument");  // (returns == nullptr: internal callers that fold the particle mean)
    if (pop < 1 || H < 1 || P < 1) return fail("bad pop/horizon/particles");
    if (check_reduce(e, P)) return 1;
    if (e->error_flag && *e->error_flag) {  // raised by an EARLIER launch: its returns were garbage
        *e->error_flag = 0;
        e->persistent_ok = false;  // fall back to one launch per step from now on
        return fail_kind(HIPETS_ERR_TIMEOUT, "a persistent DEVICE-mode rollout timed out waiting for rows of another workgroup (its workgroups were not all "
                    "resident) and nobody asked (hipets_check_async_error after the results were read): the results of that earlier "
                    "call are invalid.  Persistent launches are now disabled for this engine.");
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);  // (the public entry point that led here holds the StreamScope)
    HCHECK(hipSetDevice(e->device));
    const ModelDev& md = e->md;
    const long long B = (long long)pop * P;
    if (B > 0x7FFFFFFF / std::max(md.obs_dim, md.out_dim)) return fail("batch too large");
    if (o->rows_per_group < 0 || o->rows_per_group > kMaxR) return fail("rows_per_group outside [0, %d]", kMaxR);

    const int n_env = o->n_env > 1 ? o->n_env : 1;
    if (n_env > 1 && ((o->mode != HIPETS_MODE_FAST && o->mode != HIPETS_MODE_DEVICE) || pop % n_env != 0))
        return fail("n_env %d needs FAST or DEVICE mode and a population (%d) divisible by it", n_env, pop);
    if (e->s0.ensure((size_t)n_env * md.obs_dim * 4)) return 1;
    if (e->totals.ensure((size_t)B * 4)) return 1;
    if (s0 && stage_h2d(e, e->s0.p, s0, (size_t)n_env * md.obs_dim * 4, st)) return 1;

    RolloutArgs ra{};
    ra.pop = pop; ra.P = P; ra.H = H; ra.B = (int)B;
    ra.actions = actions;
    ra.s0 = e->s0.as<float>();
    ra.totals = e->totals.as<float>();
    ra.seed = o->seed;
    ra.stream_id = o->stream_id;
    ra.trace_next_obs = o->trace_next_obs;
    ra.trace_rewards = o->trace_rewards;
    ra.phase_cycles = reinterpret_cast<long long*>(o->phase_cycles);
    ra.pop_env = n_env > 1 ? pop / n_env : 0;
    ra.generic_only = o->generic_kernel;

    const bool device = o->mode == HIPETS_MODE_DEVICE;
    if ((device || o->mode == HIPETS_MODE_EXACT) && check_member_maps(e, o, B, false)) return 1;
    Geometry g;
    // (DEVICE: the permutation key of fixed_model; random_model re-keys per step below)
    if (bind_mode(e, o, B, H, GeoCall::rollout, o->stream_id, 0xFFFFFFFFu, &ra, &g)) return 1;
    if (o->mode != HIPETS_MODE_FAST) {
        const int R = g.R, domains = g.domains, groups = g.groups;
        const size_t lds = g.lds;
        if (!device && md.propagation == HIPETS_PROP_RANDOM_MODEL) ra.perm_step = (long long)domains * g.rpd;
        // rows change workgroups between steps only when a fresh permutation is drawn per step: one launch per step then
        // (state through HBM); TS-infinity / expectation rollouts of DEVICE mode keep their rows and run as ONE launch
        const bool per_step = !device || md.propagation == HIPETS_PROP_RANDOM_MODEL;
        if (e->state.ensure((size_t)B * md.obs_dim * 4) || e->term.ensure((size_t)B)) return 1;
        ra.state = e->state.as<float>();
        ra.term = e->term.as<unsigned char>();
        // DEVICE + random_model: ONE launch for the horizon, rows handed over between workgroups through the tagged-granule
        // table.  Only as many workgroups as are resident at once are launched; a batch with more logical workgroups (cfg4: 435)
        // is served in turns, workgroup b taking b, b + grid, ... every step.
        bool persistent = device && per_step && e->persistent_ok && H > 1;
        // the resident-heads instance (KSpec::RES) where the launch can be a STRAIGHT persistent one: it is asked for first, and kept only if
        // all logical workgroups of the call are co-resident in it; the plain instance -- turns, or one launch per step -- otherwise
        ra.resident_heads = persistent && !g.wide && resident_heads_call(md, R, domains * groups, e->num_cu, H) ? 1 : 0;
        if (ra.resident_heads) {
            int capacity = 0;
            if (launch_form(e, R, domains * groups, lds, ra, st, &persistent, &capacity)) return 1;
            if (!resident_heads_kept(persistent, capacity, domains * groups)) {
                ra.resident_heads = 0;
                persistent = e->persistent_ok;
            }
        }
        if (persistent && !ra.resident_heads && launch_form(e, R, domains * groups, lds, ra, st, &persistent)) return 1;
        if (!persistent) {  // the persistent form starts from s0 itself and writes every row's total at the end
            hipLaunchKernelGGL(init_state_kernel, dim3((unsigned)((B * md.obs_dim + 255) / 256)), dim3(256), 0, st,
                               e->state.as<float>(), e->totals.as<float>(), e->term.as<unsigned char>(), e->s0.as<float>(), (int)B,
                               md.obs_dim, P, ra.pop_env);
            HCHECK(hipGetLastError());
        }
        if (persistent) {
            const size_t nv = 2 * ((size_t)(md.obs_dim + 1) / 2 + 1);  // granules per row: the state dims padded to pairs, then {total, flag}
            const size_t cap_before = e->exchange.cap;
            if (e->exchange.ensure((size_t)B * nv * 8)) return 1;
            // hand-over tags grow monotonically across launches (step t of this launch: tag_base + t + 1), so a granule left by an
            // earlier rollout can never pass for this one's: the table is cleared only when it is new or the 32-bit tag would wrap
            if (e->exchange.cap != cap_before || e->tag_base > 0xFFFFFFFFu - 2u * (uint32_t)H - 2u) {
                HCHECK(hipMemsetAsync(e->exchange.p, 0, e->exchange.cap, st));
                e->tag_base = 0;
            }
            ra.tag_base = e->tag_base;
            e->tag_base += (uint32_t)H;
            ra.exchange = e->exchange.as<unsigned long long>();
            const uint64_t sid = o->stream_id;
            if (e->plan_keys.p && o->seed == e->plan_keys_seed && H == e->plan_keys_H && sid >= e->plan_keys_first &&
                sid - e->plan_keys_first < (uint64_t)e->plan_keys_count) {
                ra.step_keys = e->plan_keys.as<PermKeys>() + (size_t)(sid - e->plan_keys_first) * H;  // generated by the plan's prologue
            } else {
                if (e->step_keys.ensure((size_t)H * sizeof(PermKeys))) return 1;
                hipLaunchKernelGGL(step_keys_kernel, dim3((H + 63) / 64), dim3(64), 0, st, e->step_keys.as<PermKeys>(), H, (unsigned long long)o->seed,
                                   (unsigned long long)o->stream_id);
                HCHECK(hipGetLastError());
                ra.step_keys = e->step_keys.as<PermKeys>();
            }
            ra.error_flag = e->error_flag;
            ra.poll_ticks = e->poll_ticks;
            ra.t_begin = 0;
            ra.t_end = H;
            ra.n_logical = domains * groups;
            // KSpec::WIDE two-tile instances deal a ragged last turn in one-tile logical workgroups (rollout.hpp "Ragged last turn": same
            // bits, 0.69 of the turn's time); HIPETS_RAGGED_LAST_TURN=0 keeps two-tile turns throughout (A/B measurements)
            static const bool ragged_ok = [] { const char* v = std::getenv("HIPETS_RAGGED_LAST_TURN"); return !(v && v[0] == '0'); }();
            ra.ragged_last_turn = (g.wide && R == 2 && ragged_ok) ? 1 : 0;

            if (launch_rollout(e, R, domains * groups, lds, ra, st)) return 1;  // cut to the resident capacity by the launcher
        } else if (per_step) {
            for (int t = 0; t < H; ++t) {
                ra.t_begin = t;
                ra.t_end = t + 1;
                if (ra.perm_n) ra.perm_keys = perm_round_keys(perm_key(o->seed, o->stream_id, (uint32_t)t));  // this step's permutation
                if (launch_rollout(e, R, domains * groups, lds, ra, st)) return 1;
            }
        } else {
            ra.t_begin = 0;
            ra.t_end = H;
            if (launch_rollout(e, R, domains * groups, lds, ra, st)) return 1;
        }
    } else {
        const int nwg = g.groups;
        if (o->member_schedule && o->member_schedule_len != 0 && (long long)o->member_schedule_len != (long long)H * nwg)
            return fail("member_schedule holds %d entries, this call's geometry is horizon %d x %d workgroups (hipets_fast_geometry)",
                        o->member_schedule_len, H, nwg);
        ra.t_begin = 0;
        ra.t_end = H;
        if (launch_rollout(e, g.R, nwg, g.lds, ra, st)) return 1;
    }
    if (!returns) return 0;  // the caller reduces e->totals over the particles itself (hipets_plan_cem: inside the refit kernel)
    return launch_particle_reduce(e, e->totals.as<float>(), returns, pop, P, st);
}

// Which PlaNet kernel instance a launch on this engine runs: the STATIC one for models with conf's tile counts (planet_static_shape, decided
// at hipets_planet_set_model), unless HIPETS_PLANET_GENERIC=1 asks for the run-time generic instance whatever the shapes -- tests compare
// the two bit for bit.  The one rule of planet_rollout_impl's launch and of hipets_planet_kernel_class.
static bool planet_launches_static(const hipets_engine* e) {
    const char* pg = std::getenv("HIPETS_PLANET_GENERIC");
    return e->planet_static && !(pg && pg[0] == '1');
}

int planet_rollout_impl(hipets_engine* e, const float* actions, const float* latent0, const float* belief0, int32_t pop, int32_t H,
                        int32_t P, const hipets_planet_opts* o, float* returns, hipStream_t st) {
    if (check_reduce(e, P)) return 1;
    const int n_env = std::max(o->n_env, 1);
    if (o->n_env < 0 || n_env > 4096) return fail("n_env %d outside [0, 4096]", o->n_env);
    if (pop % n_env) return fail("PlaNet rollout: population %d is not divisible by n_env %d", pop, n_env);
    const long long B = (long long)pop * P;
    if (B > 0x7FFFFFFF / std::max(e->pd.belief, 16)) return fail("batch too large");
    if (e->totals.ensure((size_t)B * 4)) return 1;
    PlanetArgs ra{};
    ra.pop = pop; ra.P = P; ra.H = H; ra.B = (int)B;
    ra.n_env = n_env;
    ra.rows_env = pop / n_env * P;
    ra.actions = actions;
    ra.latent0 = latent0;
    ra.belief0 = belief0;
    ra.totals = e->totals.as<float>();
    ra.eps = o->eps;
    ra.use_philox = (o->eps || o->no_sample) ? 0 : 1;
    ra.seed = o->seed;
    ra.stream_id = o->stream_id;
    ra.trace_latent = o->trace_latent;
    ra.trace_belief = o->trace_belief;
    ra.trace_rewards = o->trace_rewards;
    ra.phase_cycles = reinterpret_cast<long long*>(o->phase_cycles);
    const size_t lds = planet_smem_bytes(e->pd.ld);
    const int nwg = (int)((B + kTile - 1) / kTile);
    HCHECK(launch_planet_rollout(nwg, (unsigned)lds, (int)e->lds_max, e->pd, ra, st, planet_launches_static(e)));
    if (!returns) return 0;
    return launch_particle_reduce(e, e->totals.as<float>(), returns, pop, P, st);
}

}  // namespace hipets

extern "C" {

int hipets_fast_geometry(hipets_engine* e, int32_t pop, int32_t P, int32_t horizon, int32_t rows_per_group,
                         int32_t* n_workgroups, int32_t* row_tiles) {
    if (!e || !e->has_model) return fail("engine has no model");
    if (pop < 1 || P < 1) return fail("bad pop/P");
    if (rows_per_group < -1 || rows_per_group > kMaxR) return fail("rows_per_group outside [-1, %d]", kMaxR);
    RolloutArgs probe{};  // a default call: in-kernel draws, nothing injected or traced; -1: a call that runs the general layout
    probe.use_philox = 1;
    probe.generic_only = rows_per_group < 0 ? 1 : 0;
    Geometry g;
    if (rollout_geometry(e, HIPETS_MODE_FAST, (long long)pop * P, 0, horizon, std::max(rows_per_group, 0), GeoCall::query, probe, &g)) return 1;
    if (n_workgroups) *n_workgroups = g.groups;
    if (row_tiles) *row_tiles = g.R;
    return 0;
}

int hipets_kernel_class(hipets_engine* e, int32_t pop, int32_t P, int32_t horizon, int32_t mode, int32_t rows_per_group, int32_t* kernel_class,
                        int32_t* row_tiles) {
    if (!e || !e->has_model) return fail("engine has no model");
    if (pop < 1 || P < 1 || horizon < 1) return fail("bad pop/horizon/particles");
    if (rows_per_group < 0 || rows_per_group > kMaxR) return fail("rows_per_group outside [0, %d]", kMaxR);
    if (mode != HIPETS_MODE_FAST && mode != HIPETS_MODE_DEVICE) return fail("hipets_kernel_class: mode must be HIPETS_MODE_FAST or HIPETS_MODE_DEVICE");
    const ModelDev& md = e->md;
    const long long B = (long long)pop * P;
    if (mode == HIPETS_MODE_DEVICE && md.propagation != HIPETS_PROP_EXPECTATION) {
        if (md.iid_members && md.M > 1) return fail("DEVICE mode has no BasicEnsemble (iid member map) variant");
        if (B % md.M != 0) return fail("GaussianMLP ensemble requires batch size to be a multiple of the number of models. "
                                       "Current batch size is %lld for %d models.", B, md.M);
    }
    RolloutArgs probe{};  // what a default call's arguments look like to the launcher: in-kernel draws, nothing injected or traced
    probe.use_philox = 1;
    Geometry g;
    if (rollout_geometry(e, mode, B, 0, horizon, rows_per_group, GeoCall::query, probe, &g)) return fail("the model does not fit LDS");
    probe.whole_horizon = g.whole_horizon ? 1 : 0;
    probe.wide_lds = g.wide ? 1 : 0;
    int cls = HIPETS_KERNEL_GENERIC;
    switch (pick_rollout_instance(md, probe, g.R)) {
        case RolloutInstance::lean: case RolloutInstance::lean_resident: case RolloutInstance::b3: cls = HIPETS_KERNEL_FUSED; break;
        case RolloutInstance::bf16: cls = HIPETS_KERNEL_BF16; break;
        case RolloutInstance::lean_wide: cls = HIPETS_KERNEL_WIDE; break;
        case RolloutInstance::hidden_static: cls = HIPETS_KERNEL_HIDDEN_STATIC; break;
        case RolloutInstance::generic_silu: case RolloutInstance::generic: break;
        case RolloutInstance::no_b3: return fail("bf16x3 arithmetic exists for the shape-specialised instances only");
        case RolloutInstance::no_bf16: return fail("bf16 arithmetic exists for the shape-specialised instances only");
        case RolloutInstance::no_wide: return fail("no WIDE instance of this model's shape for R = %d", g.R);
    }
    if (kernel_class) *kernel_class = cls;
    if (row_tiles) *row_tiles = g.R;
    return 0;
}

int hipets_rollout(hipets_engine* e, const float* actions, const float* s0, int32_t pop, int32_t H, int32_t P,
                   const hipets_rollout_opts* o, float* returns, void* stream) {
    if (!e || !s0) return fail("null argument");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    return rollout_impl(e, actions, s0, pop, H, P, o, returns, stream);
}

int hipets_step(hipets_engine* e, const float* obs, const float* actions, int32_t B, const hipets_rollout_opts* o, float* next_obs,
                float* rewards, uint8_t* dones, void* stream) {
    if (!e || !e->has_model) return fail("engine has no model (call hipets_set_model)");
    if (!obs || !actions || !o || !next_obs || !rewards || !dones) return fail("null argument");
    if (B < 1) return fail("bad batch");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const ModelDev& md = e->md;
    if (o->rows_per_group < 0 || o->rows_per_group > kMaxR) return fail("rows_per_group outside [0, %d]", kMaxR);
    if (check_member_maps(e, o, B, true)) return 1;
    RolloutArgs ra{};
    ra.pop = B; ra.P = 1; ra.H = 1; ra.B = B;
    ra.actions = actions;
    ra.state = next_obs;  // the kernel updates state / totals / terminated in place: it runs on the caller's output buffers
    ra.totals = rewards;
    ra.term = dones;
    ra.seed = o->seed;
    ra.stream_id = o->stream_id;
    ra.generic_only = o->generic_kernel;
    ra.t_begin = 0;
    ra.t_end = 1;
    // DEVICE, random_model: the permutation of (seed, stream_id), step 0.  fixed_model (a ModelEnv.step of a TS-infinity rollout keeps
    // its member map while the eps change): the TS-infinity permutation of (seed, perm_stream_id) -- the stream of the reset --
    // next to eps drawn from (seed, stream_id), the stream of the step
    const bool fixed = md.propagation == HIPETS_PROP_FIXED_MODEL;
    const uint64_t pstream = (fixed && o->perm_stream_id) ? o->perm_stream_id : o->stream_id;
    Geometry g;
    if (bind_mode(e, o, B, 1, GeoCall::step, pstream, fixed ? 0xFFFFFFFFu : 0u, &ra, &g)) return 1;
    if (o->mode == HIPETS_MODE_FAST && o->member_schedule && o->member_schedule_len != 0 && o->member_schedule_len != g.groups)
        return fail("member_schedule holds %d entries, this call's geometry is %d workgroups (hipets_fast_geometry with rows_per_group -1)",
                    o->member_schedule_len, g.groups);
    HCHECK(hipMemcpyAsync(next_obs, obs, (size_t)B * md.obs_dim * 4, hipMemcpyDeviceToDevice, st));
    HCHECK(hipMemsetAsync(rewards, 0, (size_t)B * 4, st));
    HCHECK(hipMemsetAsync(dones, 0, (size_t)B, st));
    return launch_rollout(e, g.R, g.domains * g.groups, g.lds, ra, st);
}

int hipets_trajectory_returns(hipets_engine* e, const float* rewards, const uint8_t* dones, int32_t pop, int32_t H, int32_t P, float* returns,
                              float* row_totals, int32_t* first_done, void* stream) {
    if (!e || !rewards || !dones || !returns) return fail("null argument");
    if (pop < 1 || H < 1 || P < 1) return fail("bad pop/horizon/particles");
    const long long B = (long long)pop * P;
    if (B > 0x7FFFFFFF) return fail("batch too large");
    if (check_reduce(e, P)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);  // (the two-pass form below may run on the engine's row totals)
    return launch_trajectory_returns<false>(e, rewards, dones, nullptr, 1.0f, pop, H, P, returns, row_totals, first_done, st);
}

int hipets_particle_reduce(hipets_engine* e, const float* totals, int32_t pop, int32_t num_particles, float* returns, void* stream) {
    if (!e || !totals || !returns) return fail("null argument");
    if (pop < 1 || num_particles < 1) return fail("bad pop/particles");
    if ((long long)pop * num_particles > 0x7FFFFFFF) return fail("batch too large");
    if (check_reduce(e, num_particles)) return 1;
    HCHECK(hipSetDevice(e->device));
    return launch_particle_reduce(e, totals, returns, pop, num_particles, reinterpret_cast<hipStream_t>(stream));
}

int hipets_fast_schedule(hipets_engine* e, int32_t H, int32_t nwg, uint64_t seed, uint64_t stream_id, int32_t* schedule,
                         void* stream) {
    if (!e || !e->has_model) return fail("engine has no model");
    if (!schedule || H < 1 || nwg < 1) return fail("bad argument");
    HCHECK(hipSetDevice(e->device));
    uint32_t fa, fb;
    perm_radices((uint32_t)nwg, &fa, &fb);
    hipLaunchKernelGGL(member_schedule_kernel, dim3((unsigned)((nwg + 255) / 256), H), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), schedule, nwg, fa, fb,
                       e->md.M, e->md.propagation == HIPETS_PROP_FIXED_MODEL ? 1 : 0, e->md.iid_members, (unsigned long long)seed,
                       (unsigned long long)stream_id);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_fast_normals(hipets_engine* e, int32_t H, int32_t B, uint64_t seed, uint64_t stream_id, float* normals, void* stream) {
    if (!e || !e->has_model) return fail("engine has no model");
    if (!normals || H < 1 || B < 1) return fail("bad argument");
    HCHECK(hipSetDevice(e->device));
    const long long n = (long long)H * B * ((e->md.out_dim + 3) / 4);
    hipLaunchKernelGGL(export_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       normals, H, B, e->md.out_dim, (unsigned long long)seed, (unsigned long long)stream_id);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_device_perms(hipets_engine* e, int32_t H, int32_t B, uint64_t seed, uint64_t stream_id, int64_t* perms, void* stream) {
    if (!e || !e->has_model) return fail("engine has no model");
    if (!perms || H < 1 || B < 1) return fail("bad argument");
    HCHECK(hipSetDevice(e->device));
    uint32_t a, b;
    perm_radices((uint32_t)B, &a, &b);
    const int fixed = e->md.propagation == HIPETS_PROP_FIXED_MODEL ? 1 : 0;
    const int rows = fixed ? 1 : H;
    const long long n = (long long)rows * B;
    hipLaunchKernelGGL(export_perms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<long long*>(perms), rows, (unsigned)B, a, b, fixed, (unsigned long long)seed,
                       (unsigned long long)stream_id);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_planet_rollout(hipets_engine* e, const float* actions, const float* latent0, const float* belief0, int32_t pop, int32_t H,
                          int32_t P, const hipets_planet_opts* o, float* returns, void* stream) {
    if (!e || !e->has_planet) return fail("engine has no PlaNet model (call hipets_planet_set_model)");
    if (!actions || !latent0 || !belief0 || !o || !returns) return fail("null argument");
    if (pop < 1 || H < 1 || P < 1) return fail("bad pop/horizon/particles");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    return planet_rollout_impl(e, actions, latent0, belief0, pop, H, P, o, returns, st);
}

int hipets_planet_kernel_class(hipets_engine* e, int32_t* is_static) {
    if (!e || !e->has_planet) return fail("engine has no PlaNet model (call hipets_planet_set_model)");
    if (!is_static) return fail("null argument");
    *is_static = planet_launches_static(e) ? 1 : 0;
    return 0;
}

}  // extern "C"
