// plan.hip -- planning of the C ABI (include/hipets.h): the fused CEM / MPPI / iCEM plans over an ensemble, a sharded ensemble or a
// PlaNet objective, and the stand-alone entry points of the optimizers' kernels (cem.hpp, optim.hpp: this is the one unit that includes them).
#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.hpp"
#include "lds_optin.hpp"
#include "optim.hpp"

using namespace hipets;

namespace {

// MPPI sampling (optim.hpp): whole candidates staged in LDS where one fits, else one thread per series
int launch_mppi_sample(int n_env, int pop, int H, int A, float beta, const float* mean, const float* past_action, const float* lower, const float* upper,
                       const float* z, uint64_t seed, uint64_t stream_id, float* population, hipStream_t st) {
    const long long npop = (long long)n_env * pop;
    const long long D = (long long)H * A;
    if (D <= kMppiSampleMaxD) {
        const int G = mppi_sample_group(npop, (int)D);
        hipLaunchKernelGGL(mppi_sample_staged_kernel, dim3((unsigned)((npop + G - 1) / G)), dim3(kMppiSampleThreads), (size_t)G * D * 4, st, n_env, pop, H, A, G, beta,
                           mean, past_action, lower, upper, z, (unsigned long long)seed, (unsigned long long)stream_id, population);
    } else {
        const long long n = npop * A;
        hipLaunchKernelGGL(mppi_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n_env, pop, H, A, beta, mean, past_action, lower, upper, z,
                           (unsigned long long)seed, (unsigned long long)stream_id, population);
    }
    HCHECK(hipGetLastError());
    return 0;
}

// MPPI update (optim.hpp): the weighted sum stages the population through LDS tiles as large as the CU holds -- the kernel opts in to the
// full LDS once per device, like the rollout kernels
int launch_mppi_update(hipets_engine* e, int n_env, int pop, int D, float gamma, float* values, const float* population, float* mean, hipStream_t st) {
    static LdsOptIn once[2];
    HCHECK(full_lds_once(once[0], reinterpret_cast<const void*>(&mppi_update_kernel<kMppiTileMax / 16>), (int)e->lds_max));
    HCHECK(full_lds_once(once[1], reinterpret_cast<const void*>(&mppi_update_kernel<kMppiTileMax / 32>), (int)e->lds_max));
    const int tile_c = mppi_update_tile(pop, e->lds_max);
    const dim3 grid(mppi_update_blocks(D), n_env);
    if (tile_c == kMppiTileMax)
        hipLaunchKernelGGL(mppi_update_kernel<kMppiTileMax / 16>, grid, dim3(kMppiThreads), mppi_update_smem(pop, tile_c), st, pop, D, gamma, values, population, mean);
    else
        hipLaunchKernelGGL(mppi_update_kernel<kMppiTileMax / 32>, grid, dim3(kMppiThreads), mppi_update_smem(pop, tile_c), st, pop, D, gamma, values, population, mean);
    HCHECK(hipGetLastError());
    return 0;
}

// Plan-level prologue shared by the fused plans: stage the observation(s) once (the same for every iteration) and, for DEVICE-mode
// plans, have the per-step permutation keys of ALL `iters` rollouts (stream ids first_stream, +1, ...) generated in one launch (rollout.hip
// plan_step_keys).  (FAST-mode rollouts need nothing up front: every workgroup draws its own member schedule in its prologue, common.hpp fast_member.)
int plan_prologue(hipets_engine* e, const float* s0, int n_env, int H, int iters, uint64_t seed, uint64_t first_stream, hipStream_t st) {
    const ModelDev& md = e->md;
    if (e->s0.ensure((size_t)n_env * md.obs_dim * 4)) return 1;
    if (stage_h2d(e, e->s0.p, s0, (size_t)n_env * md.obs_dim * 4, st)) return 1;
    return plan_step_keys(e, H, iters, seed, first_stream, st);
}

// candidates of rank r when pop candidates are dealt to `world` ranks (first pop % world ranks hold one more)
inline void shard_bounds(int pop, int world, int r, int* lo, int* hi) {
    const int base = pop / world, extra = pop % world;
    *lo = r * base + std::min(r, extra);
    *hi = *lo + base + (r < extra ? 1 : 0);
}

// hipets_set_plan_trace: record iteration i of a fused plan (population as evaluated, values after the NaN filter, refitted
// mean / dispersion) into the caller's buffers.  A no-op unless a trace is set.
int trace_iter(hipets_engine* e, int i, int rows, size_t nd, const float* population, const float* values, const float* mu,
               const float* disp, hipStream_t st, int n_env = 1) {
    if (!e->has_trace) return 0;
    const hipets_plan_trace& t = e->trace;
    if (rows > t.max_rows) return fail("plan trace: iteration %d evaluates %d candidates, trace buffers hold %d", i, rows, t.max_rows);
    const size_t ne = (size_t)n_env;
    if (t.populations && population)
        HCHECK(hipMemcpyAsync(t.populations + (size_t)i * t.max_rows * nd, population, (size_t)rows * nd * 4, hipMemcpyDeviceToDevice, st));
    if (t.values && values) HCHECK(hipMemcpyAsync(t.values + (size_t)i * t.max_rows, values, (size_t)rows * 4, hipMemcpyDeviceToDevice, st));
    if (t.mus && mu) HCHECK(hipMemcpyAsync(t.mus + (size_t)i * ne * nd, mu, ne * nd * 4, hipMemcpyDeviceToDevice, st));
    if (t.dispersions && disp) HCHECK(hipMemcpyAsync(t.dispersions + (size_t)i * ne * nd, disp, ne * nd * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

CemDev make_cem(const hipets_cem_params* p, int n_env = 1) {
    CemDev c{};
    c.n_env = n_env;
    c.pop = p->population_size;
    c.H = p->horizon;
    c.A = p->act_dim;
    c.D = p->horizon * p->act_dim;
    c.K = p->elite_num;
    c.alpha = (float)p->alpha;
    c.one_minus_alpha = (float)(1.0 - (double)p->alpha);
    c.return_mean = p->return_mean_elites;
    c.clipped = p->clipped_normal;
    c.unbiased = p->unbiased_var;
    return c;
}

int check_cem(const hipets_cem_params* p) {
    if (!p) return fail("null cem params");
    if (p->population_size < 1 || p->population_size > kMaxPop)
        return fail("population_size %d outside [1, %d]", p->population_size, kMaxPop);
    if (p->elite_num < 1 || p->elite_num > p->population_size) return fail("elite_num %d invalid", p->elite_num);
    if (p->unbiased_var && !p->clipped_normal && p->elite_num < 2) {
        // torch.var of one sample is NaN in the reference too; allowed, just flagged by NaN results
    }
    if (p->horizon < 1 || p->act_dim < 1) return fail("bad horizon/act_dim");
    return 0;
}

// Everything that can fail for ONE rank's shard size must fail on EVERY rank, before the first collective (a rank that returned
// early would leave its peers blocked in ncclAllGather): the shards of `rows` candidates hold rows / world or one more, and
// EXACT / DEVICE-mode rollouts of a GaussianMLP ensemble need shard rows % members == 0 (gaussian_mlp.py:195-200) for both sizes.
int check_shards(const hipets_engine* e, const int rows, const int P) {
    const int world = e->comm_world;
    if (rows < world) return fail("population_size %d < world_size %d", rows, world);
    if (e->plan_mode == HIPETS_MODE_DEVICE && !e->md.iid_members) {
        const int base = rows / world, extra = rows % world;
        for (int n : {base, extra ? base + 1 : base})
            if (((long long)n * P) % e->md.M != 0)
                return fail("GaussianMLP ensemble requires batch size to be a multiple of the number of models. A shard of %d candidates x %d "
                            "particles = %lld rows for %d models (population %d over %d ranks).", n, P, (long long)n * P, e->md.M, rows, world);
    }
    return 0;
}

// The objective of one iteration of a sharded plan: `population` holds ALL `rows` candidates (sampled identically on
// every rank: counter-based RNG), this rank rolls out its shard shard_bounds(rows, world, rank) with all particles, ONE
// ncclAllGather of the per-candidate returns (padded to ceil(rows / world) per rank), and e->values [rows] then holds every
// candidate's return on every rank.  The caller has sized e->values / shard_values / gathered.  Returns non-zero only when the
// collective itself failed (RCCL error: the plan is over for everybody); local failures go to *le and the collective still runs.
int sharded_evaluate(hipets_engine* e, const float* population, const int rows, const int H, const int P, const hipets_rollout_opts* ro,
                     void* stream, LocalErr* le) {
    const int world = e->comm_world, rank = e->comm_rank;
    int lo, hi;
    shard_bounds(rows, world, rank, &lo, &hi);
    const int width = (rows + world - 1) / world;
    const size_t nd = (size_t)H * e->md.act_dim;
    float* shard_out = world == 1 ? e->values.as<float>() : e->shard_values.as<float>();
    if (le->ok()) le->note(rollout_impl(e, population + (size_t)lo * nd, nullptr, hi - lo, H, P, ro, shard_out, stream));
    if (world > 1) {  // every rank, every iteration, whatever happened locally
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        if (comm_all_gather(e, (size_t)width, st)) return 1;
        if (le->ok()) le->note(comm_unpad_shards(e, rows, width, st));
    }
    return 0;
}

// The objective a fused plan rolls out every iteration (trajectory_opt.py's obj_fun, model_env.py:145-191), of one of three kinds:
//   ENSEMBLE  the engine's ensemble from HOST observations s0 [n_env, obs_dim], staged once by the plan's prologue;
//   SHARDED   the same over the engine's communicator (one environment): every rank samples all candidates, rolls out its shard and
//             all-gathers the returns (sharded_evaluate);
//   PLANET    the PlaNet latent model from DEVICE start states latent0 [n_env, latent] / belief0 [n_env, belief] (planet.py:656-672,
//             one per environment; nothing to stage, no communicator).
// The plan drivers below are shared; this is where the kinds differ.
struct PlanObjective {
    enum Kind { ENSEMBLE, SHARDED, PLANET } kind = ENSEMBLE;
    const float* s0 = nullptr;
    const float* latent0 = nullptr;
    const float* belief0 = nullptr;

    bool is_planet() const { return kind == PLANET; }
    bool is_sharded() const { return kind == SHARDED; }
    // ranks draw independent rollout randomness (rank 0, and every local plan: `seed` itself)
    uint64_t rollout_seed(const hipets_engine* e, uint64_t seed) const {
        return seed + (is_sharded() ? (uint64_t)e->comm_rank : 0ull) * 0x9E3779B97F4A7C15ull;
    }
    // sharded: the all-gather buffers for the widest iteration (`max_rows` candidates), and (in the prologue) their zeroed padding slot
    size_t shard_width(const hipets_engine* e, int max_rows) const { return (size_t)((max_rows + e->comm_world - 1) / e->comm_world); }
    int reserve_shards(hipets_engine* e, int max_rows) const {
        if (!is_sharded()) return 0;
        const size_t width = shard_width(e, max_rows);
        return e->shard_values.ensure(width * 4) || e->gathered.ensure((size_t)e->comm_world * width * 4);
    }
    int clear_padding(hipets_engine* e, int max_rows, hipStream_t st) const {
        if (is_sharded()) HCHECK(hipMemsetAsync(e->shard_values.p, 0, shard_width(e, max_rows) * 4, st));
        return 0;
    }
    // a local rollout left its per-row totals: the refit kernel reduces them over the particles under the engine's reduction (the rule of
    // particle_mean_kernel: same bits).  A sharded plan's values come from the all-gather.
    void refit_from_totals(hipets_engine* e, CemDev* c, int P) const {
        if (is_sharded()) return;
        c->totals = e->totals.as<float>();
        c->P = P;
        c->reduce = e->reduce;
    }
    // `rows` candidates of ro->n_env environments (environment after environment), iteration ro->stream_id, into `returns` (nullptr:
    // the per-row totals stay in e->totals for the refit; a sharded objective always fills e->values).  Returns non-zero only when a
    // collective failed; a local failure is noted in `le` (skipping the rollout), and a sharded objective still joins the all-gather.
    int evaluate(hipets_engine* e, const float* population, int rows, int H, int P, const hipets_rollout_opts* ro, float* returns,
                 void* stream, LocalErr& le) const {
        if (is_sharded()) return sharded_evaluate(e, population, rows, H, P, ro, stream, &le);
        if (!le.ok()) return 0;
        if (!is_planet()) {
            le.note(rollout_impl(e, population, nullptr, rows, H, P, ro, returns, stream));
            return 0;
        }
        hipets_planet_opts po{};
        po.seed = ro->seed;
        po.stream_id = ro->stream_id;
        po.n_env = ro->n_env;
        le.note(planet_rollout_impl(e, population, latent0, belief0, rows, H, P, &po, returns, reinterpret_cast<hipStream_t>(stream)));
        return 0;
    }
};
PlanObjective ensemble_objective(const float* s0, PlanObjective::Kind kind = PlanObjective::ENSEMBLE) {
    PlanObjective o;
    o.kind = kind;
    o.s0 = s0;
    return o;
}
PlanObjective planet_objective(const float* latent0, const float* belief0) {
    PlanObjective o;
    o.kind = PlanObjective::PLANET;
    o.latent0 = latent0;
    o.belief0 = belief0;
    return o;
}

// The front checks every fused plan shares: the objective's model, the driver's own pointers (`args`) and the start state, act_dim
// against the model, n_env, and a PlaNet objective's particles
int check_plan(const hipets_engine* e, const PlanObjective& obj, bool args, int A, int n_env, int P) {
    const bool planet = obj.is_planet();
    if (planet && !(e && e->has_planet)) return fail("engine has no PlaNet model (call hipets_planet_set_model)");
    if (!planet && !(e && e->has_model)) return fail("engine has no model (call hipets_set_model)");
    if (!args || (planet ? !(obj.latent0 && obj.belief0) : !obj.s0)) return fail("null argument");
    if (planet && A != e->pd.action) return fail("act_dim %d != model action_size %d", A, e->pd.action);
    if (!planet && A != e->md.act_dim) return fail("act_dim %d != model act_dim %d", A, e->md.act_dim);
    if (n_env < 1 || n_env > 4096) return fail("n_env %d outside [1, 4096]", n_env);
    if (planet && P < 1) return fail("bad pop/horizon/particles");
    return check_reduce(e, P);  // (a sharded plan: on every rank alike, before the first collective)
}

// CEM refit (cem.hpp): one row of workgroups per environment; the elite selection sorts the next power of two >= c.pop values in LDS
int launch_cem_refit(const CemDev& c, float* values, const float* population, float* mu, float* disp, float* best_value, float* best_solution,
                     int* elite_idx, hipStream_t st) {
    int n2 = 1;
    while (n2 < c.pop) n2 <<= 1;
    hipLaunchKernelGGL(cem_refit_kernel, dim3(refit_blocks(c.D), c.n_env), dim3(kRefitThreads), (size_t)n2 * 8 + kRefitScratchBytes, st, c, values,
                       population, mu, disp, best_value, best_solution, elite_idx);
    HCHECK(hipGetLastError());
    return 0;
}

// What the three fused plans share.  Iteration i owns the random streams sid = (first_stream + i) * stream_stride, sid + 1, ...: sample(i, sid)
// draws the candidates from them, the objective rolls rows(i) candidates of `population` out on stream sid + rollout_stream into `returns`
// (nullptr: the per-row totals stay in e->totals for the refit), refit(i) updates the distribution.  prologue(rollout seed) runs once.
// A local plan stops at its first failure.  A rank of a sharded plan carries on to the end instead -- skipping its own work, joining every
// collective, because its peers wait there (engine.hpp LocalErr) -- and reports the failure afterwards.
struct PlanLoop {
    int n_env, H, P, iters;
    uint64_t first_stream, stream_stride, rollout_stream;
    const float* population;
    float* returns;
};
template <class Prologue, class Rows, class Sample, class Refit>
int run_plan(hipets_engine* e, const PlanObjective& obj, const PlanLoop& pl, uint64_t seed, void* stream, Prologue prologue, Rows rows, Sample sample,
             Refit refit) {
    hipets_rollout_opts ro{};
    ro.mode = e->plan_mode;
    ro.seed = obj.rollout_seed(e, seed);
    ro.n_env = pl.n_env;
    const bool carry_on = obj.is_sharded();
    LocalErr le;
    le.note(prologue(ro.seed));
    for (int i = 0; i < pl.iters && (carry_on || le.ok()); ++i) {
        const uint64_t sid = (pl.first_stream + (uint64_t)i) * pl.stream_stride;
        if (le.ok()) le.note(sample(i, sid));
        ro.stream_id = sid + pl.rollout_stream;
        if (obj.evaluate(e, pl.population, rows(i), pl.H, pl.P, &ro, pl.returns, stream, le)) return 1;  // a collective failed: over for everybody
        if (le.ok()) le.note(refit(i));
    }
    return le.report();
}

int plan_cem_impl(hipets_engine* e, const hipets_cem_params* p, int32_t n_env, const float* x0, const float* lower, const float* upper,
                  const PlanObjective& obj, int32_t P, uint64_t seed, uint64_t plan_id, float* out, void* stream) {
    if (check_cem(p) || check_plan(e, obj, x0 && lower && upper && out, p->act_dim, n_env, P)) return 1;
    if (obj.is_sharded() && check_shards(e, p->population_size, P)) return 1;  // identical on every rank, before any collective
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const CemDev c = make_cem(p, n_env);
    const size_t nd = (size_t)n_env * c.D, npop = (size_t)n_env * c.pop;
    if (e->mu.ensure(nd * 4) || e->disp.ensure(nd * 4) || e->best_solution.ensure(nd * 4) || e->best_value.ensure((size_t)n_env * 4 + 16) ||
        e->population.ensure(npop * c.D * 4) || e->values.ensure(npop * 4) || obj.reserve_shards(e, c.pop))
        return 1;
    const int iters = p->num_iterations;
    const PlanLoop pl{n_env, c.H, P, iters, plan_id * (uint64_t)iters, 1, 0, e->population.as<float>(), nullptr};
    auto prologue = [&](uint64_t rollout_seed) -> int {
        if (obj.clear_padding(e, c.pop, st)) return 1;
        hipLaunchKernelGGL(cem_init_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, c, x0, lower, upper, e->mu.as<float>(),
                           e->disp.as<float>(), e->best_value.as<float>());
        HCHECK(hipGetLastError());
        HCHECK(hipMemsetAsync(e->best_solution.p, 0, nd * 4, st));
        return obj.is_planet() ? 0 : plan_prologue(e, obj.s0, n_env, c.H, iters, rollout_seed, pl.first_stream, st);
    };
    auto sample = [&](int, uint64_t sid) -> int {  // identical on every rank of a sharded plan: same seed, same counters
        const long long n = (long long)npop * c.D;
        hipLaunchKernelGGL(cem_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c, e->mu.as<float>(), e->disp.as<float>(),
                           lower, upper, (const float*)nullptr, (unsigned long long)seed, (unsigned long long)sid, e->population.as<float>());
        HCHECK(hipGetLastError());
        return 0;
    };
    auto refit = [&](int i) -> int {
        int* eidx = (e->has_trace && e->trace.elite_idx) ? e->trace.elite_idx + (size_t)i * n_env * c.K : nullptr;
        CemDev cr = c;
        obj.refit_from_totals(e, &cr, P);  // (the particle mean of the returns, model_env.py:190-191: one launch less per iteration)
        if (launch_cem_refit(cr, e->values.as<float>(), e->population.as<float>(), e->mu.as<float>(), e->disp.as<float>(), e->best_value.as<float>(),
                             e->best_solution.as<float>(), eidx, st))
            return 1;
        return trace_iter(e, i, (int)npop, (size_t)c.D, e->population.as<float>(), e->values.as<float>(), e->mu.as<float>(), e->disp.as<float>(), st, n_env);
    };
    if (run_plan(e, obj, pl, seed, stream, prologue, [&](int) { return (int)npop; }, sample, refit)) return 1;
    HCHECK(hipMemcpyAsync(out, p->return_mean_elites ? e->mu.p : e->best_solution.p, nd * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

int plan_mppi_impl(hipets_engine* e, int32_t pop, int32_t H, int32_t A, int32_t num_iterations, double gamma, double beta, int32_t n_env,
                   float* mean, const float* lower, const float* upper, const PlanObjective& obj, int32_t P, uint64_t seed, uint64_t plan_id,
                   void* stream) {
    if (check_plan(e, obj, mean && lower && upper, A, n_env, P)) return 1;
    if (pop < 1 || pop > 12000) return fail("population_size %d outside [1, 12000]", pop);
    if (H < 1 || num_iterations < 0) return fail("bad horizon/num_iterations");
    if (obj.is_sharded() && check_shards(e, pop, P)) return 1;  // identical on every rank, before any collective
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const size_t nd = (size_t)H * A, npop = (size_t)n_env * pop;
    if (e->mu.ensure(n_env * nd * 4) || e->past_action.ensure((size_t)n_env * A * 4) || e->population.ensure(npop * nd * 4) ||
        e->values.ensure(npop * 4) || obj.reserve_shards(e, pop))
        return 1;
    const PlanLoop pl{n_env, H, P, num_iterations, plan_id * (uint64_t)num_iterations, 1, 0, e->population.as<float>(), e->values.as<float>()};
    auto prologue = [&](uint64_t rollout_seed) -> int {
        if (obj.clear_padding(e, pop, st)) return 1;
        HCHECK(hipMemcpyAsync(e->mu.p, mean, n_env * nd * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(mppi_shift_kernel, dim3((unsigned)((n_env * nd + 255) / 256)), dim3(256), 0, st, n_env, H, A, e->mu.as<float>(), mean,
                           e->past_action.as<float>());
        HCHECK(hipGetLastError());
        return obj.is_planet() ? 0 : plan_prologue(e, obj.s0, n_env, H, num_iterations, rollout_seed, pl.first_stream, st);
    };
    auto sample = [&](int, uint64_t sid) -> int {
        return launch_mppi_sample(n_env, pop, H, A, (float)beta, mean, e->past_action.as<float>(), lower, upper, nullptr, seed, sid,
                                  e->population.as<float>(), st);  // sharded: identical on every rank (same seed, same counters)
    };
    auto update = [&](int k) -> int {
        if (launch_mppi_update(e, n_env, pop, (int)nd, (float)gamma, e->values.as<float>(), e->population.as<float>(), mean, st)) return 1;
        return trace_iter(e, k, (int)npop, nd, e->population.as<float>(), e->values.as<float>(), mean, nullptr, st, n_env);
    };
    return run_plan(e, obj, pl, seed, stream, prologue, [&](int) { return (int)npop; }, sample, update);
}

int plan_icem_impl(hipets_engine* e, const hipets_icem_params* p, int32_t n_env, const float* x0, const float* lower, const float* upper,
                   float* elite, int32_t has_elite, const int32_t* keep_idx, const PlanObjective& obj, int32_t P, uint64_t seed, uint64_t plan_id,
                   float* out, void* stream) {
    if (check_plan(e, obj, p && x0 && lower && upper && elite && out, p ? p->act_dim : 0, n_env, P)) return 1;
    if (p->horizon < 2 || p->horizon > kMaxHorizon) return fail("iCEM horizon %d outside [2, %d]", p->horizon, kMaxHorizon);
    const int K = p->elite_num, keep = p->keep_elite_size, iters = p->num_iterations, H = p->horizon, A = p->act_dim;
    if (K < 1 || keep < 0 || keep > K) return fail("elite_num %d / keep_elite_size %d invalid", K, keep);
    if (p->population_size < 1 || iters < 0 || !(p->population_decay_factor > 0.0)) return fail("bad iCEM parameters");
    // population sizes (:419-431) and the rows every iteration evaluates are known up front: size the workspace for the largest, and
    // (sharded) refuse on EVERY rank, before the first collective, what one rank's shard of some iteration could not take
    std::vector<int> sizes(iters), rows_of(iters);
    int max_rows = 1;
    for (int i = 0, he = has_elite; i < iters; ++i, he = 1) {
        int n = (int)std::ceil(std::fmax((double)p->population_size * std::pow(p->population_decay_factor, -(double)i), 2.0 * K));
        const int m = p->population_size_module;
        if (m > 0 && n % m) n += m - n % m;
        sizes[i] = n;
        if (n + keep > kMaxPop) return fail("iCEM iteration %d evaluates %d candidates (max %d)", i, n + keep, kMaxPop);
        rows_of[i] = n + (he ? ((i == iters - 1 && i != 0) ? 1 : keep) : 0);
        if (K > rows_of[i]) return fail("elite_num %d invalid", K);
        max_rows = std::max(max_rows, n + keep);
        if (obj.is_sharded() && check_shards(e, rows_of[i], P)) return 1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HCHECK(hipSetDevice(e->device));
    ENTER_STREAM(e, st);
    const size_t nd = (size_t)H * A, ne = (size_t)n_env;
    if (e->mu.ensure(ne * nd * 4) || e->disp.ensure(ne * nd * 4) || e->best_solution.ensure(ne * nd * 4) || e->best_value.ensure(ne * 4 + 16) ||
        e->population.ensure(ne * max_rows * nd * 4) || e->values.ensure(ne * max_rows * 4) ||
        e->kept.ensure(ne * std::max(keep, 1) * nd * 4) || e->elite_idx.ensure(ne * K * 4) || e->keep_idx.ensure(ne * std::max(keep, 1) * 4) ||
        (!obj.is_planet() && e->s0.ensure(ne * e->md.obs_dim * 4)) || obj.reserve_shards(e, max_rows))
        return 1;
    hipets_cem_params cp{};
    cp.population_size = std::max(K, 1);
    cp.horizon = H;
    cp.act_dim = A;
    cp.num_iterations = iters;
    cp.elite_num = K;
    cp.alpha = p->alpha;
    cp.return_mean_elites = p->return_mean_elites;
    cp.clipped_normal = 0;  // initial variance ((ub - lb)^2) / 16 (:373) and variance (not std) refit
    cp.unbiased_var = 0;    // :479
    float* popbuf = e->population.as<float>();  // [n_env][rows][H][A], rows = this iteration's candidates per environment
    // (the rollout reads the s0 staged by the prologue and leaves its totals to the refit: CemDev::totals)
    const PlanLoop pl{n_env, H, P, iters, plan_id * (uint64_t)iters, 4, 3, popbuf, nullptr};
    auto prologue = [&](uint64_t) -> int {
        if (obj.clear_padding(e, max_rows, st)) return 1;
        hipLaunchKernelGGL(cem_init_kernel, dim3((unsigned)((ne * nd + 255) / 256)), dim3(256), 0, st, make_cem(&cp, n_env), x0, lower, upper,
                           e->mu.as<float>(), e->disp.as<float>(), e->best_value.as<float>());
        HCHECK(hipGetLastError());
        HCHECK(hipMemsetAsync(e->best_solution.p, 0, ne * nd * 4, st));
        // the observations are the same for every iteration: staged once (a PlaNet objective reads its DEVICE start states in place)
        return obj.is_planet() ? 0 : stage_h2d(e, e->s0.p, obj.s0, ne * e->md.obs_dim * 4, st);
    };
    auto sample = [&](int i, uint64_t sid) -> int {  // identical on every rank of a sharded plan: same seed, same counters
        const int n = sizes[i], rows = rows_of[i], extra = rows - n;
        launch_icem_sample(st, n_env, rows, n, H, A, (float)p->colored_noise_exponent, e->mu.as<float>(), e->disp.as<float>(), lower, upper,
                           (const float*)nullptr, (unsigned long long)seed, (unsigned long long)sid, popbuf);
        HCHECK(hipGetLastError());
        if (!extra) return 0;
        float* tail = popbuf + (size_t)n * nd;  // environment 0's extra rows; the others follow rows * nd floats apart
        if (i == iters - 1 && i != 0) {  // :463-464
            hipLaunchKernelGGL(icem_append_mu_kernel, dim3((unsigned)((ne * nd + 255) / 256)), dim3(256), 0, st, n_env, rows, n, (int)nd,
                               e->mu.as<float>(), popbuf);
            HCHECK(hipGetLastError());
            return 0;
        }
        const int32_t* kidx = keep_idx ? keep_idx + (size_t)i * n_env * keep : e->keep_idx.as<int32_t>();
        if (!keep_idx) {
            hipLaunchKernelGGL(icem_keep_select_kernel, dim3(n_env), dim3(256), (size_t)K * 8, st, K, keep, (unsigned long long)seed,
                               (unsigned long long)(sid + 2), e->keep_idx.as<int32_t>());
            HCHECK(hipGetLastError());
        }
        const long long ng = (long long)keep * nd;
        if (i == 0) {  // :450-462: kept elites shifted one step with a fresh tail action
            hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((ng + 255) / 256), n_env), dim3(256), 0, st, keep, (int)nd, elite, kidx,
                               e->kept.as<float>(), (long long)K * nd, (long long)keep * nd);
            HCHECK(hipGetLastError());
            hipLaunchKernelGGL(icem_shift_kernel, dim3((unsigned)((ne * ng + 255) / 256)), dim3(256), 0, st, n_env, rows, keep, H, A,
                               e->kept.as<float>(), e->mu.as<float>(), e->disp.as<float>(), (const float*)nullptr,
                               (unsigned long long)seed, (unsigned long long)(sid + 1), tail);
            HCHECK(hipGetLastError());
        } else {  // :465-466
            hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((ng + 255) / 256), n_env), dim3(256), 0, st, keep, (int)nd, elite, kidx,
                               tail, (long long)K * nd, (long long)rows * nd);
            HCHECK(hipGetLastError());
        }
        return 0;
    };
    auto refit = [&](int i) -> int {
        const int rows = rows_of[i];
        cp.population_size = rows;
        if (check_cem(&cp)) return 1;
        CemDev cr = make_cem(&cp, n_env);
        obj.refit_from_totals(e, &cr, P);
        if (launch_cem_refit(cr, e->values.as<float>(), popbuf, e->mu.as<float>(), e->disp.as<float>(), e->best_value.as<float>(),
                             e->best_solution.as<float>(), e->elite_idx.as<int>(), st))
            return 1;
        const long long nk = (long long)K * nd;  // self.elite = population[elite_idx] (:476), per environment
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((nk + 255) / 256), n_env), dim3(256), 0, st, K, (int)nd, popbuf, e->elite_idx.as<int32_t>(),
                           elite, (long long)rows * nd, (long long)K * nd);
        HCHECK(hipGetLastError());
        if (trace_iter(e, i, n_env * rows, nd, popbuf, e->values.as<float>(), e->mu.as<float>(), e->disp.as<float>(), st, n_env)) return 1;
        if (e->has_trace && e->trace.elite_idx)
            HCHECK(hipMemcpyAsync(e->trace.elite_idx + (size_t)i * n_env * K, e->elite_idx.p, ne * K * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    if (run_plan(e, obj, pl, seed, stream, prologue, [&](int i) { return n_env * rows_of[i]; }, sample, refit)) return 1;
    HCHECK(hipMemcpyAsync(out, p->return_mean_elites ? e->mu.p : e->best_solution.p, ne * nd * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

}  // namespace

extern "C" {

int hipets_cem_sample(hipets_engine* e, const hipets_cem_params* p, const float* mu, const float* dispersion,
                      const float* lower, const float* upper, const float* z, uint64_t seed, uint64_t stream_id,
                      float* population, void* stream) {
    if (!e) return fail("null engine");
    if (check_cem(p)) return 1;
    if (!mu || !dispersion || !lower || !upper || !population) return fail("null argument");
    HCHECK(hipSetDevice(e->device));
    const CemDev c = make_cem(p);
    const long long n = (long long)c.pop * c.D;
    hipLaunchKernelGGL(cem_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), c,
                       mu, dispersion, lower, upper, z, (unsigned long long)seed, (unsigned long long)stream_id, population);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_cem_refit(hipets_engine* e, const hipets_cem_params* p, float* values, const float* population, float* mu,
                     float* dispersion, float* best_value, float* best_solution, int32_t* elite_idx, void* stream) {
    if (!e) return fail("null engine");
    if (check_cem(p)) return 1;
    if (!values || !population || !mu || !dispersion || !best_value || !best_solution) return fail("null argument");
    HCHECK(hipSetDevice(e->device));
    return launch_cem_refit(make_cem(p), values, population, mu, dispersion, best_value, best_solution, elite_idx, reinterpret_cast<hipStream_t>(stream));
}

int hipets_cem_refit_elites(hipets_engine* e, const hipets_cem_params* p, float* values, const float* population, const int32_t* elites,
                            float* mu, float* dispersion, float* best_value, float* best_solution, void* stream) {
    if (!e) return fail("null engine");
    if (check_cem(p)) return 1;
    if (!values || !population || !elites || !mu || !dispersion || !best_value || !best_solution) return fail("null argument");
    HCHECK(hipSetDevice(e->device));
    CemDev c = make_cem(p);
    c.elite_in = elites;
    return launch_cem_refit(c, values, population, mu, dispersion, best_value, best_solution, nullptr, reinterpret_cast<hipStream_t>(stream));
}

int hipets_gather_rows(hipets_engine* e, int32_t rows, int32_t dim, const float* src, const int32_t* index, float* dst,
                       void* stream) {
    if (!e || !src || !index || !dst || rows < 1 || dim < 1) return fail("bad argument");
    HCHECK(hipSetDevice(e->device));
    const long long n = (long long)rows * dim;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), rows,
                       dim, src, index, dst, 0ll, 0ll);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_mppi_sample(hipets_engine* e, int32_t pop, int32_t H, int32_t A, double beta, const float* mean, const float* past_action,
                       const float* lower, const float* upper, const float* z, uint64_t seed, uint64_t stream_id,
                       float* population, void* stream) {
    if (!e || !mean || !past_action || !lower || !upper || !population) return fail("null argument");
    if (pop < 1 || H < 1 || A < 1) return fail("bad pop/horizon/act_dim");
    HCHECK(hipSetDevice(e->device));
    return launch_mppi_sample(1, pop, H, A, (float)beta, mean, past_action, lower, upper, z, seed, stream_id, population, reinterpret_cast<hipStream_t>(stream));
}

int hipets_mppi_update(hipets_engine* e, int32_t pop, int32_t H, int32_t A, double gamma, float* values, const float* population,
                       float* mean, void* stream) {
    if (!e || !values || !population || !mean) return fail("null argument");
    if (pop < 1 || pop > 12000 || H < 1 || A < 1) return fail("population_size %d outside [1, 12000]", pop);
    HCHECK(hipSetDevice(e->device));
    return launch_mppi_update(e, 1, pop, H * A, (float)gamma, values, population, mean, reinterpret_cast<hipStream_t>(stream));
}

int hipets_icem_sample(hipets_engine* e, int32_t n, int32_t H, int32_t A, double exponent, const float* mu, const float* var,
                       const float* lower, const float* upper, const float* normals, uint64_t seed, uint64_t stream_id,
                       float* population, void* stream) {
    if (!e || !mu || !var || !lower || !upper || !population) return fail("null argument");
    if (n < 1 || A < 1) return fail("bad n/act_dim");
    if (H < 2 || H > kMaxHorizon) return fail("iCEM horizon %d outside [2, %d]", H, kMaxHorizon);
    HCHECK(hipSetDevice(e->device));
    launch_icem_sample(reinterpret_cast<hipStream_t>(stream), 1, n, n, H, A, (float)exponent, mu, var, lower, upper, normals, (unsigned long long)seed,
                       (unsigned long long)stream_id, population);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_icem_shift(hipets_engine* e, int32_t keep, int32_t H, int32_t A, const float* kept, const float* mu, const float* var,
                      const float* end_noise, uint64_t seed, uint64_t stream_id, float* out, void* stream) {
    if (!e || !kept || !mu || !var || !out) return fail("null argument");
    if (keep < 1 || H < 1 || A < 1) return fail("bad keep/horizon/act_dim");
    HCHECK(hipSetDevice(e->device));
    const int n = keep * H * A;
    hipLaunchKernelGGL(icem_shift_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), 1, keep, keep, H, A, kept,
                       mu, var, end_noise, (unsigned long long)seed, (unsigned long long)stream_id, out);
    HCHECK(hipGetLastError());
    return 0;
}

int hipets_plan_cem(hipets_engine* e, const hipets_cem_params* p, const float* x0, const float* lower, const float* upper,
                    const float* s0, int32_t P, uint64_t seed, uint64_t plan_id, float* out, void* stream) {
    return hipets_plan_cem_batched(e, p, 1, x0, lower, upper, s0, P, seed, plan_id, out, stream);
}

int hipets_plan_cem_batched(hipets_engine* e, const hipets_cem_params* p, int32_t n_env, const float* x0, const float* lower,
                            const float* upper, const float* s0, int32_t P, uint64_t seed, uint64_t plan_id, float* out,
                            void* stream) {
    return plan_cem_impl(e, p, n_env, x0, lower, upper, ensemble_objective(s0), P, seed, plan_id, out, stream);
}

int hipets_plan_cem_sharded(hipets_engine* e, const hipets_cem_params* p, const float* x0, const float* lower, const float* upper,
                            const float* s0, int32_t P, uint64_t seed, uint64_t plan_id, float* out, void* stream) {
    if (e && !e->comm) return fail("no communicator (call hipets_comm_init)");
    return plan_cem_impl(e, p, 1, x0, lower, upper, ensemble_objective(s0, PlanObjective::SHARDED), P, seed, plan_id, out, stream);
}

int hipets_plan_mppi(hipets_engine* e, int32_t pop, int32_t H, int32_t A, int32_t num_iterations, double gamma, double beta,
                     float* mean, const float* lower, const float* upper, const float* s0, int32_t P, uint64_t seed,
                     uint64_t plan_id, void* stream) {
    return hipets_plan_mppi_batched(e, pop, H, A, num_iterations, gamma, beta, 1, mean, lower, upper, s0, P, seed, plan_id, stream);
}

int hipets_plan_mppi_batched(hipets_engine* e, int32_t pop, int32_t H, int32_t A, int32_t num_iterations, double gamma, double beta,
                             int32_t n_env, float* mean, const float* lower, const float* upper, const float* s0, int32_t P,
                             uint64_t seed, uint64_t plan_id, void* stream) {
    return plan_mppi_impl(e, pop, H, A, num_iterations, gamma, beta, n_env, mean, lower, upper, ensemble_objective(s0), P, seed, plan_id, stream);
}

int hipets_plan_mppi_sharded(hipets_engine* e, int32_t pop, int32_t H, int32_t A, int32_t num_iterations, double gamma, double beta,
                             float* mean, const float* lower, const float* upper, const float* s0, int32_t P, uint64_t seed,
                             uint64_t plan_id, void* stream) {
    if (e && !e->comm) return fail("no communicator (call hipets_comm_init)");
    return plan_mppi_impl(e, pop, H, A, num_iterations, gamma, beta, 1, mean, lower, upper, ensemble_objective(s0, PlanObjective::SHARDED), P, seed, plan_id, stream);
}

int hipets_plan_icem(hipets_engine* e, const hipets_icem_params* p, const float* x0, const float* lower, const float* upper,
                     float* elite, int32_t has_elite, const int32_t* keep_idx, const float* s0, int32_t P, uint64_t seed,
                     uint64_t plan_id, float* out, void* stream) {
    return hipets_plan_icem_batched(e, p, 1, x0, lower, upper, elite, has_elite, keep_idx, s0, P, seed, plan_id, out, stream);
}

int hipets_plan_icem_batched(hipets_engine* e, const hipets_icem_params* p, int32_t n_env, const float* x0, const float* lower,
                             const float* upper, float* elite, int32_t has_elite, const int32_t* keep_idx, const float* s0, int32_t P,
                             uint64_t seed, uint64_t plan_id, float* out, void* stream) {
    return plan_icem_impl(e, p, n_env, x0, lower, upper, elite, has_elite, keep_idx, ensemble_objective(s0), P, seed, plan_id, out, stream);
}

int hipets_plan_icem_sharded(hipets_engine* e, const hipets_icem_params* p, const float* x0, const float* lower, const float* upper,
                             float* elite, int32_t has_elite, const int32_t* keep_idx, const float* s0, int32_t P, uint64_t seed,
                             uint64_t plan_id, float* out, void* stream) {
    if (e && !e->comm) return fail("no communicator (call hipets_comm_init)");
    return plan_icem_impl(e, p, 1, x0, lower, upper, elite, has_elite, keep_idx, ensemble_objective(s0, PlanObjective::SHARDED), P, seed, plan_id, out, stream);
}

int hipets_plan_planet_cem(hipets_engine* e, const hipets_cem_params* p, const float* x0, const float* lower, const float* upper,
                           const float* latent0, const float* belief0, int32_t P, uint64_t seed, uint64_t plan_id, float* out,
                           void* stream) {
    return plan_cem_impl(e, p, 1, x0, lower, upper, planet_objective(latent0, belief0), P, seed, plan_id, out, stream);
}

// Batched PlaNet plans: the ensemble's batched drivers with the PlaNet objective (trajectory_opt.py:142-188, 238-311, 391-487 per
// environment over planet.py:531-581); never sharded, so an engine's communicator stays out of them
int hipets_plan_planet_cem_batched(hipets_engine* e, const hipets_cem_params* p, int32_t n_env, const float* x0, const float* lower,
                                   const float* upper, const float* latent0, const float* belief0, int32_t P, uint64_t seed,
                                   uint64_t plan_id, float* out, void* stream) {
    return plan_cem_impl(e, p, n_env, x0, lower, upper, planet_objective(latent0, belief0), P, seed, plan_id, out, stream);
}

int hipets_plan_planet_mppi_batched(hipets_engine* e, int32_t pop, int32_t H, int32_t A, int32_t num_iterations, double gamma, double beta,
                                    int32_t n_env, float* mean, const float* lower, const float* upper, const float* latent0,
                                    const float* belief0, int32_t P, uint64_t seed, uint64_t plan_id, void* stream) {
    return plan_mppi_impl(e, pop, H, A, num_iterations, gamma, beta, n_env, mean, lower, upper, planet_objective(latent0, belief0), P, seed,
                          plan_id, stream);
}

int hipets_plan_planet_icem_batched(hipets_engine* e, const hipets_icem_params* p, int32_t n_env, const float* x0, const float* lower,
                                    const float* upper, float* elite, int32_t has_elite, const int32_t* keep_idx, const float* latent0,
                                    const float* belief0, int32_t P, uint64_t seed, uint64_t plan_id, float* out, void* stream) {
    return plan_icem_impl(e, p, n_env, x0, lower, upper, elite, has_elite, keep_idx, planet_objective(latent0, belief0), P, seed, plan_id,
                          out, stream);
}

}  // extern "C"
