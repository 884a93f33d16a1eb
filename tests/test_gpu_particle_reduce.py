"""Risk-aware particle reductions on the GPU (include/hipets.h, hipets_set_particle_reduce), bit for bit against the numpy float32
restatement of the rule (tests/particle_reduce_restatement.py), NaN equal to NaN:

A  the rule alone: Engine.particle_reduce (particle_mean_kernel) over the eight-wide fetch's edges, the 256-thread block's edge, the
   largest rank count, and totals with ties, equal values, NaN and infinities
B  hipets_trajectory_returns on both forms (P <= 256 through LDS, P = 300 in two passes): returns == the restatement of its own row totals
C  rollouts of a tiny ensemble (DEVICE, FAST) and a tiny PlaNet model: returns == the restatement of the rollout's own row totals
D  fused CEM / iCEM / MPPI plans == their per-iteration paths (particle_mean_kernel against the refit prologue); batched plans
E  a shared engine does not leak one objective's reduction into the next; every invalid argument is refused as one"""
import numpy as np
import pytest
import torch

import hipets
from conftest import to_spec
from hipets import HipetsError, ParticleReduce, _lib
from hipets.planning import _BoundObjective
from oracle import pets_oracle as po
from oracle import planet_oracle as pl
from particle_reduce_restatement import edge_totals, particle_reduce, same_bits
from test_gpu_planet import to_planet_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = ParticleReduce


@pytest.fixture(autouse=True)
def back_to_the_mean(engine):
    """The session's engine is shared with every other test file: each test here leaves it at the mean."""
    yield
    engine.set_particle_reduce(R.mean())


def reductions(P):
    """(ParticleReduce, the restatement's arguments) of every kind for P particles; WORST_K (k = 1, the middle, P) up to 256 particles"""
    out = [(R.mean(), dict(kind="mean")), (R.mean_std(1.25), dict(kind="mean_std", kappa=1.25)), (R.mean_std(-0.5), dict(kind="mean_std", kappa=-0.5)),
           (R.worst_case(), dict(kind="min")), (R.best_case(), dict(kind="max"))]
    if P <= 256:
        out += [(R.worst_k(k), dict(kind="worst_k", k=k)) for k in sorted({1, (P + 1) // 2, P})]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# A  the rule alone
# ---------------------------------------------------------------------------------------------------------------------------
RULE_SHAPES = [(1, 1), (3, 2), (5, 7), (4, 8), (4, 9), (257, 20), (2, 256), (2, 300)]


@pytest.mark.parametrize("pop,P", RULE_SHAPES, ids=[f"pop{a}_P{b}" for a, b in RULE_SHAPES])
def test_particle_reduce_equals_the_restatement_bit_for_bit(engine, pop, P):
    for first in range(6 if pop < 6 else 1):  # (fewer than six candidates: every kind of totals reaches every candidate in turn)
        tot = edge_totals(pop, P, first)
        dev = torch.from_numpy(tot).to(DEV)
        for r, kw in reductions(P):
            engine.set_particle_reduce(r)
            got = engine.particle_reduce(dev, pop, P).cpu().numpy()
            assert same_bits(got, particle_reduce(tot, pop, P, **kw)), (first, r)


# ---------------------------------------------------------------------------------------------------------------------------
# B  hipets_trajectory_returns
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop,P", [(5, 7), (37, 7), (3, 300)], ids=["lds", "lds_two_blocks", "two_pass"])
def test_trajectory_returns_reduces_its_own_row_totals(engine, pop, P):
    H, B = 3, pop * P
    rng = np.random.default_rng(pop + P)
    rewards = (rng.standard_normal((H, B)) * 10).astype(np.float32)
    rewards[1, 2] = np.nan  # (row 2 of candidate 0 carries a NaN unless it terminated at step 0)
    dones = (rng.random((H, B)) < 0.3).astype(np.uint8)
    r, d = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
    base = None
    for red, kw in reductions(P):
        engine.set_particle_reduce(red)
        ret, tot, _ = engine.trajectory_returns(r, d, pop, P, row_totals=True)
        tot = tot.cpu().numpy()
        assert same_bits(ret.cpu().numpy(), particle_reduce(tot, pop, P, **kw)), red
        assert same_bits(engine.trajectory_returns(r, d, pop, P).cpu().numpy(), ret.cpu().numpy())  # (two passes: on the engine's own totals)
        base = tot if base is None else base
        assert same_bits(tot, base)  # the row totals do not depend on the reduction
    assert dones[:, : B // 2].any() and not dones.all()


# ---------------------------------------------------------------------------------------------------------------------------
# C  rollouts
# ---------------------------------------------------------------------------------------------------------------------------
OBS, ACT, MEMBERS, HID, POP, P, H = 5, 2, 3, 32, 6, 6, 4


def tiny_spec(seed=0):
    """obs 5, act 2, 3 members, hid 32; a learned reward and a termination that fires for some rows"""
    om = po.make_synthetic_model(OBS, ACT, ensemble_size=MEMBERS, hid=HID, seed=seed, learned_rewards=True, reward=None, termination="inverted_pendulum")
    return to_spec(om, OBS, ACT)


def tiny_actions(pop=POP, horizon=H, seed=0):
    return (torch.rand(pop, horizon, ACT, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


S0 = (np.random.default_rng(3).standard_normal(OBS) * 0.1).astype(np.float32)


@pytest.mark.parametrize("mode", ["device", "fast"])
def test_ensemble_rollouts_reduce_their_own_row_totals(engine, mode):
    spec, a = tiny_spec(), tiny_actions()
    base = None
    for red, kw in reductions(P):
        fn = hipets.make_eval_fn(spec, P, engine=engine, mode=mode, seed=11, particle_reduce=red)
        tr = fn.trajectories(S0, a)
        tot, ret = tr["row_totals"].cpu().numpy(), tr["returns"].clone()
        assert same_bits(ret.cpu().numpy(), particle_reduce(tot, POP, P, **kw)), red
        assert same_bits(fn.evaluate_seeded(S0, a, fn.seed, fn.calls).cpu().numpy(), ret.cpu().numpy())  # a plain call on the same stream
        base = (tot, tr["dones"].clone()) if base is None else base
        assert same_bits(tot, base[0])  # every objective ran stream 1 of seed 11: the same rows
    tot = base[0].reshape(POP, P)
    assert np.isfinite(tot).all() and (tot.max(1) > tot.min(1)).all()  # the particles of a candidate do spread
    assert base[1].any() and not base[1].all()  # some rows terminate


def test_planet_rollouts_reduce_their_own_row_totals(engine):
    L, A, Hb, F = 7, 2, 22, 19
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=5)
    spec = to_planet_spec(pm)
    g = torch.Generator().manual_seed(2)
    latent0, belief0 = torch.randn(1, L, generator=g) * 0.3, torch.randn(1, Hb, generator=g) * 0.3
    a = (torch.rand(POP, H, A, generator=g) * 2 - 1).to(DEV)
    base = None
    for red, kw in reductions(P):
        fn = hipets.make_eval_fn(spec, P, engine=engine, seed=4, particle_reduce=red)
        assert isinstance(fn, hipets.PlaNetTrajectoryEvalFn)
        fn.set_state(latent0, belief0)
        ret = fn(None, a).clone()  # stream 1 of seed 4
        rew = torch.zeros(H, POP * P, device=DEV)
        traced = engine.planet_rollout(a, latent0.to(DEV).reshape(-1), belief0.to(DEV).reshape(-1), P, seed=4, stream_id=1, trace_rewards=rew)
        assert same_bits(traced.cpu().numpy(), ret.cpu().numpy())
        steps = rew.cpu().numpy()
        tot = np.zeros(POP * P, np.float32)
        for t in range(H):  # planet.hpp: tot += r, step after step
            tot = (tot + steps[t]).astype(np.float32)
        assert same_bits(ret.cpu().numpy(), particle_reduce(tot, POP, P, **kw)), red
        base = tot if base is None else base
        assert same_bits(tot, base)
    assert (base.reshape(POP, P).max(1) > base.reshape(POP, P).min(1)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# D  plans
# ---------------------------------------------------------------------------------------------------------------------------
RISK = [R.worst_k(2), R.mean_std(1.0)]
RISK_IDS = ["worst_k2", "mean_std1"]
PP = 3  # particles of the plan tests: with 3 members every population is a whole number of member shares


def plan_objective(engine, mode, red, seed=13):
    fn = hipets.make_eval_fn(tiny_spec(seed=2), PP, engine=engine, seed=seed, mode=mode, particle_reduce=red)
    return _BoundObjective(fn, S0)


def bounds(horizon):
    return [[-1.0] * ACT] * horizon, [[1.0] * ACT] * horizon


@pytest.mark.parametrize("red", RISK, ids=RISK_IDS)
@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("pop,horizon", [(120, 4), (1030, 2)], ids=["pop120", "pop1030"])
def test_fused_cem_plan_equals_per_iteration_path(engine, mode, red, pop, horizon):
    """The fused plan reduces in the refit kernel's prologue (pop 1030: more candidates than its 1024 threads), the per-iteration path
    in particle_mean_kernel: one rule, the same bits -- and not the mean's plan."""
    obj = plan_objective(engine, mode, red)
    lb, ub = bounds(horizon)
    mk = lambda: hipets.CEMOptimizer(3, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)  # noqa: E731
    a, b, x0 = mk(), mk(), torch.zeros(horizon, ACT)
    for _ in range(2):
        fused = a.optimize(obj, x0=x0)
        seen = []
        generic = b.optimize(obj, x0=x0, callback=lambda p_, v_, i_: seen.append(i_))
        assert torch.equal(fused, generic) and len(seen) == 3
        x0 = fused
    assert torch.isfinite(fused).all()
    x0 = torch.zeros(horizon, ACT)  # (fresh optimizers: the same streams under both reductions)
    assert not torch.equal(mk().optimize(plan_objective(engine, mode, R.mean()), x0=x0), mk().optimize(obj, x0=x0))


@pytest.mark.parametrize("red", RISK, ids=RISK_IDS)
@pytest.mark.parametrize("mode", ["device", "fast"])
def test_fused_mppi_plan_equals_per_iteration_path(engine, mode, red):
    obj = plan_objective(engine, mode, red)
    lb, ub = bounds(H)
    mk = lambda: hipets.MPPIOptimizer(3, 120, 0.9, 1.0, 0.9, lb, ub, DEV, seed=21)  # noqa: E731
    a, b = mk(), mk()
    for _ in range(2):
        fused = a.optimize(obj)
        generic = b.optimize(obj, force_generic=True)
        assert torch.equal(fused, generic) and torch.equal(a.mean, b.mean)
    assert torch.isfinite(fused).all() and fused.abs().max() > 0


@pytest.mark.parametrize("red", RISK, ids=RISK_IDS)
@pytest.mark.parametrize("mode", ["device", "fast"])
def test_fused_icem_plan_equals_per_iteration_path(engine, mode, red):
    obj = plan_objective(engine, mode, red)
    lb, ub = bounds(H)
    mk = lambda: hipets.ICEMOptimizer(3, 0.1, 150, 1.3, 2.0, lb, ub, 0.3, 0.1, DEV, return_mean_elites=True, population_size_module=5, seed=17)  # noqa: E731
    a, b = mk(), mk()
    K, keep = int(a.elite_num), int(a.keep_elite_size)
    g = torch.Generator().manual_seed(0)
    x0 = torch.zeros(H, ACT)
    for call in range(2):
        perms = [torch.randperm(K, generator=g) for _ in range(3)]
        keep_idx = torch.stack([p_[:keep] for p_ in perms]).to(torch.int32).to(DEV).contiguous()
        fused = a.optimize(obj, x0=x0, keep_idx=keep_idx)
        generic = b.optimize(obj, x0=x0, inject=[{"keep_perm": p_} for p_ in perms])
        assert torch.equal(fused, generic) and torch.equal(a.elite, b.elite), call
        x0 = fused.cpu()
    assert torch.isfinite(fused).all()


@pytest.mark.parametrize("red", RISK, ids=RISK_IDS)
def test_batched_plan_of_one_environment_equals_the_single_plan(engine, red):
    obj = plan_objective(engine, "device", red)
    lb, ub = [-1.0] * ACT, [1.0] * ACT
    single = hipets.CEMOptimizer(3, 0.1, 120, [lb] * H, [ub] * H, 0.1, DEV, return_mean_elites=True, seed=7)
    agent = hipets.BatchedCEMAgent(obj.eval_fn, 1, lb, ub, H, 3, 0.1, 120, 0.1, return_mean_elites=True, seed=7)
    x0 = torch.zeros(H, ACT)
    for _ in range(2):
        one = single.optimize(obj, x0=x0)
        got = torch.from_numpy(agent.plan(S0[None]))[0]
        assert torch.isfinite(got).all() and torch.equal(got, one.cpu())
        x0 = agent.previous_solution[0].cpu().clone()


@pytest.mark.parametrize("kind", ["cem", "icem"])
@pytest.mark.parametrize("mode", ["device", "fast"])
def test_batched_plans_under_the_means_other_names_equal_the_mean(engine, kind, mode):
    """n_env = 3: worst_k(P) and mean_std(0.0) run the new arms of the refit prologue behind the per-environment offset, and give the
    mean's bits (the totals are finite)."""
    n_env = 3
    lb, ub = [-1.0] * ACT, [1.0] * ACT
    s0 = (np.random.default_rng(1).standard_normal((n_env, OBS)) * 0.1).astype(np.float32)
    plans = []
    for red in (R.mean(), R.worst_k(PP), R.mean_std(0.0)):
        fn = plan_objective(engine, mode, red).eval_fn
        if kind == "cem":
            agent = hipets.BatchedCEMAgent(fn, n_env, lb, ub, H, 3, 0.1, 120, 0.1, return_mean_elites=True, seed=7)
        else:
            agent = hipets.BatchedICEMAgent(fn, n_env, lb, ub, H, num_iterations=3, elite_ratio=0.1, population_size=150, population_decay_factor=1.3,
                                            colored_noise_exponent=2.0, keep_elite_frac=0.3, alpha=0.1, return_mean_elites=True, population_size_module=5,
                                            seed=7)
        plans.append([agent.plan(s0).copy() for _ in range(2)])
        assert engine.reduce == red
    for other in plans[1:]:
        for x, y in zip(plans[0], other):
            assert np.isfinite(x).all() and np.array_equal(x, y)
    assert not np.array_equal(plans[0][0][0], plans[0][0][1])  # the environments differ


# ---------------------------------------------------------------------------------------------------------------------------
# E  no leak, invalid arguments
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_shared_engine_does_not_leak_the_reduction(engine):
    spec, a = tiny_spec(), tiny_actions()
    default = hipets.make_eval_fn(spec, P, engine=engine, seed=11)
    low = hipets.make_eval_fn(spec, P, engine=engine, seed=11, particle_reduce="min")
    named = hipets.make_eval_fn(spec, P, engine=engine, seed=11, particle_reduce="mean")
    first = default.evaluate_seeded(S0, a, 11, 5).clone()
    lowest = low.evaluate_seeded(S0, a, 11, 5).clone()
    third = default.evaluate_seeded(S0, a, 11, 5).clone()
    fourth = named.evaluate_seeded(S0, a, 11, 5).clone()
    assert torch.equal(first, third) and torch.equal(first, fourth)
    assert (lowest < first).all() and engine.reduce == R.mean()
    env = hipets.ModelEnv(spec, engine=engine, seed=11)
    assert torch.equal(env.evaluate_action_sequences(a, S0, P, particle_reduce=R.worst_case()), low(S0, a))  # both: stream 1 of seed 11
    assert torch.equal(env.evaluate_action_sequences(a, S0, P), default.evaluate_seeded(S0, a, 11, 2))


def refused(call):
    with pytest.raises(HipetsError) as caught:
        call()
    assert caught.value.kind == _lib.ERR_INVALID_ARGUMENT, str(caught.value)


def test_invalid_arguments_are_refused_as_such(engine):
    setter = lambda **kw: engine._query("hipets_set_particle_reduce", **kw)  # noqa: E731  (ParticleReduce refuses these itself)
    tot = torch.from_numpy(edge_totals(2, 4)).to(DEV)
    engine.set_particle_reduce(R.best_case())
    want = engine.particle_reduce(tot, 2, 4).clone()
    for bad in (dict(kind=5, kappa=0.0, worst_k=0), dict(kind=-1, kappa=0.0, worst_k=0), dict(kind=1, kappa=float("nan"), worst_k=0),
                dict(kind=1, kappa=float("inf"), worst_k=0), dict(kind=4, kappa=0.0, worst_k=0), dict(kind=4, kappa=0.0, worst_k=-2)):
        refused(lambda bad=bad: setter(**bad))
        assert torch.equal(engine.particle_reduce(tot, 2, 4), want)  # a refused setter changes nothing
    # worst_k > num_particles, at every call that knows P
    engine.set_model(tiny_spec())
    a = tiny_actions()
    engine.set_particle_reduce(R.worst_k(5))
    rew, done = torch.zeros(H, 8, device=DEV), torch.zeros(H, 8, dtype=torch.uint8, device=DEV)
    lower, upper = -torch.ones(H, ACT, device=DEV), torch.ones(H, ACT, device=DEV)
    cem = hipets.Engine.cem_params(30, H, ACT, 2, 3, 0.1)
    refused(lambda: engine.particle_reduce(tot, 2, 4))
    refused(lambda: engine.trajectory_returns(rew, done, 2, 4))
    refused(lambda: engine.rollout(a, S0, 3, mode="device"))
    refused(lambda: engine.plan_cem(cem, torch.zeros(H, ACT, device=DEV), lower, upper, S0, 3))
    refused(lambda: engine.plan_mppi(30, H, ACT, 2, 0.9, 0.9, torch.zeros(H, ACT, device=DEV), lower, upper, S0, 3))
    assert torch.isfinite(engine.rollout(a, S0, 6, mode="device")).all()  # 5 of 6 particles: accepted
    # more than 256 particles under WORST_K (every other kind takes them: test A)
    engine.set_particle_reduce(R.worst_k(2))
    wide = torch.zeros(2 * 300, device=DEV)
    refused(lambda: engine.particle_reduce(wide, 2, 300))
    refused(lambda: engine.trajectory_returns(torch.zeros(H, 600, device=DEV), torch.zeros(H, 600, dtype=torch.uint8, device=DEV), 2, 300))
    refused(lambda: engine.rollout(a, S0, 300, mode="device"))
    torch.cuda.synchronize()
