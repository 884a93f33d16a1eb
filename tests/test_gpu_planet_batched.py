"""Batched PlaNet planning: PlaNet rollouts and the fused CEM / MPPI / iCEM plans over n_env latent
start states (latent0[g], belief0[g]) in one launch per iteration.  Every environment's slice of a batched rollout is a
single-environment rollout from its own start state bit for bit; batched plans are replayed PER ENVIRONMENT through the oracle with
the plan's exported draws (eps keyed by the launch-global row), teacher-forced per iteration where the optimizer selects elites."""
import numpy as np
import pytest
import torch

import hipets
from hipets.planning import _BoundObjective
from oracle import pets_oracle as po
from oracle import planet_oracle as pl
from test_gpu_planet import close, engine_normals, to_planet_spec
from test_gpu_plans_full_size import check_values, elites_agree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONF = (30, 6, 200, 200)  # conf/dynamics_model/planet.yaml: latent, action, belief, hidden (the STATIC kernel instance)


def start_states(n_env, latent, belief, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n_env, latent, generator=g) * 0.3, torch.randn(n_env, belief, generator=g) * 0.3


def planet_replay(engine, pm, latent0, belief0, P, H, seed):
    """values of ALL environments' candidates for (population_all, stream): environment g's slice goes through the oracle from its
    own start state with that slice of the launch's in-kernel eps."""
    def f(population_all, stream):
        n_env = latent0.shape[0]
        rows_env = population_all.shape[0] // n_env
        eps = engine_normals(engine, H, population_all.shape[0] * P, pm.latent_size, seed, stream)
        out = []
        for g in range(n_env):
            sl = slice(g * rows_env * P, (g + 1) * rows_env * P)
            out.append(pl.planet_rollout(pm, population_all[g * rows_env:(g + 1) * rows_env], latent0[g:g + 1], belief0[g:g + 1], P,
                                         eps=eps[:, sl]))
        return torch.cat(out)

    return f


# conf shape: 400 rows per environment (whole tiles); (7, 2, 22, 19): 74 rows per environment, so tiles straddle environments
@pytest.mark.parametrize("dims,pop_env,P,H", [(CONF, 200, 2, 12), ((7, 2, 22, 19), 37, 2, 5)], ids=["conf", "straddle"])
@pytest.mark.parametrize("n_env", [1, 3])
def test_batched_planet_rollout_injected_eps(engine, monkeypatch, dims, pop_env, P, H, n_env):
    L, A, Hb, F = dims
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=L + pop_env)
    engine.planet_set_model(to_planet_spec(pm))
    latent0, belief0 = start_states(n_env, L, Hb, seed=n_env)
    g = torch.Generator().manual_seed(7)
    pop = n_env * pop_env
    B, rows_env = pop * P, pop_env * P
    actions = (torch.rand(pop, H, A, generator=g) * 2 - 1).to(DEV)
    eps = torch.randn(H, B, L, generator=g).to(DEV)
    lat_d, bel_d = latent0.to(DEV), belief0.to(DEV)

    def batched():
        tl, tb, tr = torch.zeros(H, B, L, device=DEV), torch.zeros(H, B, Hb, device=DEV), torch.zeros(H, B, device=DEV)
        out = engine.planet_rollout(actions, lat_d, bel_d, P, eps=eps, trace_latent=tl, trace_belief=tb, trace_rewards=tr, n_env=n_env)
        return out.clone(), tl, tb, tr

    # conf runs the STATIC instance, so the comparison with the generic one at the end is between two kernels
    assert engine.planet_kernel_class() == ("static" if dims == CONF else "generic")
    static = batched()
    assert torch.isfinite(static[0]).all()
    for e_ in range(n_env):
        cs, rs = slice(e_ * pop_env, (e_ + 1) * pop_env), slice(e_ * rows_env, (e_ + 1) * rows_env)
        tl, tb, tr = torch.zeros(H, rows_env, L, device=DEV), torch.zeros(H, rows_env, Hb, device=DEV), torch.zeros(H, rows_env, device=DEV)
        one = engine.planet_rollout(actions[cs].contiguous(), lat_d[e_].contiguous(), bel_d[e_].contiguous(), P, eps=eps[:, rs].contiguous(),
                                    trace_latent=tl, trace_belief=tb, trace_rewards=tr)
        assert torch.equal(static[0][cs], one), e_
        assert torch.equal(static[1][:, rs], tl) and torch.equal(static[2][:, rs], tb) and torch.equal(static[3][:, rs], tr), e_
        ref = pl.planet_rollout(pm, actions[cs].cpu(), latent0[e_:e_ + 1], belief0[e_:e_ + 1], P, eps=eps[:, rs].cpu())
        close(static[0][cs], ref)
    if n_env > 1:  # the environments really start from different states
        assert not torch.equal(static[0][:pop_env], static[0][pop_env:2 * pop_env])
    monkeypatch.setenv("HIPETS_PLANET_GENERIC", "1")
    assert engine.planet_kernel_class() == "generic"
    generic = batched()
    for a, b in zip(static, generic):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n_env", [1, 3])
def test_batched_planet_rollout_philox(engine, n_env):
    """In-kernel draws stay keyed by the launch-global row: replay per environment with the eps exported for those rows."""
    L, A, Hb, F = 12, 3, 48, 40
    pop_env, P, H, seed, stream = 21, 3, 6, 5, 9
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=9)
    engine.planet_set_model(to_planet_spec(pm))
    latent0, belief0 = start_states(n_env, L, Hb, seed=4)
    g = torch.Generator().manual_seed(1)
    actions = torch.rand(n_env * pop_env, H, A, generator=g) * 2 - 1
    out = engine.planet_rollout(actions.to(DEV), latent0.to(DEV), belief0.to(DEV), P, seed=seed, stream_id=stream, n_env=n_env).cpu()
    ref = planet_replay(engine, pm, latent0, belief0, P, H, seed)(actions, stream)
    close(out, ref)


def test_batched_planet_cem_single_environment_equals_the_fused_plan(engine):
    """BatchedCEMAgent with n_env = 1 (hipets_plan_planet_cem_batched) is CEMOptimizer's fused PlaNet plan (hipets_plan_planet_cem) bit
    for bit, over two plans: the second from the agent's shifted warm start."""
    L, A, Hb, F = CONF
    H, pop, iters, P = 12, 300, 4, 2
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=4)
    fn = hipets.make_eval_fn(to_planet_spec(pm), P, engine=engine, seed=2)
    latent0, belief0 = start_states(1, L, Hb, seed=0)
    fn.set_state(latent0, belief0)
    lb, ub = [-1.0] * A, [1.0] * A
    single = hipets.CEMOptimizer(iters, 0.1, pop, [lb] * H, [ub] * H, 0.0, DEV, return_mean_elites=True, clipped_normal=True, seed=7)
    agent = hipets.BatchedCEMAgent(fn, 1, lb, ub, H, iters, 0.1, pop, 0.0, return_mean_elites=True, clipped_normal=True, seed=7)
    obs = np.zeros((1, 3, 64, 64), np.float32)
    obj = _BoundObjective(fn, obs[0])
    x0 = torch.zeros(H, A)
    for _ in range(2):
        one = single.optimize(obj, x0=x0)
        got = torch.from_numpy(agent.plan(obs, latent=latent0, belief=belief0))[0]
        assert torch.isfinite(got).all() and torch.equal(got, one.cpu())
        x0 = agent.previous_solution[0].cpu().clone()
        assert torch.equal(x0[:-1], got[1:]) and (x0[-1] == 0).all()


def test_batched_planet_cem_replayed_per_environment(engine):
    """n_env = 3 at the conf shape: each environment is the oracle's CEM over the oracle's PlaNet rollouts from its own start state,
    replayed with the plan's population noise and eps and teacher-forced from the plan trace."""
    L, A, Hb, F = CONF
    H, pop, iters, P, n_env = 12, 400, 5, 1, 3
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=4)
    fn = hipets.make_eval_fn(to_planet_spec(pm), P, engine=engine, seed=2)
    latent0, belief0 = start_states(n_env, L, Hb, seed=1)
    lb, ub = [-1.0] * A, [1.0] * A
    agent = hipets.BatchedCEMAgent(fn, n_env, lb, ub, H, iters, 0.1, pop, 0.0, return_mean_elites=True, clipped_normal=True, seed=7)
    K = agent.elite_num
    tr = engine.set_plan_trace(iters, n_env * pop, H, A, K, n_env=n_env)
    plans = agent.plan(np.zeros((n_env, 3, 64, 64), np.float32), latent=latent0.to(DEV), belief=belief0.to(DEV))
    torch.cuda.synchronize()
    engine.set_plan_trace(0)
    assert plans.shape == (n_env, H, A) and np.isfinite(plans).all()
    seed, plan_id = agent.seed ^ fn.seed, agent.calls
    # z of the clipped-normal sampler, indexed over all environments' candidates (mu 0, dispersion 1, wide bounds -> population == z)
    p = engine.cem_params(n_env * pop, H, A, iters, K, 0.0, True, True)
    one, zero = torch.ones(H, A, device=DEV), torch.zeros(H, A, device=DEV)
    z = []
    for i in range(iters):
        buf = torch.empty(n_env * pop, H, A, device=DEV)
        engine.cem_sample(p, zero, one, -1e3 * one, 1e3 * one, buf, seed=seed, stream_id=plan_id * iters + i)
        z.append(buf.cpu())
    eps = [engine_normals(engine, H, n_env * pop * P, L, seed, plan_id * iters + i) for i in range(iters)]
    lower, upper = -torch.ones(H, A), torch.ones(H, A)
    for e_ in range(n_env):
        it = {"i": 0}

        def oracle_obj(population, e_=e_):
            i = it["i"]
            it["i"] += 1
            return pl.planet_rollout(pm, population, latent0[e_:e_ + 1], belief0[e_:e_ + 1], P,
                                     eps=eps[i][:, e_ * pop * P:(e_ + 1) * pop * P])

        teacher = [(tr["mus"][i][e_].cpu(), tr["dispersions"][i][e_].cpu()) for i in range(iters)]
        rec = []
        po.cem_optimize(oracle_obj, torch.zeros(H, A), lower, upper, iters, 0.1, pop, 0.0, return_mean_elites=True, clipped_normal=True,
                        noise=[zi[e_ * pop:(e_ + 1) * pop] for zi in z], record=rec, teacher=teacher)
        for i in range(iters):
            rows = slice(e_ * pop, (e_ + 1) * pop)
            assert torch.allclose(tr["populations"][i][rows].cpu(), rec[i]["population"], rtol=0, atol=1e-5), (e_, i)
            check_values(tr["values"][i][rows].cpu(), rec[i]["values"])
            if set(tr["elite_idx"][i][e_].cpu().tolist()) == set(rec[i]["elite_idx"].tolist()):
                assert torch.allclose(tr["mus"][i][e_].cpu(), rec[i]["mu"], rtol=0, atol=1e-4), (e_, i)  # T4
                assert torch.allclose(tr["dispersions"][i][e_].cpu(), rec[i]["disp"], rtol=1e-4, atol=1e-5), (e_, i)
        assert np.array_equal(plans[e_], tr["mus"][iters - 1][e_].cpu().numpy())
    assert not np.array_equal(plans[0], plans[1])


def test_batched_planet_mppi_plans(engine):
    L, A, Hb, F = 12, 3, 48, 40
    H, P, pop, n_env, iters = 7, 3, 90, 3, 3
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=6)
    fn = hipets.make_eval_fn(to_planet_spec(pm), P, engine=engine, seed=3)
    latent0, belief0 = start_states(n_env, L, Hb, seed=2)
    lb, ub = [-1.0] * A, [1.0] * A
    agent = hipets.BatchedMPPIAgent(fn, n_env, lb, ub, H, iters, pop, 0.9, 1.0, 0.9, seed=7)
    lower, upper = -torch.ones(H, A), torch.ones(H, A)
    states = [po.MPPIState(H, A) for _ in range(n_env)]
    one_t, zero_t = torch.ones(H, A, device=DEV), torch.zeros(H, A, device=DEV)
    obs = np.zeros((n_env, 3, 64, 64), np.float32)
    for call in range(2):  # the persistent mean carries over, shifted one step
        tr = engine.set_plan_trace(iters, n_env * pop, H, A, 1, n_env=n_env)
        plans = agent.plan(obs, latent=latent0, belief=belief0)
        torch.cuda.synchronize()
        engine.set_plan_trace(0)
        seed, plan_id = agent.seed ^ fn.seed, agent.calls
        roll = planet_replay(engine, pm, latent0, belief0, P, H, seed)
        z = []
        for k in range(iters):
            buf = torch.empty(n_env * pop, H, A, device=DEV)
            engine.mppi_sample(n_env * pop, H, A, 1.0, zero_t, torch.zeros(A, device=DEV), -1e3 * one_t, 1e3 * one_t, buf, seed=seed,
                               stream_id=plan_id * iters + k)
            z.append(buf.cpu())
        vals = [roll(tr["populations"][k].cpu(), plan_id * iters + k) for k in range(iters)]
        for k in range(iters):
            check_values(tr["values"][k].cpu(), vals[k])
        for e_ in range(n_env):
            it = {"i": 0}

            def obj(population, e_=e_):
                k = it["i"]
                it["i"] += 1
                assert torch.allclose(population, tr["populations"][k].cpu()[e_ * pop:(e_ + 1) * pop], rtol=0, atol=2e-5)
                return vals[k][e_ * pop:(e_ + 1) * pop]

            ref = po.mppi_optimize(obj, states[e_], lower, upper, iters, pop, 0.9, 1.0, 0.9, noise=[zk[e_ * pop:(e_ + 1) * pop] for zk in z])
            assert np.allclose(plans[e_], ref.numpy(), rtol=0, atol=1e-4), (call, e_)
    assert plans.shape == (n_env, H, A)
    assert agent.act(obs, latent=latent0, belief=belief0).shape == (n_env, A)


def test_batched_planet_icem_plans(engine):
    L, A, Hb, F = 12, 3, 48, 40
    H, P, pop, n_env, iters, module = 8, 2, 150, 3, 4, 5
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=8)
    fn = hipets.make_eval_fn(to_planet_spec(pm), P, engine=engine, seed=3)
    latent0, belief0 = start_states(n_env, L, Hb, seed=3)
    lb, ub = [-1.0] * A, [1.0] * A
    kw = dict(num_iterations=iters, elite_ratio=0.1, population_size=pop, population_decay_factor=1.3, colored_noise_exponent=2.0,
              keep_elite_frac=0.3, alpha=0.1, return_mean_elites=True, population_size_module=module)
    K, keep, sizes = po.icem_sizes(iters, 0.1, pop, 1.3, 0.3, module)
    g = torch.Generator().manual_seed(0)
    agent = hipets.BatchedICEMAgent(fn, n_env, lb, ub, H, seed=7, **kw)
    lower, upper = -torch.ones(H, A), torch.ones(H, A)
    states = [po.ICEMState() for _ in range(n_env)]
    one_t, zero_t = torch.ones(H, A, device=DEV), torch.zeros(H, A, device=DEV)
    obs = np.zeros((n_env, 3, 64, 64), np.float32)
    for call in range(2):  # the second plan starts from kept / shifted elites and ends on the +1 mu row
        perms = [[torch.randperm(K, generator=g) for _ in range(n_env)] for _ in range(iters)]
        kidx = torch.stack([torch.stack([pe[:keep] for pe in perms[i]]) for i in range(iters)]).to(torch.int32).to(DEV).contiguous()
        had_elite = agent.has_elite
        x0_all = agent.previous_solution.cpu().clone()
        tr = engine.set_plan_trace(iters, n_env * (sizes[0] + keep), H, A, K, n_env=n_env)
        plans = agent.plan(obs, keep_idx=kidx, latent=latent0, belief=belief0)
        torch.cuda.synchronize()
        engine.set_plan_trace(0)
        seed, plan_id = agent.seed ^ fn.seed, agent.calls
        roll = planet_replay(engine, pm, latent0, belief0, P, H, seed)
        rows_i, noise_i, tail_i = [], [], None
        for i in range(iters):
            sid = (plan_id * iters + i) * 4
            extra = 0
            if had_elite or i > 0:
                extra = 1 if (i == iters - 1 and i != 0) else keep
            rows_i.append(sizes[i] + extra)
            buf = torch.empty(n_env * sizes[i], H, A, device=DEV)
            engine.icem_sample(n_env * sizes[i], H, A, 2.0, zero_t, one_t, -1e3 * one_t, 1e3 * one_t, buf, seed=seed, stream_id=sid)
            noise_i.append(buf.cpu())
            if i == 0 and had_elite:
                sh = torch.empty(n_env * keep, H, A, device=DEV)
                engine.icem_shift(n_env * keep, H, A, torch.zeros(n_env * keep, H, A, device=DEV), zero_t, one_t, sh, seed=seed, stream_id=sid + 1)
                tail_i = sh[:, H - 1, :].cpu()
        vals = [roll(tr["populations"][i][: n_env * rows_i[i]].cpu(), (plan_id * iters + i) * 4 + 3) for i in range(iters)]
        for i in range(iters):
            check_values(tr["values"][i][: n_env * rows_i[i]].cpu(), vals[i])
        for e_ in range(n_env):
            inject, teacher = [], []
            for i in range(iters):
                n, r = sizes[i], rows_i[i]
                inj = {"noise": noise_i[i][e_ * n:(e_ + 1) * n], "keep_perm": perms[i][e_]}
                if i == 0 and had_elite:
                    inj["end_noise"] = tail_i[e_ * keep:(e_ + 1) * keep]
                inject.append(inj)
                pop_e = tr["populations"][i].cpu()[e_ * r:(e_ + 1) * r]
                teacher.append((tr["mus"][i][e_].cpu(), tr["dispersions"][i][e_].cpu(), pop_e[tr["elite_idx"][i][e_].cpu().long()]))
            it = {"i": 0}

            def obj(population, e_=e_):
                i = it["i"]
                it["i"] += 1
                r = rows_i[i]
                assert torch.allclose(population, tr["populations"][i].cpu()[e_ * r:(e_ + 1) * r], rtol=0, atol=1e-5), (call, e_, i)
                return vals[i][e_ * r:(e_ + 1) * r]

            rec = []
            po.icem_optimize(obj, states[e_], x0_all[e_], lower, upper, iters, 0.1, pop, 1.3, 2.0, 0.3, 0.1, return_mean_elites=True,
                             population_size_module=module, inject=inject, record=rec, teacher=teacher)
            states[e_].elite = agent.elite[e_].cpu()
            for i in range(iters):
                if elites_agree(tr["elite_idx"][i][e_].cpu(), rec[i]["values"], K):
                    assert torch.allclose(tr["mus"][i][e_].cpu(), rec[i]["mu"], rtol=0, atol=1e-4), (call, e_, i)
                    assert torch.allclose(tr["dispersions"][i][e_].cpu(), rec[i]["var"], rtol=1e-4, atol=1e-5), (call, e_, i)
            assert np.array_equal(plans[e_], tr["mus"][iters - 1][e_].cpu().numpy())
    assert agent.act(obs, latent=latent0, belief=belief0).shape == (n_env, A)


def test_batched_planet_refusals(engine):
    L, A, Hb, F = 12, 3, 48, 40
    H, n_env = 5, 3
    spec = to_planet_spec(pl.make_synthetic_planet(L, A, Hb, F, seed=1))
    lb, ub = [-1.0] * A, [1.0] * A
    exact = hipets.make_eval_fn(spec, 1, engine=engine, mode="exact")
    assert exact.kernel_mode is None
    with pytest.raises(ValueError, match="in-kernel randomness"):
        hipets.BatchedCEMAgent(exact, n_env, lb, ub, H, 2, 0.1, 50, 0.0)
    with pytest.raises(ValueError, match="in-kernel randomness"):
        hipets.BatchedMPPIAgent(exact, n_env, lb, ub, H, 2, 50, 0.9, 1.0, 0.9)
    with pytest.raises(ValueError, match="in-kernel randomness"):
        hipets.BatchedICEMAgent(exact, n_env, lb, ub, H, num_iterations=2, elite_ratio=0.1, population_size=50, population_decay_factor=1.3,
                                colored_noise_exponent=2.0, keep_elite_frac=0.3, alpha=0.1)
    fn = hipets.make_eval_fn(spec, 1, engine=engine)
    assert fn.kernel_mode == "device"
    latent0, belief0 = start_states(n_env, L, Hb, seed=0)
    obs = np.zeros((n_env, 3, 64, 64), np.float32)
    agents = [hipets.BatchedCEMAgent(fn, n_env, lb, ub, H, 2, 0.1, 50, 0.0),
              hipets.BatchedMPPIAgent(fn, n_env, lb, ub, H, 2, 50, 0.9, 1.0, 0.9),
              hipets.BatchedICEMAgent(fn, n_env, lb, ub, H, num_iterations=2, elite_ratio=0.1, population_size=50, population_decay_factor=1.3,
                                      colored_noise_exponent=2.0, keep_elite_frac=0.3, alpha=0.1)]
    for agent in agents:
        with pytest.raises(ValueError, match="start states"):
            agent.plan(obs)
        with pytest.raises(ValueError, match="start states"):
            agent.act(obs, latent=latent0)
        with pytest.raises(ValueError, match="latent must have shape"):
            agent.plan(obs, latent=latent0[:2], belief=belief0)
        with pytest.raises(ValueError, match="belief must have shape"):
            agent.plan(obs, latent=latent0, belief=belief0[:, :-1])
        with pytest.raises(ValueError, match="obs_batch"):
            agent.plan(obs[:2], latent=latent0, belief=belief0)
        assert agent.calls == 0
    engine.planet_set_model(spec)
    with pytest.raises(hipets.HipetsError, match="not divisible by n_env 3"):
        engine.planet_rollout(torch.zeros(10, H, A, device=DEV), latent0.to(DEV), belief0.to(DEV), 1, n_env=3)
