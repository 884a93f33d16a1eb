"""hipets.CallableTrajectoryEvalFn -- the one-launch objective for Python reward / termination callables -- and the entry point under
it, hipets_trajectory_returns:

A  the reduce kernel, bit for bit against the numpy float32 restatement of its chain (tests/returns_restatement.py)
B  the objective with the kernel's own learned reward and a Python termination that never fires == the fused objective, bitwise
C  the objective with the oracle's closed forms as Python callables, replayed through the oracle from the exports of its streams (T2)
D  trajectories(): traced states against the oracle step by step (T1), rewards / dones / returns consistent with the callables
E  through CEMOptimizer and through an agent in the closed loop of tests/test_gpu_closed_loop.py"""
import ctypes as C

import numpy as np
import pytest
import torch

import callable_cases as cc
import hipets
from conftest import to_spec
from hipets import _lib
from hipets.planning import _BoundObjective
from oracle import pets_oracle as po
from returns_restatement import same_bits, trajectory_returns_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T1 = dict(rtol=1e-5, atol=2e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# A  hipets_trajectory_returns
# ---------------------------------------------------------------------------------------------------------------------------
# B = 1, 35, 120, 2000, 900 rows: off every multiple of 64 and 256 but for none; (3, 300, 4): a candidate's particles exceed a workgroup,
# the row pass + particle_mean_kernel
REDUCE_SHAPES = [(1, 1, 1), (5, 7, 33), (24, 5, 6), (100, 20, 5), (3, 300, 4)]


def reduce_inputs(pop, P, H, seed, plant=False):
    rng = np.random.default_rng(seed)
    B = pop * P
    rewards = rng.standard_normal((H, B)).astype(np.float32) * 3
    first = rng.integers(0, H + 2, size=B)  # the first firing step: 0 .. H - 1, or never (H, H + 1)
    first[: min(B, 3)] = [0, H, H - 1][: min(B, 3)]
    dones = (rng.random((H, B)) < 0.3) & (np.arange(H)[:, None] > first[None, :])  # later flags behind the first change nothing
    dones |= np.arange(H)[:, None] == first[None, :]
    if plant:  # non-finite rewards behind a termination (masked: exactly 0), at one (counted) and ahead of one (propagate)
        for row, (t_done, t_bad, v) in enumerate([(1, 3, np.nan), (1, 2, np.inf), (0, 1, -np.inf), (2, 2, np.nan), (3, 1, np.inf), (H, 0, np.nan)]):
            dones[:, row] = np.arange(H) == t_done
            rewards[t_bad, row] = v
    return rewards, dones.astype(np.uint8)


@pytest.mark.parametrize("pop,P,H", REDUCE_SHAPES, ids=[f"pop{a}_P{b}_H{c}" for a, b, c in REDUCE_SHAPES])
@pytest.mark.parametrize("as_bool", [False, True], ids=["uint8", "bool"])
def test_trajectory_returns_equals_its_restatement_bit_for_bit(engine, pop, P, H, as_bool):
    rewards, dones = reduce_inputs(pop, P, H, seed=pop + H)
    want_ret, want_tot, want_first = trajectory_returns_np(rewards, dones, pop, P)
    r, d = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
    if as_bool:
        d = d.bool()
    ret, tot, first = engine.trajectory_returns(r, d, pop, P, row_totals=True, first_done=True)
    assert same_bits(ret.cpu().numpy(), want_ret) and same_bits(tot.cpu().numpy(), want_tot)
    assert first.dtype == torch.int32 and np.array_equal(first.cpu().numpy(), want_first)
    only = engine.trajectory_returns(r, d, pop, P)  # no optional outputs (the two-pass form then runs on the engine's own row totals)
    assert same_bits(only.cpu().numpy(), want_ret)
    ret2, tot2, first2 = engine.trajectory_returns(r, d, pop, P, first_done=True)
    assert tot2 is None and same_bits(ret2.cpu().numpy(), want_ret) and np.array_equal(first2.cpu().numpy(), want_first)


@pytest.mark.parametrize("pop,P,H", [(5, 7, 33), (3, 300, 4)])
def test_trajectory_returns_masks_by_select(engine, pop, P, H):
    """inf / NaN rewards behind a termination add exactly 0; at or ahead of it they count"""
    rewards, dones = reduce_inputs(pop, P, H, seed=1, plant=True)
    want_ret, want_tot, want_first = trajectory_returns_np(rewards, dones, pop, P)
    assert np.isfinite(want_tot[:3]).all() and np.isnan(want_tot[3]) and np.isinf(want_tot[4]) and np.isnan(want_tot[5])
    ret, tot, first = engine.trajectory_returns(torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV), pop, P, row_totals=True,
                                                first_done=True)
    assert same_bits(tot.cpu().numpy(), want_tot) and same_bits(ret.cpu().numpy(), want_ret) and np.array_equal(first.cpu().numpy(), want_first)


def test_trajectory_returns_refuses_invalid_arguments(engine):
    lib = _lib.load()
    r, d, out = torch.zeros(2, 6, device=DEV), torch.zeros(2, 6, dtype=torch.uint8, device=DEV), torch.zeros(3, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ok = (engine._h, p(r), p(d), 3, 2, 2, p(out), None, None, None)
    assert lib.hipets_trajectory_returns(*ok) == 0
    for pos, bad in ((0, None), (1, None), (2, None), (6, None), (3, 0), (4, 0), (5, 0), (3, -1)):
        args = list(ok)
        args[pos] = bad
        assert lib.hipets_trajectory_returns(*args) != 0
        assert lib.hipets_last_error_kind() == _lib.ERR_INVALID_ARGUMENT, lib.hipets_last_error()
    with pytest.raises(ValueError):
        engine.trajectory_returns(r, d, 4, 2)  # 6 rows per step are not 4 x 2
    with pytest.raises(ValueError):
        engine.trajectory_returns(r, d.float(), 3, 2)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# B  bitwise anchor: the kernel's learned reward off the tap + a termination that never fires == the fused objective
# ---------------------------------------------------------------------------------------------------------------------------
ANCHORS = [("hid40", 11, 3, dict(ensemble_size=5, hid=40), 24, 5, 6),
           ("hid200_elites", 11, 3, dict(ensemble_size=7, elite=cc.ELITE, hid=200), 100, 20, 5)]


def never(act, nobs):
    return torch.zeros(len(nobs), dtype=torch.bool, device=nobs.device)


@pytest.mark.parametrize("name,obs,act,mkw,pop,P,H", ANCHORS, ids=[c[0] for c in ANCHORS])
@pytest.mark.parametrize("mode,persistent", [("device", True), ("device", False), ("fast", True)], ids=["device_persistent", "device_per_step", "fast"])
def test_learned_reward_with_idle_termination_equals_the_fused_objective(engine, name, obs, act, mkw, pop, P, H, mode, persistent):
    om = po.make_synthetic_model(obs, act, seed=4, learned_rewards=True, reward=None, **mkw)
    spec = to_spec(om, obs, act)
    s0 = (np.random.default_rng(5).standard_normal(obs) * 0.1).astype(np.float32)
    fused = hipets.HipTrajectoryEvalFn(spec, P, engine=engine, seed=23, mode=mode)
    fn = hipets.CallableTrajectoryEvalFn(spec, P, termination_fn=never, engine=engine, seed=23, mode=mode)
    engine.set_persistent(persistent)
    try:
        for a in cc.call_actions(act, pop, H):
            want = fused(s0, a.to(DEV))
            got = fn(s0, a.to(DEV))
            assert fused.calls == fn.calls
            assert torch.isfinite(want).all() and float(want.abs().max()) > 0
            assert torch.equal(got, want), f"max diff {(got - want).abs().max():.3e}"
    finally:
        engine.set_persistent(True)


# ---------------------------------------------------------------------------------------------------------------------------
# C  oracle replays
# ---------------------------------------------------------------------------------------------------------------------------
def engine_draws(engine, om, pop, P, H, mode, stream):
    """oracle kwargs of the call with stream `stream`, from what the engine exports for (seed, stream)"""
    B = pop * P
    eps = engine.fast_normals(H, B, cc.SEED, stream).cpu()
    if mode == "device":
        return dict(perms=engine.device_perms(H, B, cc.SEED, stream).cpu(), eps=eps)
    nwg, r = engine.fast_geometry(pop, P, H, -1)  # a call with traces runs the general layout
    return dict(members=cc.fast_member_map(engine.fast_schedule(H, nwg, cc.SEED, stream).cpu(), B, P, r), eps=eps)


@pytest.mark.parametrize("name,obs,act,mkw,pop,P,H,mode", cc.REPLAYS, ids=cc.REPLAY_IDS)
def test_callable_objective_replayed_through_oracle(engine, name, obs, act, mkw, pop, P, H, mode):
    """Two consecutive calls; the oracle's own closed forms are the Python callables.  T2: |out - ref| <= 1e-4 max(|ref|, 1) on the
    candidates none of whose rows comes within 1e-4 of a termination threshold, at most cc.MAX_EXCLUDED excluded."""
    om, s0 = cc.make_case(obs, act, mkw)
    spec = to_spec(om, obs, act)
    rew_fn, term_fn = cc.callables(om)
    fn = hipets.CallableTrajectoryEvalFn(spec, P, reward_fn=rew_fn, termination_fn=term_fn, engine=engine, seed=cc.SEED, mode=mode,
                                         rng=torch.Generator().manual_seed(cc.EXACT_GENERATOR_SEED))
    replay_generator = torch.Generator().manual_seed(cc.EXACT_GENERATOR_SEED)
    for call, actions in enumerate(cc.call_actions(act, pop, H), start=1):
        if mode == "exact":
            torch.manual_seed(100 + call)  # (the permutations of the reference order come from the global generator)
        out = fn(s0, actions.to(DEV)).cpu()
        assert fn.calls == call
        draws = cc.exact_draws(spec, pop * P, H, call, replay_generator) if mode == "exact" else engine_draws(engine, om, pop, P, H, mode, call)
        ref, keep, ended, _ = cc.oracle_replay(om, actions, s0, P, draws)
        cc.assert_replay_is_usable(om, keep, ended)
        assert torch.isfinite(out).all()
        err = (out - ref).abs()[keep]
        print(f"{name} call {call}: max err {err.max():.3e}, excluded {int((~keep).sum())}")
        assert (err <= 1e-4 * torch.clamp(ref[keep].abs(), min=1.0)).all(), f"max err {err.max():.3e}"  # T2


# ---------------------------------------------------------------------------------------------------------------------------
# D  trajectories()
# ---------------------------------------------------------------------------------------------------------------------------
def test_trajectories_of_the_callable_objective(engine):
    name, obs, act, mkw, pop, P, H, mode = cc.REPLAYS[2]
    assert name == "small_hopper_device"
    om, s0 = cc.make_case(obs, act, mkw)
    spec = to_spec(om, obs, act)
    rew_fn, term_fn = cc.callables(om)
    B = pop * P
    fns = [hipets.CallableTrajectoryEvalFn(spec, P, reward_fn=rew_fn, termination_fn=term_fn, engine=engine, seed=cc.SEED) for _ in range(2)]
    actions = cc.call_actions(act, pop, H)[0]
    returns = fns[1](s0, actions.to(DEV)).clone()
    tr = fns[0].trajectories(s0, actions.to(DEV))
    assert {k: tuple(v.shape) for k, v in tr.items()} == {"next_obs": (H, B, obs), "rewards": (H, B), "dones": (H, B), "first_done": (B,),
                                                          "row_totals": (B,), "returns": (pop,)}
    assert tr["dones"].dtype == torch.bool and tr["first_done"].dtype == torch.int32
    assert torch.equal(tr["returns"], returns)  # == __call__ of the same stream
    # the traced states, one step at a time from the GPU's own previous state: T1, the rule of one transition
    draws = engine_draws(engine, om, pop, P, H, mode, 1)
    nobs = tr["next_obs"].cpu()
    x = torch.from_numpy(np.tile(s0, (B, 1)))
    for t in range(H):
        a = torch.repeat_interleave(actions[:, t], P, dim=0)
        ref_nobs, _, _ = po.step(om, x, a, perm=draws["perms"][t], eps=draws["eps"][t])
        assert torch.allclose(nobs[t], ref_nobs, **T1), f"step {t}: max err {(nobs[t] - ref_nobs).abs().max():.3e}"
        x = nobs[t]
    # rewards / dones are the callables over the traced states; totals, first terminating steps and returns follow from them
    act_rows = torch.stack([torch.repeat_interleave(actions[:, t], P, dim=0) for t in range(H)]).view(H * B, act).to(DEV)
    obs_rows = tr["next_obs"].view(H * B, obs)
    assert torch.equal(tr["rewards"], rew_fn(act_rows, obs_rows).view(H, B))
    assert torch.equal(tr["dones"], term_fn(act_rows, obs_rows).view(H, B))
    assert 0 < int(tr["dones"][0].sum()) and int(tr["dones"].any(0).sum()) < B
    ret, tot, first = trajectory_returns_np(tr["rewards"].cpu().numpy(), tr["dones"].cpu().numpy(), pop, P)
    assert same_bits(tr["returns"].cpu().numpy(), ret) and same_bits(tr["row_totals"].cpu().numpy(), tot)
    assert np.array_equal(tr["first_done"].cpu().numpy(), first)


@pytest.mark.parametrize("hid,members,elite,pop,P,H", [(40, 5, None, 24, 5, 6), (200, 7, cc.ELITE, 100, 20, 5)], ids=["hid40", "hid200"])
def test_trajectories_of_the_fused_objective_return_the_untapped_bits(engine, hid, members, elite, pop, P, H):
    """HipTrajectoryEvalFn.trajectories on a closed-form model (halfcheetah reward, hopper termination): the kernel's rewards off the
    tap, the termination restated in torch, reduced by hipets_trajectory_returns == the untapped call of the same (seed, stream),
    generic_kernel=2 for both."""
    om, s0 = cc.make_case(11, 3, dict(ensemble_size=members, elite=elite, hid=hid, termination="hopper"))
    spec = to_spec(om, 11, 3)
    fn = hipets.HipTrajectoryEvalFn(spec, P, engine=engine, seed=cc.SEED)
    fn.rollout_kw = {"generic_kernel": 2}
    for call, actions in enumerate(cc.call_actions(3, pop, H), start=1):
        tr = fn.trajectories(s0, actions.to(DEV))
        assert fn.calls == call
        want = engine.rollout(actions.to(DEV), s0, P, mode="device", seed=cc.SEED, stream_id=call, generic_kernel=2)
        assert torch.equal(tr["returns"], want), f"max diff {(tr['returns'] - want).abs().max():.3e}"
        ended = tr["dones"].cummax(0).values
        assert 0 < int(ended[0].sum()) < int(ended[-1].sum()) < pop * P  # the termination matters to these returns
        assert torch.equal(tr["dones"], po.term_hopper(None, tr["next_obs"].view(-1, 11)).view(H, -1))


# ---------------------------------------------------------------------------------------------------------------------------
# E  through an optimizer and an agent
# ---------------------------------------------------------------------------------------------------------------------------
def test_cem_runs_its_iteration_loop_and_calls_the_callable_once_per_iteration(engine):
    obs, act, pop, P, H, iters = 11, 3, 50, 5, 6, 4
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=40, seed=2)
    s0 = np.zeros(obs, np.float32)
    sizes = []

    def rew(a, o):
        sizes.append(len(o))
        return po.rew_halfcheetah(a, o)

    for check, extra in ((True, [pop * P]), (False, [])):
        del sizes[:]
        fn = hipets.CallableTrajectoryEvalFn(to_spec(om, obs, act), P, reward_fn=rew, engine=engine, seed=3, check_rowwise=check)
        opt = hipets.CEMOptimizer(iters, 0.1, pop, [[-1.0] * act] * H, [[1.0] * act] * H, 0.1, DEV, return_mean_elites=True, seed=7)
        plan = opt.optimize(_BoundObjective(fn, s0), x0=torch.zeros(H, act))
        assert torch.isfinite(plan).all() and tuple(plan.shape) == (H, act)
        assert fn.calls == iters
        assert sizes == [H * pop * P] + extra + [H * pop * P] * (iters - 1)  # one call per iteration (+ the row-wise check's, once)


def test_pets_solves_the_point_mass_task_with_the_callable_objective(engine):
    """tests/test_gpu_closed_loop.py's unfused_python_reward case with the one-launch objective in place of the per-step one: the same
    task, training, planner and threshold."""
    import test_gpu_closed_loop as cl

    torch.manual_seed(12345)
    rng = np.random.default_rng(12345)
    env = cl.MockLineEnv()
    o, a, nx = cl.collect_random(env, 600, rng)
    ws, bs, mn, mx, nmean, nstd = cl.train_ensemble(o, a, nx)
    spec = hipets.ModelSpec(reward="none", termination="no_termination", weights=ws, biases=bs, obs_dim=2, act_dim=1, min_logvar=mn,
                            max_logvar=mx, norm_mean=nmean, norm_std=nstd, activation="silu", propagation="random_model")
    fn = hipets.CallableTrajectoryEvalFn(spec, 20, reward_fn=cl.mock_reward_fn, engine=engine, seed=1)
    cfg = dict(_target_="hipets.CEMOptimizer", num_iterations=5, elite_ratio=0.1, population_size=500, alpha=0.1, device=DEV,
               lower_bound="???", upper_bound="???", return_mean_elites=True, seed=3)
    agent = hipets.TrajectoryOptimizerAgent(cfg, [-1.0], [1.0], planning_horizon=15)
    agent.set_trajectory_eval_fn(fn)
    best = -np.inf
    for trial in range(3):
        obs = env.reset()
        agent.reset()
        total, done = 0.0, False
        while not done:
            obs, r, done = env.step(agent.act(obs))
            total += r
        best = max(best, total)
        if best > cl.TARGET:
            break
    assert best > cl.TARGET, best
