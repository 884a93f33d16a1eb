"""Value-bootstrapped planning on the MI355X (hipets/value.py; hipets_critic_* and hipets_discounted_returns of include/hipets.h):

A  the critic kernel against the float64 restatement of QNetwork.forward (tests/value_restatement.py) under the actor tests' rule,
   T1 x max(1, 4 u) with u = torch CPU's own float32 share of T1 on the case's rows; qmin, row independence, determinism, geometry
B  hipets_discounted_returns bit for bit against its numpy float32 restatement, and against hipets_trajectory_returns at gamma = 1
C  hipets.ValueTrajectoryEvalFn: the fused objective's bits without discount and agent, the restatement over its own trajectory with a
   critic, staleness after SAC updates, through CEM and an agent, and a decision that only the terminal value explains"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import callable_cases as cc
import hipets
import policy_restatement as pr
import value_restatement as vr
from conftest import to_spec
from hipets import _lib
from hipets.planning import _BoundObjective
from hipets.reduce import ParticleReduce
from oracle import pets_oracle as po
from returns_restatement import same_bits
from sac_restatement import FixedMemory, TinyGaussianPolicy, TinyQNetwork, TinySAC
from test_gpu_callable_objective import REDUCE_SHAPES, reduce_inputs
from test_gpu_policy import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_LIMIT = 160 * 1024


def pad16(x):
    return (x + 15) // 16 * 16


def bare_critic(w, device=DEV):
    """A QNetwork-shaped module holding a case's weights"""
    hid, K = w["cw1"].shape
    q = TinyQNetwork(K - 1, 1, hid)
    with torch.no_grad():
        for i in range(1, 7):
            getattr(q, f"linear{i}").weight.copy_(torch.from_numpy(w[f"cw{i}"]))
            getattr(q, f"linear{i}").bias.copy_(torch.from_numpy(w[f"cb{i}"]))
    return q.to(device)


def critic_weights(q):
    return {f"c{k}{i}": getattr(getattr(q, f"linear{i}"), "weight" if k == "w" else "bias").detach().cpu().numpy().copy()
            for i in range(1, 7) for k in "wb"}


def policy_weights(p):
    w = {}
    for k, lin in (("1", p.linear1), ("2", p.linear2), ("m", p.mean_linear), ("s", p.log_std_linear)):
        w["w" + k], w["b" + k] = lin.weight.detach().cpu().numpy().copy(), lin.bias.detach().cpu().numpy().copy()
    w["action_scale"], w["action_bias"] = p.action_scale.cpu().numpy().copy(), p.action_bias.cpu().numpy().copy()
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# A  the critic kernel
# ---------------------------------------------------------------------------------------------------------------------------
CRITIC_RUNS = [(n, o, a, h, b) for n, o, a, h, batches in vr.CRITIC_CASES for b in batches]


@pytest.mark.parametrize("name,obs_dim,act_dim,hid,batch", CRITIC_RUNS, ids=[f"{c[0]}_b{c[4]}" for c in CRITIC_RUNS])
def test_critic_matches_the_f64_restatement(engine, name, obs_dim, act_dim, hid, batch):
    w, obs, act, u_rows = vr.make_critic_case(name, obs_dim, act_dim, hid)
    assert engine.critic_set(bare_critic(w), obs_dim, act_dim) == (obs_dim, act_dim, hid)
    # the R rule: the largest of 4, 2, 1 row tiles whose two buffers fit the limit, cut down to what the batch fills
    per_tile = 16 * 4 * (max(pad16(obs_dim + act_dim), pad16(hid)) + pad16(hid) + 8)
    R, lds = engine.critic_geometry(10 ** 6)
    assert R == next(r for r in (4, 2, 1) if per_tile * r <= LDS_LIMIT) and lds == per_tile * R <= LDS_LIMIT
    assert R == {1024: 1, 512: 2}.get(hid, 4)
    B = {"R-1": 16 * R - 1, "R+1": 16 * R + 1}.get(batch, batch)
    r_b, lds_b = engine.critic_geometry(B)
    assert r_b == min(R, next((r for r in (1, 2, 4) if 16 * r >= B), 4)) and lds_b == per_tile * r_b
    obs, act, u = obs[:B], act[:B], float(u_rows[:B].max())
    x, a = torch.from_numpy(obs).to(DEV), torch.from_numpy(act).to(DEV)
    print(f"{name}: B {B}, row tiles {R} ({r_b} for this batch), LDS {lds_b}")
    r1, r2 = vr.critic_f64(w, obs, act)
    q1, q2, qmin = engine.critic_q(x, a)
    assert_within(q1, r1, u, "q1")
    assert_within(q2, r2, u, "q2")
    # qmin: the select of the kernel's own q1 and q2, bit for bit; both branches occur where the batch has more than a few rows
    assert torch.equal(qmin, torch.where(q1 < q2, q1, q2))
    if B >= 33:
        assert 0 < int((q1 < q2).sum()) < B
    # a row's arithmetic does not depend on the batch it arrives in, nor on R (a one-row call runs R = 1)
    for r in sorted({0, B // 2, B - 1}):
        o1, o2, om = engine.critic_q(x[r:r + 1].contiguous(), a[r:r + 1].contiguous())
        assert torch.equal(o1[0], q1[r]) and torch.equal(o2[0], q2[r]) and torch.equal(om[0], qmin[r]), f"row {r} alone differs"
    # the same call twice gives the same bits; outputs are optional
    again = engine.critic_q(x, a)
    assert all(torch.equal(g, h) for g, h in zip(again, (q1, q2, qmin)))
    only = engine.critic_q(x, a, q1=False, q2=False)
    assert only[0] is None and only[1] is None and torch.equal(only[2], qmin)
    only = engine.critic_q(x, a, q2=False, qmin=False)
    assert only[1] is None and only[2] is None and torch.equal(only[0], q1)


def test_qmin_follows_torch_min_on_nan(engine):
    """a NaN in either network's value is a NaN in qmin (torch.min's rule): a NaN observation poisons both, so plant it in the weights
    of one network at a time"""
    w, obs, act, _ = vr.make_critic_case("k16_h16", 12, 4, 16)
    x, a = torch.from_numpy(obs[:20]).to(DEV), torch.from_numpy(act[:20]).to(DEV)
    for layer in ("cb3", "cb6"):
        bad = dict(w)
        bad[layer] = np.full_like(w[layer], np.nan)
        engine.critic_set(bare_critic(bad), 12, 4)
        q1, q2, qmin = engine.critic_q(x, a)
        assert bool(torch.isnan(q1 if layer == "cb3" else q2).all()) and bool(torch.isfinite(q2 if layer == "cb3" else q1).all())
        assert bool(torch.isnan(qmin).all())


def test_sac_critic_reads_agents_and_shares_an_engine(engine):
    sac = TinySAC(11, 3, 24, device=DEV)
    crit = hipets.SACCritic(sac, engine=engine)
    assert crit.dims == (11, 3, 24) and crit.critic is sac.critic and not crit.stale()
    target = hipets.SACCritic(SimpleNamespace(sac_agent=sac), engine=engine, target=True)
    assert target.critic is sac.critic_target and crit.stale() and not target.stale()  # one owner slot per engine
    bare = hipets.SACCritic(sac.critic, engine=engine)  # the split comes with the first call
    assert bare.dims == (None, None, 24)
    g = torch.Generator().manual_seed(0)
    x, a = torch.randn(50, 11, generator=g).to(DEV), (torch.rand(50, 3, generator=g) * 2 - 1).to(DEV)
    q = bare.q(x, a)
    assert bare.dims == (11, 3, 24) and all(torch.equal(g_, h) for g_, h in zip(q, crit.q(x, a)))  # (crit takes the slot back)
    r1, r2 = vr.critic_f64(critic_weights(sac.critic), x.cpu().numpy(), a.cpu().numpy())
    u = float(vr.torch_cpu_share(critic_weights(sac.critic), x.cpu().numpy(), a.cpu().numpy()).max())
    assert_within(q[0], r1, u, "q1")
    assert_within(q[1], r2, u, "q2")
    # a snapshot until refresh(); a stock parameter write moves a version, which stale() sees
    with torch.no_grad():
        sac.critic.linear3.bias.add_(0.5)
    assert crit.stale() and torch.equal(crit.q(x, a)[0], q[0])
    crit.refresh()
    assert not crit.stale() and torch.allclose(crit.q(x, a)[0], q[0] + 0.5, atol=1e-5)
    with pytest.raises(ValueError, match=r"must be \[B, 11\] / \[B, 3\]"):
        crit.q(x[:, :10].contiguous(), a)
    # a critic on the CPU is snapshotted across devices
    cpu = hipets.SACCritic(TinySAC(11, 3, 24), engine=engine)
    assert all(t.device.type == "cuda" for t in cpu.q(x, a))


def test_critic_argument_refusals(engine):
    sac = TinySAC(5, 2, 16, device=DEV)
    engine.critic_set(sac.critic, 5, 2)
    z = torch.zeros(64, device=DEV)
    table = np.full(12, z.data_ptr(), dtype=np.uint64)

    def refused(symbol, **kw):
        with pytest.raises(hipets.HipetsError) as err:
            engine._call(symbol, **kw)
        assert err.value.kind == hipets.ERR_INVALID_ARGUMENT, str(err.value)

    for bad in (dict(obs_dim=0), dict(obs_dim=513), dict(hidden=0), dict(hidden=1025), dict(act_dim=0), dict(act_dim=33), dict(n_ptrs=11),
                dict(n_ptrs=13), dict(ptrs=None)):
        refused("hipets_critic_set", **{**dict(obs_dim=5, act_dim=2, hidden=16, ptrs=table, n_ptrs=12), **bad})
    holed = table.copy()
    holed[7] = 0
    refused("hipets_critic_set", obs_dim=5, act_dim=2, hidden=16, ptrs=holed, n_ptrs=12)
    # a refused set leaves the engine without a critic: a call before hipets_critic_set
    refused("hipets_critic_q", obs=z, actions=z, batch=4, q1=z, q2=None, qmin=None)
    with pytest.raises(hipets.HipetsError) as err:
        engine._query("hipets_critic_geometry", batch=4, row_tiles=None, lds_bytes=None)
    assert err.value.kind == hipets.ERR_INVALID_ARGUMENT
    engine.critic_set(sac.critic, 5, 2)
    for bad in (dict(batch=0), dict(batch=-3), dict(obs=None), dict(actions=None)):
        refused("hipets_critic_q", **{**dict(obs=z, actions=z, batch=4, q1=z, q2=None, qmin=None), **bad})
    with pytest.raises(hipets.HipetsError) as err:
        engine._query("hipets_critic_geometry", batch=0, row_tiles=None, lds_bytes=None)
    assert err.value.kind == hipets.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        engine.critic_q(torch.zeros(4, 6, device=DEV), torch.zeros(4, 2, device=DEV))
    with pytest.raises(ValueError):
        engine.critic_q(torch.zeros(4, 5, device=DEV), torch.zeros(4, 3, device=DEV))
    with pytest.raises(hipets.UnsupportedModelError):
        engine.critic_set(sac.critic, 4, 2)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# B  hipets_discounted_returns
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop,P,H", REDUCE_SHAPES, ids=[f"pop{a}_P{b}_H{c}" for a, b, c in REDUCE_SHAPES])
@pytest.mark.parametrize("gamma", [1.0, 0.99, 0.5, 0.0])
@pytest.mark.parametrize("with_values", [False, True], ids=["no_values", "values"])
@pytest.mark.parametrize("as_bool", [False, True], ids=["uint8", "bool"])
def test_discounted_returns_equal_their_restatement_bit_for_bit(engine, pop, P, H, gamma, with_values, as_bool):
    engine.set_particle_reduce(ParticleReduce.mean())
    for plant in (False, True) if (pop * P >= 6 and H >= 4) else (False,):  # (reduce_inputs plants rows 0 .. 5, steps 0 .. 3)
        rewards, dones = reduce_inputs(pop, P, H, seed=pop + H, plant=plant)
        values = np.random.default_rng(H).standard_normal(pop * P).astype(np.float32) * 5 if with_values else None
        if plant and with_values:
            values[4] = np.nan  # row 4 terminates at step 3: no bootstrap, the NaN is selected away ... (its own total is inf already)
            values[6 % (pop * P)] = np.inf
        want = vr.discounted_returns_np(rewards, dones, pop, P, gamma, values)
        r, d = torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV)
        v = torch.from_numpy(values).to(DEV) if with_values else None
        if as_bool:
            d = d.bool()
        ret, tot, first = engine.discounted_returns(r, d, pop, P, gamma=gamma, terminal_values=v, row_totals=True, first_done=True)
        assert same_bits(tot.cpu().numpy(), want[1]), f"row totals differ (plant {plant})"
        assert same_bits(ret.cpu().numpy(), want[0]) and first.dtype == torch.int32 and np.array_equal(first.cpu().numpy(), want[2])
        only = engine.discounted_returns(r, d, pop, P, gamma=gamma, terminal_values=v)  # (P > 256: on the engine's own row totals)
        assert same_bits(only.cpu().numpy(), want[0])
        if gamma == 1.0 and not with_values:  # all three outputs are hipets_trajectory_returns' bits
            ret0, tot0, first0 = engine.trajectory_returns(r, d, pop, P, row_totals=True, first_done=True)
            assert same_bits(ret.cpu().numpy(), ret0.cpu().numpy()) and same_bits(tot.cpu().numpy(), tot0.cpu().numpy())
            assert torch.equal(first, first0)


def test_a_terminated_row_gets_no_bootstrap_and_the_last_step_counts(engine):
    engine.set_particle_reduce(ParticleReduce.mean())
    H, pop, P = 4, 3, 2
    rewards = torch.ones(H, pop * P, device=DEV)
    dones = torch.zeros(H, pop * P, dtype=torch.bool, device=DEV)
    dones[H - 1, 1] = True  # terminates at the last step: its reward counts, the value does not
    dones[0, 2] = True
    values = torch.full((pop * P,), 100.0, device=DEV)
    _, tot, first = engine.discounted_returns(rewards, dones, pop, P, gamma=0.5, terminal_values=values, row_totals=True, first_done=True)
    assert tot.cpu().tolist() == [1.875 + 6.25, 1.875, 1.0, 8.125, 8.125, 8.125] and first.cpu().tolist() == [4, 3, 0, 4, 4, 4]


def test_discounted_returns_under_cvar(engine):
    pop, P, H = 24, 5, 6
    rewards, dones = reduce_inputs(pop, P, H, seed=11)
    values = np.random.default_rng(1).standard_normal(pop * P).astype(np.float32)
    red = ParticleReduce.cvar(0.4).resolve(P)
    assert red.worst_k == 2
    engine.set_particle_reduce(red)
    try:
        ret = engine.discounted_returns(torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV), pop, P, gamma=0.99,
                                        terminal_values=torch.from_numpy(values).to(DEV))
        want = vr.discounted_returns_np(rewards, dones, pop, P, 0.99, values, reduce=("worst_k", 0.0, 2))[0]
        mean = vr.discounted_returns_np(rewards, dones, pop, P, 0.99, values)[0]
        assert same_bits(ret.cpu().numpy(), want) and not same_bits(want, mean)
    finally:
        engine.set_particle_reduce(ParticleReduce.mean())


def test_discounted_returns_argument_refusals(engine):
    lib = _lib.load()
    r, d, out = torch.zeros(2, 6, device=DEV), torch.zeros(2, 6, dtype=torch.uint8, device=DEV), torch.zeros(3, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ok = [engine._h, p(r), p(d), None, C.c_float(0.9), 3, 2, 2, p(out), None, None, None]
    assert lib.hipets_discounted_returns(*ok) == 0
    for pos, bad in ((0, None), (1, None), (2, None), (8, None), (5, 0), (6, 0), (7, 0), (4, C.c_float(-0.5)), (4, C.c_float(1.5)),
                     (4, C.c_float(float("nan")))):
        args = list(ok)
        args[pos] = bad
        assert lib.hipets_discounted_returns(*args) != 0
        assert lib.hipets_last_error_kind() == _lib.ERR_INVALID_ARGUMENT, lib.hipets_last_error()
    with pytest.raises(ValueError):
        engine.discounted_returns(r, d, 4, 2)  # 6 rows per step are not 4 x 2
    with pytest.raises(ValueError, match="discount must be in"):
        engine.discounted_returns(r, d, 3, 2, gamma=1.5)
    with pytest.raises(ValueError):
        engine.discounted_returns(r, d, 3, 2, terminal_values=torch.zeros(5, device=DEV))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# C  the objective
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [("hid40", dict(ensemble_size=5, hid=40), 24, 5, 6), ("hid200_elites", dict(ensemble_size=7, elite=cc.ELITE, hid=200), 100, 20, 5)]
SHAPE_IDS = [s[0] for s in SHAPES]
OBS, ACT = 11, 3


@pytest.mark.parametrize("name,mkw,pop,P,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("mode,persistent", [("device", True), ("device", False), ("fast", True)], ids=["device_persistent", "device_per_step", "fast"])
def test_without_discount_and_agent_it_is_the_fused_objective(engine, name, mkw, pop, P, H, mode, persistent):
    """discount=1, agent=None == HipTrajectoryEvalFn of the same seed and stream, bit for bit (a learned reward off the tap; the
    closed-form termination that never fires restated over the traced states)"""
    om = po.make_synthetic_model(OBS, ACT, seed=4, learned_rewards=True, reward=None, **mkw)
    spec = to_spec(om, OBS, ACT)
    s0 = (np.random.default_rng(5).standard_normal(OBS) * 0.1).astype(np.float32)
    fused = hipets.HipTrajectoryEvalFn(spec, P, engine=engine, seed=23, mode=mode)
    fn = hipets.ValueTrajectoryEvalFn(spec, P, engine=engine, seed=23, mode=mode)
    assert fn.discount == 1.0 and fn.actor is None and fn.kernel_mode is None
    engine.set_persistent(persistent)
    try:
        for a in cc.call_actions(ACT, pop, H):
            want = fused(s0, a.to(DEV))
            got = fn(s0, a.to(DEV))
            assert fused.calls == fn.calls
            assert torch.isfinite(want).all() and float(want.abs().max()) > 0
            assert torch.equal(got, want), f"max diff {(got - want).abs().max():.3e}"
    finally:
        engine.set_persistent(True)


@pytest.mark.parametrize("name,mkw,pop,P,H", SHAPES, ids=SHAPE_IDS)
def test_without_discount_and_agent_a_terminating_model_gives_the_fused_bits(engine, name, mkw, pop, P, H):
    """the same with a closed-form reward and hopper's termination firing along the horizon; the rollout instance is pinned for both
    (generic_kernel=2), as tests/test_gpu_callable_objective.py pins it for HipTrajectoryEvalFn.trajectories"""
    om, s0 = cc.make_case(OBS, ACT, dict(termination="hopper", **mkw))
    spec = to_spec(om, OBS, ACT)
    fused = hipets.HipTrajectoryEvalFn(spec, P, engine=engine, seed=cc.SEED)
    fn = hipets.ValueTrajectoryEvalFn(spec, P, engine=engine, seed=cc.SEED)
    fused.rollout_kw = fn.rollout_kw = {"generic_kernel": 2}
    for a in cc.call_actions(ACT, pop, H):
        want = fused(s0, a.to(DEV))
        tr = fn.trajectories(s0, a.to(DEV))
        assert torch.equal(tr["returns"], want), f"max diff {(tr['returns'] - want).abs().max():.3e}"
        ended = tr["dones"].cummax(0).values
        assert 0 < int(ended[-1].sum()) < pop * P and tr["terminal_values"] is None


def _terminal_reference(sac, last_obs, target=False):
    """(float64 min(Q1, Q2) at the actor's float64 mean action, u of torch CPU's float32 chain) on `last_obs` numpy [B, obs]"""
    pw, cw = policy_weights(sac.policy), critic_weights(sac.critic_target if target else sac.critic)
    a64 = pr.actor_f64(pw, last_obs)[0]
    v64 = np.minimum(*vr.critic_f64(cw, last_obs, a64))
    a32 = pr.actor_f32(pw, last_obs)[0]
    v32 = np.minimum(*vr.critic_f32_torch(cw, last_obs, a32))
    return v64, float(pr.t1_share(v32, v64).max())


@pytest.mark.parametrize("name,mkw,pop,P,H", SHAPES, ids=SHAPE_IDS)
def test_with_a_critic_returns_are_the_restatement_of_the_calls_own_trajectory(engine, name, mkw, pop, P, H):
    om, s0 = cc.make_case(OBS, ACT, dict(termination="hopper", **mkw))
    torch.manual_seed(3)
    sac = TinySAC(OBS, ACT, 32, device=DEV)
    with torch.no_grad():  # (a target that differs from the critic)
        for p in sac.critic_target.parameters():
            p.mul_(1.25)
    for target in (False, True):
        fn = hipets.ValueTrajectoryEvalFn(to_spec(om, OBS, ACT), P, agent=sac, discount=0.97, target_critic=target, engine=engine, seed=cc.SEED)
        actions = cc.call_actions(ACT, pop, H)[0].to(DEV)
        tr = fn.trajectories(s0, actions)
        assert fn.calls == 1 and tuple(tr["terminal_actions"].shape) == (pop * P, ACT) and tuple(tr["terminal_values"].shape) == (pop * P,)
        rew, dones, tv = tr["rewards"].cpu().numpy(), tr["dones"].cpu().numpy(), tr["terminal_values"].cpu().numpy()
        ended = dones.any(axis=0)
        print(f"{name}: {int(ended.sum())} rows terminated, {int((~ended).sum())} did not")
        assert int(ended.sum()) > 0 and int((~ended).sum()) > 0
        want = vr.discounted_returns_np(rew, dones, pop, P, 0.97, tv)
        assert same_bits(tr["row_totals"].cpu().numpy(), want[1]) and same_bits(tr["returns"].cpu().numpy(), want[0])
        assert np.array_equal(tr["first_done"].cpu().numpy(), want[2])
        plain = vr.discounted_returns_np(rew, dones, pop, P, 0.97, None)
        assert np.array_equal(want[1][ended], plain[1][ended]) and not np.array_equal(want[1][~ended], plain[1][~ended])  # the bootstrap is there
        v64, u = _terminal_reference(sac, tr["next_obs"][-1].cpu().numpy(), target)
        assert_within(tr["terminal_values"], v64, u, f"terminal values ({'target' if target else 'critic'})")
        # __call__ returns what trajectories() returns for the same stream
        again = hipets.ValueTrajectoryEvalFn(to_spec(om, OBS, ACT), P, agent=sac, discount=0.97, target_critic=target, engine=engine, seed=cc.SEED)
        assert torch.equal(again(s0, actions), tr["returns"])


def _sac_batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(state=torch.randn(B, OBS, generator=g), action=torch.rand(B, ACT, generator=g) * 2 - 1, next_state=torch.randn(B, OBS, generator=g),
                reward=torch.randn(B, generator=g), terminated=(torch.rand(B, generator=g) < 0.2).float())


def test_the_objective_follows_the_live_agent(engine):
    """after one SACUpdater.update_parameters (its kernels write through raw pointers: no version moves) and, separately, after ONE stock
    critic_optim.step(), the next call's terminal values are the LIVE weights', and the weights from before no longer explain them"""
    name, mkw, pop, P, H = SHAPES[0]
    om, s0 = cc.make_case(OBS, ACT, dict(termination="hopper", **mkw))
    torch.manual_seed(5)
    sac = TinySAC(OBS, ACT, 32, device=DEV)
    fn = hipets.ValueTrajectoryEvalFn(to_spec(om, OBS, ACT), P, agent=sac, discount=0.97, engine=engine, seed=cc.SEED)
    actions = cc.call_actions(ACT, pop, H)[0].to(DEV)

    def call_and_check(what, old, factor=100):
        tr = fn.trajectories(s0, actions)
        last = tr["next_obs"][-1].cpu().numpy()
        v64, u = _terminal_reference(sac, last)
        assert_within(tr["terminal_values"], v64, u, what)
        if old is not None:  # the snapshot from before would be off by far more than the rule allows
            pw, cw = old
            v_old = np.minimum(*vr.critic_f64(cw, last, pr.actor_f64(pw, last)[0]))
            off = np.abs(v_old - v64) > factor * vr.allowance(v64, u)
            print(f"  {what}: the weights from before are off by {np.median(np.abs(v_old - v64) / vr.allowance(v64, u)):.0f} allowances (median)")
            assert off.mean() > 0.9, f"{what}: the update moved the values on {off.mean():.0%} of the rows only"
            assert (pr.t1_share(tr["terminal_values"].cpu().numpy(), v_old) > factor * vr.bound_factor(u)).mean() > 0.9
        return policy_weights(sac.policy), critic_weights(sac.critic)

    old = call_and_check("fresh agent", None)
    updater = hipets.SACUpdater(sac, engine=engine)
    versions = [int(p._version) for p in sac.critic.parameters()]
    updater.update_parameters(FixedMemory([_sac_batch(64, 1)]), 64, 0, reverse_mask=True)
    assert versions == [int(p._version) for p in sac.critic.parameters()]  # (what makes the counter necessary)
    old = call_and_check("after SACUpdater.update_parameters", old)
    b = _sac_batch(64, 2)
    q1, q2 = sac.critic(b["state"].to(DEV), b["action"].to(DEV))
    sac.critic_optim.zero_grad()
    ((q1 - 1.0).square().mean() + (q2 + 1.0).square().mean()).backward()
    sac.critic_optim.step()  # ONE stock step: it moves the parameters' versions, and the values by about lr = 3e-4 per parameter
    old = call_and_check("after one critic_optim.step()", old, factor=1)  # (differs: the old weights miss the rule itself)
    # another owner in the engine's slots: the next call takes them back
    other = TinySAC(OBS, ACT, 32, device=DEV)
    hipets.SACCritic(other, engine=engine)
    hipets.SACActor(other, engine=engine)
    call_and_check("after another agent used the engine", None)
    # an explicit refresh exists
    with torch.no_grad():
        sac.critic.linear3.bias.data += 0.25  # (.data: no version moves)
        sac.critic.linear6.bias.data += 0.25
    fn.refresh_agent()
    call_and_check("after refresh_agent()", None)


def test_a_target_critic_follows_the_stock_soft_update(engine):
    """target_critic=True under STOCK training: the agent writes its target as ``target_param.data.copy_(...)``
    (pytorch_sac_pranz24/utils.py:28), which moves no version of the target's parameters -- the objective sees the critic_optim.step()
    that precedes every such write, and the next call's terminal values are the live target's"""
    name, mkw, pop, P, H = SHAPES[0]
    om, s0 = cc.make_case(OBS, ACT, dict(termination="hopper", **mkw))
    torch.manual_seed(11)
    sac = TinySAC(OBS, ACT, 32, device=DEV)
    fn = hipets.ValueTrajectoryEvalFn(to_spec(om, OBS, ACT), P, agent=sac, discount=0.97, target_critic=True, engine=engine, seed=cc.SEED)
    assert fn.critic.critic is sac.critic_target
    actions = cc.call_actions(ACT, pop, H)[0].to(DEV)
    tr = fn.trajectories(s0, actions)
    v64, u = _terminal_reference(sac, tr["next_obs"][-1].cpu().numpy(), True)
    assert_within(tr["terminal_values"], v64, u, "fresh target")
    before = critic_weights(sac.critic_target)
    # sac.py:76-173 as far as the critic goes: a loss, critic_optim.step(), then utils.soft_update (tau = 0.5 to move the target far)
    b = _sac_batch(64, 3)
    q1, q2 = sac.critic(b["state"].to(DEV), b["action"].to(DEV))
    sac.critic_optim.zero_grad()
    ((q1 - 1.0).square().mean() + (q2 + 1.0).square().mean()).backward()
    sac.critic_optim.step()
    with torch.no_grad():  # (the critic itself moved by ~lr per parameter: scale it so that half of it is a visible move of the target)
        for p in sac.critic.parameters():
            p.data.mul_(1.5)
    versions = [int(p._version) for p in sac.critic_target.parameters()]
    for target_param, param in zip(sac.critic_target.parameters(), sac.critic.parameters()):
        target_param.data.copy_(target_param.data * 0.5 + param.data * 0.5)
    assert versions == [int(p._version) for p in sac.critic_target.parameters()]  # (what makes watching the live critic necessary)
    tr = fn.trajectories(s0, actions)
    last = tr["next_obs"][-1].cpu().numpy()
    v64, u = _terminal_reference(sac, last, True)
    assert_within(tr["terminal_values"], v64, u, "target after the stock soft update")
    v_old = np.minimum(*vr.critic_f64(before, last, pr.actor_f64(policy_weights(sac.policy), last)[0]))
    assert (np.abs(v_old - v64) > 100 * vr.allowance(v64, u)).mean() > 0.9  # the snapshot from before would be far off


def test_cem_calls_it_once_per_iteration(engine):
    name, mkw, pop, P, H = SHAPES[0]
    iters = 4
    om, s0 = cc.make_case(OBS, ACT, dict(termination="hopper", **mkw))
    torch.manual_seed(7)
    sac = TinySAC(OBS, ACT, 32, device=DEV)
    fn = hipets.ValueTrajectoryEvalFn(to_spec(om, OBS, ACT), P, agent=sac, discount=0.97, engine=engine, seed=3)
    opt = hipets.CEMOptimizer(iters, 0.1, 50, [[-1.0] * ACT] * H, [[1.0] * ACT] * H, 0.1, DEV, return_mean_elites=True, seed=7)
    plan = opt.optimize(_BoundObjective(fn, s0), x0=torch.zeros(H, ACT))
    assert torch.isfinite(plan).all() and tuple(plan.shape) == (H, ACT) and fn.calls == iters


def test_an_agent_acts_on_make_eval_fns_objective(engine):
    name, mkw, pop, P, H = SHAPES[0]
    om, s0 = cc.make_case(OBS, ACT, dict(termination="hopper", **mkw))
    torch.manual_seed(9)
    sac = TinySAC(OBS, ACT, 32, device=DEV)
    fn = hipets.make_eval_fn(to_spec(om, OBS, ACT), P, engine=engine, terminal_value=sac, discount=0.97, seed=2)
    assert type(fn) is hipets.ValueTrajectoryEvalFn and fn.discount == 0.97 and fn.critic.critic is sac.critic
    cfg = dict(_target_="hipets.CEMOptimizer", num_iterations=3, elite_ratio=0.1, population_size=50, alpha=0.1, device=DEV,
               lower_bound="???", upper_bound="???", return_mean_elites=True, seed=3)
    agent = hipets.TrajectoryOptimizerAgent(cfg, [-1.0] * ACT, [1.0] * ACT, planning_horizon=H)
    agent.set_trajectory_eval_fn(fn)
    a = agent.act(s0)
    assert a.shape == (ACT,) and np.isfinite(a).all() and (np.abs(a) <= 1.0).all() and fn.calls == 3
    with pytest.raises(ValueError, match="in-kernel randomness"):
        hipets.BatchedCEMAgent(fn, 2, [-1.0] * ACT, [1.0] * ACT, H, 2, 0.1, 10, 0.1)


def test_the_terminal_value_decides_between_two_candidates(engine):
    """tests/test_gpu_closed_loop.py's point mass (start 1.0, reward -0.001 pos^2) and a hand-built critic worth c |pos|: the plain
    objective prefers the candidate that ends near 0, the value objective the one that stays at 1 -- by a margin, computed from the float64
    restatement over the call's own trajectory, of at least 100 times what the rule allows the terminal values to be off"""
    import test_gpu_closed_loop as cl

    torch.manual_seed(12345)
    rng = np.random.default_rng(12345)
    o, a, nx = cl.collect_random(cl.MockLineEnv(), 600, rng)
    ws, bs, mn, mx, nmean, nstd = cl.train_ensemble(o, a, nx)
    spec = hipets.ModelSpec(reward="none", termination="no_termination", weights=ws, biases=bs, obs_dim=2, act_dim=1, min_logvar=mn,
                            max_logvar=mx, norm_mean=nmean, norm_std=nstd, activation="silu", propagation="random_model")
    c, gamma, H, P = 1.0, 0.97, 5, 5
    critic = TinyQNetwork(2, 1, 16)
    with torch.no_grad():
        for p in critic.parameters():
            p.zero_()
        for j in (1, 4):  # relu(x) + relu(-x) = |x| of obs[0], times c
            getattr(critic, f"linear{j}").weight[0, 0], getattr(critic, f"linear{j}").weight[1, 0] = 1.0, -1.0
            getattr(critic, f"linear{j + 1}").weight[0, 0], getattr(critic, f"linear{j + 1}").weight[1, 1] = 1.0, 1.0
            getattr(critic, f"linear{j + 2}").weight[0, :2] = c
    torch.manual_seed(1)
    agent = SimpleNamespace(policy=TinyGaussianPolicy(2, 1, 16).to(DEV), critic=critic.to(DEV))
    s0 = np.array([1.0, 0.0], np.float32)
    plans = torch.tensor([[-0.5, 0.0, 0.5, 0.0, 0.0], [0.0] * 5]).unsqueeze(-1).to(DEV)  # 0: to the origin and stop; 1: stay at 1
    plain = hipets.CallableTrajectoryEvalFn(spec, P, reward_fn=cl.mock_reward_fn, engine=engine, seed=1)
    fn = hipets.ValueTrajectoryEvalFn(spec, P, agent=agent, discount=gamma, reward_fn=cl.mock_reward_fn, engine=engine, seed=1)
    v_plain = plain(s0, plans).cpu().numpy()
    tr = fn.trajectories(s0, plans)
    v_value = tr["returns"].cpu().numpy()
    last = tr["next_obs"][-1].cpu().numpy()
    print(f"final positions {last[:, 0].reshape(2, P).mean(1)}, plain returns {v_plain}, value returns {v_value}")
    assert abs(last[:P, 0]).max() < 0.5 < abs(last[P:, 0]).min()  # the model has learned the task well enough
    assert v_plain[0] > v_plain[1] and v_value[1] > v_value[0]
    # the margin in float64 against the rule's allowance on the terminal values, both from the call's own trajectory
    cw = critic_weights(critic)
    acts = tr["terminal_actions"].cpu().numpy()
    v64 = np.minimum(*vr.critic_f64(cw, last, acts))
    assert np.allclose(v64, c * np.abs(last[:, 0].astype(np.float64)), rtol=0, atol=1e-12)
    u = float(pr.t1_share(np.minimum(*vr.critic_f32_torch(cw, last, acts)), v64).max())
    ret64, _ = vr.discounted_returns_f64(tr["rewards"].cpu().numpy(), tr["dones"].cpu().numpy(), 2, P, gamma, v64)
    allowed = float((gamma ** H * vr.allowance(v64, u)).max())
    print(f"float64 margin {ret64[1] - ret64[0]:.4f}, allowance {allowed:.3e}")
    assert ret64[1] - ret64[0] >= 100 * allowed
    assert_within(tr["terminal_values"], v64, u, "terminal values")
