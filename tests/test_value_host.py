"""hipets.value's host side without a GPU: the restatement of hipets_discounted_returns against the restatement of
hipets_trajectory_returns and against the geometric sum, the refusals of SACCritic / ValueTrajectoryEvalFn / make_eval_fn message by
message, and the objective's evaluation order on the CPU stand-in of the engine (tests/test_callable_objective_host.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import hipets
import value_restatement as vr
from hipets import _pack
from hipets.objectives import _BoundObjective
from hipets.optimizers import _PlanOptimizer
from returns_restatement import same_bits, trajectory_returns_np
from sac_restatement import TinyQNetwork, TinySAC
from test_callable_objective_host import ACT, H, OBS, P, POP, S0, CpuEngine, actions, spec
from test_gpu_callable_objective import REDUCE_SHAPES, reduce_inputs
from test_host_logic import _FakeModelEnv


def _plantable(pop, P_, H_):
    return pop * P_ >= 6 and H_ >= 4  # reduce_inputs(plant=True) writes rows 0 .. 5 and steps 0 .. 3


@pytest.mark.parametrize("pop,P_,H_", REDUCE_SHAPES, ids=[f"pop{a}_P{b}_H{c}" for a, b, c in REDUCE_SHAPES])
def test_gamma_one_without_values_is_the_undiscounted_restatement_bit_for_bit(pop, P_, H_):
    for plant in (False, True) if _plantable(pop, P_, H_) else (False,):
        rewards, dones = reduce_inputs(pop, P_, H_, seed=pop + H_, plant=plant)
        want = trajectory_returns_np(rewards, dones, pop, P_)
        got = vr.discounted_returns_np(rewards, dones, pop, P_, gamma=1.0)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
        if plant:  # NaN / inf behind a termination add exactly 0; at or ahead of one they count
            assert np.isfinite(want[1][:3]).all() and np.isnan(want[1][3]) and np.isinf(want[1][4]) and np.isnan(want[1][5])


@pytest.mark.parametrize("H_", [1, 6, 33])
def test_half_discount_on_constant_rewards_is_the_geometric_sum(H_):
    pop, P_ = 4, 3
    c = np.float32(1.7)
    rewards, dones = np.full((H_, pop * P_), c, np.float32), np.zeros((H_, pop * P_), np.uint8)
    ret, tot, first = vr.discounted_returns_np(rewards, dones, pop, P_, gamma=0.5)
    exact = float(c) * (1.0 - 0.5 ** H_) / 0.5
    # powers of 1/2 and their products with c are exact in float32: only the H - 1 additions round, each by at most half an ulp of a
    # partial sum below 2 c
    assert np.abs(tot.astype(np.float64) - exact).max() <= (H_ - 1) * 2.0 ** -24 * 2 * float(c)
    assert (first == H_).all() and np.allclose(ret, exact, rtol=1e-6)
    # a terminal value arrives discounted by 0.5 ** H, and a terminated row gets none
    dones[H_ - 1, 0] = 1
    values = np.full(pop * P_, 8.0, np.float32)
    _, tot_v, _ = vr.discounted_returns_np(rewards, dones, pop, P_, gamma=0.5, values=values)
    assert tot_v[0] == tot[0] and np.allclose(tot_v[1:], exact + 8.0 * 0.5 ** H_, rtol=1e-6)


def test_f64_chain_agrees_with_the_float32_restatement():
    rewards, dones = reduce_inputs(24, 5, 6, seed=3)
    values = np.random.default_rng(0).standard_normal(120).astype(np.float32)
    ret32, tot32, _ = vr.discounted_returns_np(rewards, dones, 24, 5, gamma=0.97, values=values)
    ret64, tot64 = vr.discounted_returns_f64(rewards, dones, 24, 5, 0.97, values)
    assert np.allclose(tot32, tot64, rtol=1e-5, atol=1e-5) and np.allclose(ret32, ret64, rtol=1e-5, atol=1e-5)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_critic_refusals_message_by_message():
    U = hipets.UnsupportedModelError
    q = TinyQNetwork(5, 2, 16)
    (K, hid), tensors = _pack.pack_critic(q)
    assert (K, hid) == (7, 16) and len(tensors) == 12 and tensors[0] is not q.linear1.weight and tensors[0].data_ptr() == q.linear1.weight.data_ptr()
    assert hipets.value.find_critic(q) is q
    sac = TinySAC(5, 2, 16)
    assert hipets.value.find_critic(sac) is sac.critic and hipets.value.find_critic(sac, target=True) is sac.critic_target
    assert hipets.value.find_critic(SimpleNamespace(sac_agent=sac), target=True) is sac.critic_target
    # layers missing
    with pytest.raises(U, match="has no critic: expected an mbrl SACAgent"):
        hipets.SACCritic(SimpleNamespace(policy=sac.policy))
    with pytest.raises(U, match="has no critic_target"):
        hipets.SACCritic(SimpleNamespace(policy=sac.policy), target=True)
    half = torch.nn.Module()
    half.linear1, half.linear2, half.linear3 = torch.nn.Linear(7, 16), torch.nn.Linear(16, 16), torch.nn.Linear(16, 1)
    with pytest.raises(U, match="not shaped like a QNetwork: no linear4, linear5, linear6"):
        hipets.SACCritic(half)
    no_bias = TinyQNetwork(5, 2, 16)
    no_bias.linear5 = torch.nn.Linear(16, 16, bias=False)
    with pytest.raises(U, match="no linear5 with a weight and a bias"):
        hipets.SACCritic(no_bias)
    # shapes that do not chain
    bad = TinyQNetwork(5, 2, 16)
    bad.linear5 = torch.nn.Linear(15, 16)
    with pytest.raises(U, match=r"do not chain: linear5 is \(16, 15\).*expected \(16, 16\)"):
        hipets.SACCritic(bad)
    bad = TinyQNetwork(5, 2, 16)
    bad.linear6 = torch.nn.Linear(16, 2)
    with pytest.raises(U, match=r"do not chain: linear6 is \(2, 16\)"):
        hipets.SACCritic(bad)
    bad = TinyQNetwork(5, 2, 16)
    bad.linear4 = torch.nn.Linear(8, 16)
    with pytest.raises(U, match=r"do not chain: linear4 is \(16, 8\)"):
        hipets.SACCritic(bad)
    # sizes past the limits
    with pytest.raises(U, match=r"hidden 1025\) outside the critic kernel's"):
        hipets.SACCritic(TinyQNetwork(5, 2, 1025))
    with pytest.raises(U, match=r"obs \+ act 545, hidden 16\) outside"):
        hipets.SACCritic(TinyQNetwork(513, 32, 16))
    with pytest.raises(U, match=r"\(obs 513, act 2\) outside the critic kernel's"):
        hipets.SACCritic(TinyQNetwork(513, 2, 16), obs_dim=513)
    with pytest.raises(U, match=r"\(obs 5, act 33\) outside"):
        hipets.SACCritic(TinyQNetwork(5, 33, 16), obs_dim=5)
    with pytest.raises(U, match=r"\(obs 7, act 0\) outside"):
        hipets.SACCritic(TinyQNetwork(5, 2, 16), obs_dim=7)
    # the split is read off the agent's policy
    with pytest.raises(U, match=r"takes 9 inputs, obs_dim \+ act_dim = 5 \+ 3"):
        _pack.check_critic_split(9, 5, 3)
    with pytest.raises(U, match=r"\(obs 5, act 33\) outside"):
        hipets.SACCritic(SimpleNamespace(policy=sac.policy, critic=TinyQNetwork(5, 33, 16)))


@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), float("inf")])
def test_discount_outside_the_unit_interval_is_refused(bad):
    with pytest.raises(ValueError, match=r"discount must be in \[0, 1\]"):
        hipets.ValueTrajectoryEvalFn(spec(), P, discount=bad, engine=CpuEngine())
    with pytest.raises(ValueError, match=r"discount must be in \[0, 1\]"):
        hipets.make_eval_fn(spec(), P, discount=bad, engine=CpuEngine())
    assert _pack.check_discount(0) == 0.0 and _pack.check_discount(1) == 1.0


def test_a_planet_model_is_refused():
    planet = SimpleNamespace(belief_model=None, prior_transition_model=None, reward_model=None, latent_state_size=4)
    for model in (planet, SimpleNamespace(dynamics_model=planet)):
        with pytest.raises(ValueError, match="not available for PlaNet latent models"):
            hipets.make_eval_fn(model, 1, discount=0.9)
        with pytest.raises(ValueError, match="not available for PlaNet latent models"):
            hipets.make_eval_fn(model, 1, terminal_value=TinySAC(5, 2, 16))
        with pytest.raises(ValueError, match="not available for PlaNet latent models"):
            hipets.ValueTrajectoryEvalFn(model, 1)


def test_make_eval_fn_without_the_new_arguments_returns_the_same_class_as_before():
    eng = CpuEngine()
    assert type(hipets.make_eval_fn(_FakeModelEnv(), 5, engine=eng)) is hipets.HipTrajectoryEvalFn
    assert type(hipets.make_eval_fn(spec(), 5, engine=eng, mode="fast", seed=3)) is hipets.HipTrajectoryEvalFn
    me = _FakeModelEnv()
    me.reward_fn = lambda act, nobs: nobs[:, :1]
    assert type(hipets.make_eval_fn(me, 5, engine=eng)) is hipets.UnfusedTrajectoryEvalFn
    assert type(hipets.make_eval_fn(me, 5, engine=eng, callables="trajectory")) is hipets.CallableTrajectoryEvalFn
    # ... and with any of them, the new objective
    for kw in (dict(discount=0.9), dict(target_critic=False), dict(terminal_value=None)):
        fn = hipets.make_eval_fn(spec(), 5, engine=eng, seed=4, **kw)
        assert type(fn) is hipets.ValueTrajectoryEvalFn and fn.discount == kw.get("discount", 1.0) and fn.actor is None and fn.seed == 4
    fn = hipets.make_eval_fn(me, 5, engine=eng, discount=0.5)  # the model's custom callables travel in the spec
    assert type(fn) is hipets.ValueTrajectoryEvalFn and fn.reward_fn is me.reward_fn


# ---- the objective on the CPU stand-in ---------------------------------------------------------------------------------------------
class CpuValueEngine(CpuEngine):
    def discounted_returns(self, rewards, dones, pop, num_particles, *, gamma=1.0, terminal_values=None, row_totals=False, first_done=False):
        assert rewards.dtype == torch.float32 and rewards.is_contiguous() and dones.is_contiguous() and dones.dtype in (torch.bool, torch.uint8)
        v = None if terminal_values is None else terminal_values.numpy()
        ret, tot, first = (torch.from_numpy(x) for x in vr.discounted_returns_np(rewards.numpy(), dones.numpy(), pop, num_particles, gamma, v))
        return (ret, tot if row_totals else None, first if first_done else None) if (row_totals or first_done) else ret


def test_discounting_alone_on_the_stand_in_engine():
    """agent=None: the kernel's own rewards, the spec's closed-form termination, discounted; discount=1 gives the callable objective's
    returns of the same inputs"""
    eng = CpuValueEngine()
    fn = hipets.ValueTrajectoryEvalFn(spec(), P, discount=0.5, engine=eng, seed=5)
    tr = fn.trajectories(S0, actions())
    assert fn.calls == 1 and eng.rollouts[-1]["stream_id"] == 1 and tr["terminal_values"] is None and tr["terminal_actions"] is None
    want = vr.discounted_returns_np(tr["rewards"].numpy(), tr["dones"].numpy(), POP, P, 0.5)
    assert same_bits(tr["returns"].numpy(), want[0]) and same_bits(tr["row_totals"].numpy(), want[1])
    assert same_bits(fn(S0, actions()).numpy(), want[0]) and fn.calls == 2
    one = hipets.ValueTrajectoryEvalFn(spec(), P, engine=eng, seed=5)
    plain = trajectory_returns_np(tr["rewards"].numpy(), tr["dones"].numpy(), POP, P)[0]
    assert same_bits(one(S0, actions()).numpy(), plain)
    assert tuple(tr["next_obs"].shape) == (H, POP * P, OBS) and tuple(actions().shape) == (POP, H, ACT)


def test_the_value_objective_is_not_a_fused_plan_target():
    eng = CpuValueEngine()
    fn = hipets.ValueTrajectoryEvalFn(spec(), P, discount=0.9, engine=eng, seed=5)
    opt = SimpleNamespace(sampler="philox", engine=eng, seed=9)
    assert _PlanOptimizer._fused_objective(opt, _BoundObjective(fn, S0)) == (None, 9)
    assert fn.kernel_mode is None and not isinstance(fn, hipets.HipTrajectoryEvalFn)
    with pytest.raises(ValueError, match="in-kernel randomness"):  # batched agents refuse it
        hipets.BatchedCEMAgent(fn, 2, [-1.0] * ACT, [1.0] * ACT, H, 2, 0.1, 10, 0.1)


def test_a_target_snapshot_watches_the_live_critic():
    """the stock soft update writes the target through ``.data`` (pytorch_sac_pranz24/utils.py:28): no version of the target's moves, so a
    target's snapshot also watches the live critic, whose optimizer step precedes every such write; the engine's update counter counts too"""
    from hipets.value import _Snapshot

    sac, eng = TinySAC(5, 2, 16), SimpleNamespace(sac_updates=0)
    alone, watching = _Snapshot(sac.critic_target, eng), _Snapshot(sac.critic_target, eng, watch=(sac.critic,))
    q1, q2 = sac.critic(torch.randn(8, 5), torch.randn(8, 2))
    sac.critic_optim.zero_grad()
    (q1.square().mean() + q2.square().mean()).backward()
    sac.critic_optim.step()
    for target_param, param in zip(sac.critic_target.parameters(), sac.critic.parameters()):
        target_param.data.copy_(target_param.data * 0.995 + param.data * 0.005)
    assert not alone.moved() and watching.moved()
    watching.mark()
    assert not watching.moved()
    eng.sac_updates += 1
    assert alone.moved() and watching.moved()
    assert _Snapshot(sac.critic, eng, watch=(sac.critic, None)).modules == (sac.critic,)
