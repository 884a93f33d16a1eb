"""hipets.CallableTrajectoryEvalFn's host side without a GPU: the one-launch objective for Python reward / termination callables on a
CPU stand-in of the engine that records the rollout's arguments, fills the two trace tensors from a numpy rule and reduces with the
numpy restatement of hipets_trajectory_returns (tests/returns_restatement.py)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import callable_cases as cc
import hipets
from conftest import to_spec
from hipets.objectives import UnfusedTrajectoryEvalFn, _BoundObjective
from hipets.optimizers import _PlanOptimizer
from oracle import pets_oracle as po
from returns_restatement import same_bits, trajectory_returns_np
from test_host_logic import _FakeModelEnv

OBS, ACT, POP, P, H = 4, 2, 6, 5, 3
B = POP * P


def trace_rule(t, row, d, a_sum):
    """next_obs[t][row][d] of the stand-in: a different value for every (step, row, dim), shifted by the step's action"""
    return np.float32(0.25 * (t + 1) + 0.01 * row + 0.001 * d) + a_sum


class CpuEngine:
    """Engine.set_model / rollout / trajectory_returns on the CPU (host-logic tests only)."""

    device = torch.device("cpu")

    def __init__(self):
        self.spec, self.rollouts = None, []

    def set_model(self, spec):
        self.spec = spec

    def rollout(self, actions, s0, num_particles, *, trace_next_obs=None, trace_rewards=None, **kw):
        pop, horizon, _ = actions.shape
        self.rollouts.append(dict(kw, pop=pop, H=horizon, P=num_particles, next_obs=trace_next_obs, rewards=trace_rewards))
        a = actions.numpy()
        for t in range(horizon):
            for row in range(pop * num_particles):
                a_sum = a[row // num_particles, t].sum()
                for d in range(self.spec.obs_dim):
                    trace_next_obs[t, row, d] = float(trace_rule(t, row, d, a_sum))
                trace_rewards[t, row] = 100.0 * t + row  # "the kernel's own reward"
        return torch.zeros(pop)

    def trajectory_returns(self, rewards, dones, pop, num_particles, *, row_totals=False, first_done=False):
        assert rewards.dtype == torch.float32 and rewards.is_contiguous() and dones.is_contiguous()
        assert dones.dtype in (torch.bool, torch.uint8) and rewards.shape == dones.shape
        ret, tot, first = (torch.from_numpy(v) for v in trajectory_returns_np(rewards.numpy(), dones.numpy(), pop, num_particles))
        return (ret, tot if row_totals else None, first if first_done else None) if (row_totals or first_done) else ret


def spec(members=5, **kw):
    om = po.make_synthetic_model(OBS, ACT, ensemble_size=members, hid=8, seed=0, **kw)
    return to_spec(om, OBS, ACT)


def actions(seed=0, pop=POP, horizon=H):
    return torch.rand(pop, horizon, ACT, generator=torch.Generator().manual_seed(seed)) * 2 - 1


S0 = np.zeros(OBS, np.float32)


def rew_obs0(act, nobs):
    return nobs[:, 0] - 0.1 * act.square().sum(1)


def never(act, nobs):
    return torch.zeros(len(nobs), 1, dtype=torch.bool)


def test_rows_are_time_major_and_one_rollout_feeds_both_callables():
    eng, seen = CpuEngine(), []

    def rew(act, nobs):
        seen.append((act.clone(), nobs.clone()))
        return rew_obs0(act, nobs)

    fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew, termination_fn=never, engine=eng, seed=11, check_rowwise=False)
    a = actions()
    out = fn(S0, a)
    assert len(eng.rollouts) == 1 and len(seen) == 1  # one launch, one call of the callable over all H * B rows
    r = eng.rollouts[0]
    assert (r["mode"], r["seed"], r["stream_id"], r["pop"], r["H"], r["P"]) == ("device", 11, 1, POP, H, P)
    assert tuple(r["next_obs"].shape) == (H, B, OBS) and tuple(r["rewards"].shape) == (H, B)
    act_rows, obs_rows = seen[0]
    assert tuple(act_rows.shape) == (H * B, ACT) and tuple(obs_rows.shape) == (H * B, OBS)
    for t in range(H):
        for c in range(POP):
            for p in range(P):
                n = t * B + c * P + p
                assert torch.equal(act_rows[n], a[c, t])
                assert obs_rows[n, 1].item() == trace_rule(t, c * P + p, 1, a[c, t].numpy().sum())
    want, _, _ = trajectory_returns_np(rew_obs0(act_rows, obs_rows).view(H, B).numpy(), np.zeros((H, B), bool), POP, P)
    assert same_bits(out.numpy(), want)
    fn(S0, actions(1))
    assert eng.rollouts[1]["stream_id"] == 2 and eng.rollouts[1]["next_obs"] is r["next_obs"]  # next stream, the same buffers


def test_kernel_rewards_and_closed_form_termination_fill_in_for_missing_callables():
    eng = CpuEngine()
    fn = hipets.CallableTrajectoryEvalFn(spec(), P, termination_fn=never, engine=eng, check_rowwise=False)
    tr = fn.trajectories(S0, actions())
    assert torch.equal(tr["rewards"], eng.rollouts[0]["rewards"])  # reward_fn=None: the tap of the kernel's own reward
    fn = hipets.CallableTrajectoryEvalFn(spec(termination="walker2d"), P, reward_fn=rew_obs0, engine=eng, check_rowwise=False)
    tr = fn.trajectories(S0, actions())
    want = po.term_walker2d(None, tr["next_obs"].view(-1, OBS)).view(H, B)
    assert torch.equal(tr["dones"], want) and 0 < int(want.sum()) < want.numel()
    assert set(tr) == {"next_obs", "rewards", "dones", "first_done", "row_totals", "returns"}
    ret, tot, first = trajectory_returns_np(tr["rewards"].numpy(), want.numpy(), POP, P)
    assert same_bits(tr["returns"].numpy(), ret) and same_bits(tr["row_totals"].numpy(), tot) and np.array_equal(tr["first_done"].numpy(), first)
    with pytest.raises(ValueError, match="HipTrajectoryEvalFn"):
        hipets.CallableTrajectoryEvalFn(spec(), P, engine=eng)


@pytest.mark.parametrize("name", ["cartpole", "inverted_pendulum", "hopper", "walker2d", "ant", "humanoid", "no_termination"])
def test_closed_form_dones_restate_the_termination_functions(name):
    from hipets.objectives import closed_form_dones

    g = torch.Generator().manual_seed(3)
    s = torch.randn(4000, 5, generator=g) * 1.5
    s[::7, 0] += 1.0
    s[5, 3], s[6, 2], s[9, 1] = float("nan"), float("inf"), 150.0
    for thr in (0.7, 0.2, 1.0, 2.0, 0.8, 2.4, -2.4):  # rows ON the float32 thresholds
        s[int(thr * 100) % 97, 0] = thr
        s[int(thr * 100) % 89 + 100, 1] = thr
    got = closed_form_dones(spec(termination=name), s)
    assert torch.equal(got, po.TERMINATION_FNS[name](None, s)[:, 0])


def test_box_termination_dones():
    from hipets.objectives import closed_form_dones

    box = hipets.BoxTermination(intervals=(hipets.Interval(0, lo=0.5, hi=1.5, lo_open=True), hipets.Interval(2, hi=0.0, hi_open=True)), require_finite=True)
    sp = spec()
    sp.termination = box
    s = torch.tensor([[1.0, 0, -1, 0], [0.5, 0, -1, 0], [1.5, 0, -1, 0], [1.0, 0, 0.0, 0], [1.0, float("nan"), -1, 0], [1.0, 0, -1, float("inf")]])
    assert closed_form_dones(sp, s).tolist() == [False, True, False, True, True, True]


def test_output_shapes_and_dtypes():
    eng = CpuEngine()
    outs = []
    for r_shape in ("n", "n1"):
        for d_shape in ("n", "n1"):
            rew = (lambda a, o: rew_obs0(a, o)) if r_shape == "n" else (lambda a, o: rew_obs0(a, o).unsqueeze(1))
            term = (lambda a, o: o[:, 0] > 0.6) if d_shape == "n" else (lambda a, o: (o[:, 0] > 0.6).unsqueeze(1))
            outs.append(hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew, termination_fn=term, engine=eng)(S0, actions()))
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    bad = [(lambda a, o: o[:, :2], never, r"reward_fn.*\(90, 2\)"),
           (lambda a, o: o[:5, 0], never, r"reward_fn.*\(5,\)"),
           (lambda a, o: (o[:, 0] > 0).long(), never, r"reward_fn.*torch.int64"),
           (lambda a, o: o[:, 0].numpy(), never, r"reward_fn.*ndarray"),
           (rew_obs0, lambda a, o: (o[:, 0] > 0).float(), r"termination_fn.*torch.float32"),
           (rew_obs0, lambda a, o: o[:, :2] > 0, r"termination_fn.*\(90, 2\)")]
    for rew, term, msg in bad:
        fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew, termination_fn=term, engine=eng, check_rowwise=False)
        with pytest.raises(ValueError, match=msg):
            fn(S0, actions())


def test_rowwise_check_runs_on_the_first_call_only():
    eng = CpuEngine()
    fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=lambda a, o: o[:, 0] - o[:, 0].mean(), termination_fn=never, engine=eng)
    with pytest.raises(ValueError, match="not row-wise.*UnfusedTrajectoryEvalFn"):
        fn(S0, actions())
    fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew_obs0, termination_fn=lambda a, o: o[:, 1].flip(0) > 0.6, engine=eng)
    with pytest.raises(ValueError, match="termination_fn is not row-wise"):
        fn(S0, actions())
    sizes = []

    def rew(act, nobs):  # row-wise, with a NaN in every call's first row: NaNs at equal positions are equal
        sizes.append(len(nobs))
        out = rew_obs0(act, nobs)
        out[0] = float("nan")
        return out

    fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew, termination_fn=never, engine=eng)
    fn(S0, actions())
    assert sizes == [H * B, B]  # the batched call, then step 0's rows alone
    fn(S0, actions(1))
    assert sizes == [H * B, B, H * B]  # not checked again
    unchecked = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=lambda a, o: o[:, 0] - o[:, 0].mean(), termination_fn=never, engine=eng,
                                                check_rowwise=False)
    unchecked(S0, actions())


def test_max_trajectory_bytes():
    eng = CpuEngine()
    need = H * B * (OBS + 1) * 4
    fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew_obs0, termination_fn=never, engine=eng, max_trajectory_bytes=need)
    fn(S0, actions())
    fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew_obs0, termination_fn=never, engine=eng, max_trajectory_bytes=need - 1)
    with pytest.raises(ValueError, match=f"{need} bytes.*max_trajectory_bytes = {need - 1}"):
        fn(S0, actions())
    assert len(eng.rollouts) == 1  # refused before anything was launched
    assert hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew_obs0, engine=eng).max_trajectory_bytes == 2 * 1024**3


def test_make_eval_fn_routes_custom_callables():
    def my_reward(act, nobs):
        return nobs[:, :1]

    me = _FakeModelEnv()
    me.reward_fn = my_reward
    eng = CpuEngine()
    steps = hipets.make_eval_fn(me, 5, engine=eng)
    assert type(steps) is UnfusedTrajectoryEvalFn and type(hipets.make_eval_fn(me, 5, engine=eng, callables="steps")) is UnfusedTrajectoryEvalFn
    fn = hipets.make_eval_fn(me, 5, engine=eng, callables="trajectory", mode="fast", seed=4)
    assert type(fn) is hipets.CallableTrajectoryEvalFn and fn.reward_fn is my_reward and fn.termination_fn is None
    assert (fn.mode, fn.seed, fn.num_particles) == ("fast", 4, 5)
    with pytest.raises(ValueError, match="callables must be 'steps' or 'trajectory'"):
        hipets.make_eval_fn(me, 5, engine=eng, callables="fused")
    closed = hipets.make_eval_fn(_FakeModelEnv(), 5, engine=eng, callables="trajectory")  # closed forms: the fused objective either way
    assert type(closed) is hipets.HipTrajectoryEvalFn


def test_the_new_objective_is_not_a_fused_plan_target():
    eng = CpuEngine()
    fn = hipets.CallableTrajectoryEvalFn(spec(), P, reward_fn=rew_obs0, engine=eng, seed=5)
    opt = SimpleNamespace(sampler="philox", engine=eng, seed=9)
    assert _PlanOptimizer._fused_objective(opt, _BoundObjective(fn, S0)) == (None, 9)
    assert _PlanOptimizer._fused_objective(opt, _BoundObjective(fn, S0), planet_ok=True) == (None, 9)
    fused = hipets.HipTrajectoryEvalFn(spec(), P, engine=eng, seed=5)  # ... while the fused objective next to it is one
    assert _PlanOptimizer._fused_objective(opt, _BoundObjective(fused, S0)) == (fused, 9 ^ 5)
    assert fn.kernel_mode is None and not isinstance(fn, hipets.HipTrajectoryEvalFn)
    with pytest.raises(ValueError, match="in-kernel randomness"):  # batched agents refuse it
        hipets.BatchedCEMAgent(fn, 2, [-1.0] * ACT, [1.0] * ACT, H, 2, 0.1, 10, 0.1)


def test_return_chain_on_hand_made_cases():
    nan, inf = np.float32("nan"), np.float32("inf")
    rewards = np.array([[1.0, 1.0, 1.0, 1.0, 0.1, 1.0],
                        [2.0, nan, nan, 2.0, 0.2, -inf],
                        [4.0, inf, 4.0, 4.0, 0.3, 4.0]], np.float32)  # [H = 3, B = 6]
    dones = np.array([[0, 1, 0, 0, 0, 1],
                      [0, 0, 1, 1, 0, 1],
                      [0, 0, 0, 1, 1, 0]], np.uint8)
    ret, tot, first = trajectory_returns_np(rewards, dones, 3, 2)
    # row 1 ends at t = 0: its own reward counts, the NaN and the inf behind it add exactly 0; row 2's NaN comes WITH its terminating
    # step, i.e. before the mask: it propagates; row 3: the terminating step's reward counts, the next does not
    assert tot[0] == 7.0 and tot[1] == 1.0 and np.isnan(tot[2]) and tot[3] == 3.0 and tot[5] == 1.0
    assert tot[4] == np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3))
    assert first.tolist() == [3, 0, 1, 1, 2, 0]
    assert ret[0] == 4.0 and np.isnan(ret[1]) and ret[2] == np.float32(np.float32(tot[4] + tot[5]) / np.float32(2))
    # the particle mean is a sequential float32 sum, not a pairwise or float64 one
    r = np.array([[1e8, 1.0, -1e8, 1.0]], np.float32)
    ret, _, _ = trajectory_returns_np(r, np.zeros((1, 4), np.uint8), 1, 4)
    assert ret[0] == np.float32(0.25)  # ((1e8 + 1) - 1e8) + 1 = 1 in float32; exact arithmetic gives 0.5
    # ... and through the objective: a terminating callable
    eng = CpuEngine()
    fn = hipets.CallableTrajectoryEvalFn(spec(members=3), 2, reward_fn=lambda a, o: torch.from_numpy(rewards).reshape(-1),
                                         termination_fn=lambda a, o: torch.from_numpy(dones).reshape(-1).bool(), engine=eng, check_rowwise=False)
    out = fn(S0, actions(pop=3))
    assert same_bits(out.numpy(), trajectory_returns_np(rewards, dones, 3, 2)[0])


TERMINATING = [c for c in cc.REPLAYS if "termination" in c[3]]  # (the others have no threshold to come near: nothing to choose)


@pytest.mark.parametrize("name,obs,act,mkw,pop,P_,H_,mode", TERMINATING, ids=[c[0] for c in TERMINATING])
def test_replay_seeds_keep_the_oracle_alone_inside_the_cap(name, obs, act, mkw, pop, P_, H_, mode):
    """The GPU replays (tests/test_gpu_callable_objective.py, section C) exclude at most two candidates next to a termination threshold
    and want the termination to fire progressively: both hold for the oracle ALONE at the chosen seeds, with the draws restated on the
    CPU -- for a FAST call at every row-tile count the library may choose."""
    om, s0 = cc.make_case(obs, act, mkw)
    generator = torch.Generator().manual_seed(cc.EXACT_GENERATOR_SEED)
    for call, a in enumerate(cc.call_actions(act, pop, H_), start=1):
        for r in ((1, 2, 3, 4) if mode == "fast" else (1,)):
            draws = cc.exact_draws(to_spec(om, obs, act), pop * P_, H_, call, generator) if mode == "exact" else cc.cpu_draws(om, pop, P_, H_, mode, call, r)
            ref, keep, ended, _ = cc.oracle_replay(om, a, s0, P_, draws)
            assert torch.isfinite(ref).all()
            cc.assert_replay_is_usable(om, keep, ended)
