"""tests/policy_rollout_restatement.py against the reference's own GaussianPolicy + ModelEnv.step(sample=False) (recorded by
tests/make_policy_rollout_golden.py), and the argument checking of PolicyPrior / extra_candidates that needs no engine.

Bit equality: the float32 restatement goes through torch's own CPU kernels for everything that has more than one valid float32 answer
(F.linear, matmul, exp, tanh, the activation modules, mean(dim=0)), in the reference's op order; what is left to numpy is one correctly
rounded operation per element (the normaliser's subtraction and division in its own dtype, the additions of the delta rule, the
selects).  Every step is therefore bit-equal to the recording -- actions, members' means, states -- and asserted so; the share of T1
is printed beside it."""
import os
import re

import numpy as np
import pytest
import torch

import ensemble_restatement as er
import policy_rollout_restatement as rr
from conftest import ROOT

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "policy_rollout_cases.npz"))
CASES = {
    "elite": dict(activation="silu", normalizer="f64", elites=[2, 0], learned=True, rule=dict(target_is_delta=True, no_delta_list=[0])),
    "absolute": dict(activation="silu", normalizer="none", elites=None, learned=False, rule=dict(target_is_delta=False)),
    "basic": dict(activation="tanh", normalizer="none", elites=None, learned=False, rule=dict(target_is_delta=True)),
}


def golden_case(key):
    c = CASES[key]
    n = sum(1 for k in GOLDEN.files if re.fullmatch(key + r"_w\d+", k))
    ws, bs = [GOLDEN[f"{key}_w{i}"] for i in range(n)], [GOLDEN[f"{key}_b{i}"] for i in range(n)]
    obs_dim = GOLDEN[f"{key}_s0"].shape[1]
    case = dict(E=ws[0].shape[0], weights=ws, biases=bs, deterministic=False, out_dim=ws[-1].shape[2] // 2, slope=0.01, columns=None,
                activation=c["activation"], normalizer=c["normalizer"], elites=c["elites"], min_logvar=GOLDEN[f"{key}_min_logvar"],
                max_logvar=GOLDEN[f"{key}_max_logvar"])
    if c["normalizer"] != "none":
        case.update(norm_mean=GOLDEN[f"{key}_norm_mean"], norm_std=GOLDEN[f"{key}_norm_std"])
    w = {k[len(key) + 7:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(key + "_actor_")}
    assert case["out_dim"] == obs_dim + (1 if c["learned"] else 0)
    return case, w, rr.delta_rule(obs_dim, **c["rule"])


def _same(got, want, what):
    share = er.t1_share(got, want).max()
    equal = np.array_equal(np.asarray(got, np.float32).view(np.int32), np.asarray(want, np.float32).view(np.int32))
    print(f"{what}: max share of T1 {share:.3g}, bit-equal {equal}")
    assert share <= 1.0, (what, share)
    return equal


@pytest.mark.parametrize("key", list(CASES))
def test_float32_restatement_equals_the_reference_rollout(key):
    case, w, rule = golden_case(key)
    s0, eps = GOLDEN[f"{key}_s0"], GOLDEN[f"{key}_eps"]
    H = eps.shape[0]
    actions, states = rr.rollout_f32(case, w, s0, H, eps, 1, True, rule)
    assert actions.dtype == np.float32 and states.dtype == np.float32
    equal = [_same(actions, GOLDEN[f"{key}_actions"], f"{key} actions"), _same(states, GOLDEN[f"{key}_states"], f"{key} states")]
    # per step from the RECORDED states: the members' means, then the composition
    for t in range(H):
        a, nxt, means = rr.step_f32(case, w, GOLDEN[f"{key}_states"][t], eps[t], 1, True, rule, member_means=True)
        equal.append(_same(means[..., :case["out_dim"]], GOLDEN[f"{key}_member_means"][t], f"{key} step {t} members' means"))
        equal.append(_same(nxt, GOLDEN[f"{key}_states"][t + 1], f"{key} step {t} next state"))
    assert all(equal), f"{key}: the float32 restatement left the reference's bits"


@pytest.mark.parametrize("key", list(CASES))
def test_float64_restatement_stays_within_the_bound(key):
    case, w, rule = golden_case(key)
    eps = GOLDEN[f"{key}_eps"]
    for t in range(eps.shape[0]):
        s = GOLDEN[f"{key}_states"][t]
        a64, s64 = rr.step_f64(case, w, s, eps[t], 1, True, rule)
        a32, s32 = rr.step_f32(case, w, s, eps[t], 1, True, rule)
        fa, fs = er.bound_factor(a32, a64), er.bound_factor(s32, s64)
        sa, ss = er.t1_share(GOLDEN[f"{key}_actions"][:, t], a64).max(), er.t1_share(GOLDEN[f"{key}_states"][t + 1], s64).max()
        print(f"{key} step {t}: reference actions {sa:.3f} of T1 (bound {fa:.2f}), next states {ss:.3f} of T1 (bound {fs:.2f})")
        assert sa <= fa and ss <= fs


@pytest.mark.parametrize("key", list(CASES))
def test_compose_np_is_the_restatements_last_stage(key):
    """on the same members' means: sequential float32 adds and one division give torch's mean(dim=0) for these member counts (2 and 3:
    torch sums them in order too), and the delta rule is the same additions"""
    case, w, rule = golden_case(key)
    eps = GOLDEN[f"{key}_eps"]
    for t in range(eps.shape[0]):
        s = GOLDEN[f"{key}_states"][t]
        _, nxt, means = rr.step_f32(case, w, s, eps[t], 1, True, rule, member_means=True)
        got = rr.compose_np(s, means, rule)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), nxt.view(np.int32))


def test_compose_np_on_hand_computed_rows():
    s = np.array([[1.0, 2.0, 3.0]], np.float32)
    means = np.array([[[0.5, 1.0, -1.0, 9.0]], [[1.5, 3.0, 1.0, 7.0]]], np.float32)  # (the last column: a learned reward)
    assert np.array_equal(rr.compose_np(s, means, rr.delta_rule(3)), [[2.0, 4.0, 3.0]])
    assert np.array_equal(rr.compose_np(s, means, rr.delta_rule(3, True, [0, 2])), [[1.0, 4.0, 0.0]])
    assert np.array_equal(rr.compose_np(s, means, rr.delta_rule(3, False)), [[1.0, 2.0, 0.0]])
    nan = rr.compose_np(np.array([[np.nan, 0.0, np.inf]], np.float32), means, rr.delta_rule(3))
    assert np.isnan(nan[0, 0]) and nan[0, 1] == 2.0 and np.isinf(nan[0, 2])


def test_new_symbols_are_declared():
    from hipets import _lib

    assert [n for n, _ in _lib.SYMBOLS["hipets_policy_rollout"][1]] == ["e", "s0", "n", "horizon", "mean_rows", "only_elite", "seed", "stream_id",
                                                                        "eps", "actions", "states", "stream"]
    assert [n for n, _ in _lib.SYMBOLS["hipets_policy_rollout_geometry"][1]] == ["e", "n", "row_tiles", "lds_bytes"]


def test_lds_rule_as_a_function():
    from hipets._pack import ensemble_lds_bytes, policy_rollout_lds_bytes

    # mbpo_halfcheetah's pair: the actor's two 516-float buffers decide; two row tiles fit, four do not
    assert policy_rollout_lds_bytes(17, 6, 512, 23, 200, 18, False, 5) == 64 * (36 + 8 + 2 * 516)
    assert policy_rollout_lds_bytes(17, 6, 512, 23, 200, 18, False, 5, 2) <= 160 * 1024 < policy_rollout_lds_bytes(17, 6, 512, 23, 200, 18, False, 5, 4)
    # a narrow actor: the model's areas decide (the ensemble kernel's need less one of its two accumulators)
    assert policy_rollout_lds_bytes(17, 6, 16, 23, 200, 18, False, 5) == 64 * (36 + 8) + ensemble_lds_bytes(23, 200, 18, False, 5) - 64 * 18
    # humanoid's model under a 1024-wide actor: one row tile, inside the 160 KiB of a gfx950 workgroup
    assert 152 * 1024 < policy_rollout_lds_bytes(376, 17, 1024, 393, 200, 377, False, 5) <= 160 * 1024


def test_policy_prior_refuses_bad_counts_before_it_reads_anything():
    import hipets

    for kw, word in ((dict(num=0), "num"), (dict(num=2.5), "num"), (dict(num=True), "num"), (dict(num=4, mean_rows=5), "mean_rows"),
                     (dict(num=4, mean_rows=-1), "mean_rows")):
        with pytest.raises(ValueError, match=word):
            hipets.PolicyPrior(None, None, **kw)


def test_agent_seam_argument_checking():
    """what the agent layer refuses without touching an engine: a prior without `sequences`, a PlaNet objective under a prior, the
    batched agents"""
    import hipets
    from hipets import agents

    agent = agents.TrajectoryOptimizerAgent.__new__(agents.TrajectoryOptimizerAgent)
    agent.trajectory_eval_fn, agent.policy_prior = None, None
    with pytest.raises(TypeError, match="sequences"):
        agent.set_policy_prior(object())
    prior = type("Prior", (), {"sequences": lambda self, obs, horizon: None})()
    agent.set_policy_prior(prior)
    assert agent.policy_prior is prior
    planet = hipets.PlaNetTrajectoryEvalFn.__new__(hipets.PlaNetTrajectoryEvalFn)
    with pytest.raises(ValueError, match="latent"):
        agent.set_trajectory_eval_fn(planet)
    agent.set_policy_prior(None)
    agent.set_trajectory_eval_fn(planet)
    with pytest.raises(ValueError, match="latent"):
        agent.set_policy_prior(prior)
    batched = agents.BatchedCEMAgent.__new__(agents.BatchedCEMAgent)
    with pytest.raises(NotImplementedError, match="TrajectoryOptimizerAgent"):
        batched.set_policy_prior(prior)
    with pytest.raises(ValueError, match="extra_candidates"):
        batched.plan(np.zeros((1, 3), np.float32), extra_candidates=torch.zeros(1, 2, 2))
    with pytest.raises(ValueError, match="extra_candidates"):
        batched.act(np.zeros((1, 3), np.float32), extra_candidates=torch.zeros(1, 2, 2))


def test_whole_plan_rule_counts_extra_candidates():
    from hipets.optimizers import _PlanOptimizer

    fused = object()
    assert _PlanOptimizer._whole_plan(fused, None, None, {})
    assert _PlanOptimizer._whole_plan(fused, None, None, {"extra_candidates": None})
    assert not _PlanOptimizer._whole_plan(fused, None, None, {"extra_candidates": torch.zeros(1, 2, 2)})
