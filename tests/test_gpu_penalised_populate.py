"""hipets.rollout_model_and_populate_sac_buffer(..., uncertainty=...) on the GPU: penalised model rollouts into the SAC buffer.

The trajectories of a populate call do not depend on the penalty (the model steps every row, done or not, and the actor sees
observations only), so ONE unpenalised run of the loop's parts under the same seeds -- every step's (obs, action, next_obs, reward, done)
for all rows -- plus EnsemblePredictor.uncertainty of each step's (obs, action) determine what any penalty must store: the numpy
restatement of mbpo.py:46-63 below with tests/ensemble_restatement.penalty_np between the step and the mask.  Stored rows are compared
bit for bit, through the staging path (a host buffer) and the ring path (a hipets.DeviceReplayBuffer).

Small on purpose: 96 rows, 3 steps, hid 32, obs 11 / act 3 with the hopper termination (rows terminate at every step, see
tests/test_gpu_mbpo_populate.py)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import ensemble_restatement as er
import hipets
import policy_restatement as pr
from conftest import to_spec
from oracle import pets_oracle as po
from test_gpu_policy import BarePolicy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, ACT, L, N, HID = 11, 3, 3, 96, 32


@functools.lru_cache(maxsize=None)
def model_spec():
    om = po.make_synthetic_model(OBS, ACT, ensemble_size=3, hid=HID, seed=21, termination="hopper", propagation="random_model", learned_rewards=True,
                                 reward=None)
    om.weights[-1] = om.weights[-1] * 0.2
    om.max_logvar = torch.full_like(om.max_logvar, -5.0)
    om.biases[-1][:, 0, 0] = -0.03  # the height drifts down: rows cross the hopper threshold at every step
    return to_spec(om, OBS, ACT)


def initial_obs():
    x = (np.random.default_rng(3).standard_normal((N, OBS)) * 0.1).astype(np.float32)
    x[:, 0] += np.float32(0.80)
    return x


@functools.lru_cache(maxsize=None)
def policy():
    return BarePolicy(pr.make_case("penalised", OBS, 32, ACT)[0])


def fresh(engine):
    """an environment and an actor at the start of their streams"""
    return hipets.ModelEnv(model_spec(), engine=engine, mode="device", seed=13), hipets.SACActor(policy(), engine=engine, seed=0)


def trajectory(engine):
    """every step of the unpenalised loop for ALL rows, and the statistics of each step's (obs, action): computed once"""
    if not hasattr(trajectory, "memo"):
        env, actor = fresh(engine)
        predictor = hipets.EnsemblePredictor(model_spec(), engine=engine)
        state = env.reset(initial_obs(), return_as_np=False)
        obs, steps = state["obs"], []
        for _ in range(L):
            action = actor.act_device(obs, sample=True)
            nobs, rew, done, state = env.step(action, state, sample=True)
            stats = {elite: predictor.uncertainty(obs, action, only_elite=elite).cpu().numpy() for elite in (True, False)}
            steps.append(tuple(t.cpu().numpy() for t in (obs, action, nobs, rew.reshape(-1), done.reshape(-1))) + (stats,))
            obs = nobs
        trajectory.memo = steps
    return trajectory.memo


def expected(steps, penalty):
    """mbpo.py:46-63 in numpy over the recorded steps, the penalty between the step and the mask -> (rows per step, stored arrays)"""
    accum, counts, out = np.zeros(N, bool), [], [[] for _ in range(5)]
    for obs, action, nobs, rew, done, stats in steps:
        if penalty is not None:
            rew, done = er.penalty_np(stats[penalty.only_elite], penalty.stat, penalty.coef, rew, done, penalty.halt_threshold, penalty.halt_reward)
        done = np.asarray(done) != 0
        keep = ~accum
        for dst, src in zip(out, (obs, action, nobs, rew, done)):
            dst.append(src[keep])
        counts.append(int(keep.sum()))
        accum |= done
    return counts, [np.concatenate(a) for a in out]


def populate(engine, on_device, **kw):
    """one populate call on a fresh environment and actor -> (rows per step, stored [obs, action, next_obs, reward, done])"""
    env, actor = fresh(engine)
    cap = N * L + 7
    source = pr.MiniReplayBuffer(N, OBS, ACT, initial_obs())
    sac = hipets.DeviceReplayBuffer(cap, (OBS,), (ACT,), engine=engine) if on_device else pr.MiniReplayBuffer(cap, OBS, ACT)
    hipets.rollout_model_and_populate_sac_buffer(env, source, actor, sac, True, L, N, **kw)
    assert env._steps == L and env._resets == 0 and getattr(env, "uncertainty", None) is None  # the environment itself is not changed
    n = sac.num_stored
    if on_device:
        stored = [v[:n].cpu().numpy() for v in sac.views()]
        stored[4] = stored[4] != 0
        return list(sac.last_populate_counts), stored
    return [b[0] for b in sac.batches], [sac.obs[:n], sac.action[:n], sac.next_obs[:n], sac.reward[:n], sac.terminated[:n]]


def same(got, want, what):
    for name, a, b in zip(("obs", "action", "next_obs", "reward", "done"), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("on_device", [False, True], ids=["staging", "ring"])
def test_no_penalty_changes_nothing(engine, on_device, monkeypatch):
    plain = populate(engine, on_device)

    def never(*a, **k):
        raise AssertionError("an ensemble launch without a penalty")

    monkeypatch.setattr(engine, "ensemble_predict", never)
    monkeypatch.setattr(engine, "uncertainty_penalty", never)
    none = populate(engine, on_device, uncertainty=None)
    monkeypatch.undo()
    assert plain[0] == none[0]
    same(none[1], plain[1], "uncertainty=None")
    counts, want = expected(trajectory(engine), None)  # ... and the restatement of the loop is the loop
    assert plain[0] == counts and 0 < counts[-1] < N
    same(plain[1], want, "unpenalised")


@pytest.mark.parametrize("on_device", [False, True], ids=["staging", "ring"])
@pytest.mark.parametrize("kind,coef,elite", [("max_std", 1.0, True), ("disagreement", 0.37, False), ("total_std", 2.5, True), ("max_deviation", 1.0, True)])
def test_penalty_without_halt(engine, on_device, kind, coef, elite):
    penalty = hipets.UncertaintyPenalty(kind, coef=coef, only_elite=elite)
    steps = trajectory(engine)
    counts, want = expected(steps, penalty)
    plain_counts, plain = expected(steps, None)
    got_counts, got = populate(engine, on_device, uncertainty=penalty)
    assert got_counts == counts == plain_counts
    same([got[i] for i in (0, 1, 2, 4)], [plain[i] for i in (0, 1, 2, 4)], f"{kind}: rows other than the reward")
    same(got, want, kind)
    assert not np.array_equal(got[3], plain[3])  # (the penalty is not nothing)


@pytest.mark.parametrize("on_device", [False, True], ids=["staging", "ring"])
@pytest.mark.parametrize("halt_reward", [None, -100.0], ids=["halt", "halt_reward"])
def test_halt_at_the_median_of_the_first_step(engine, on_device, halt_reward):
    steps = trajectory(engine)
    u0 = steps[0][5][True][:, 1]  # (the disagreement: this model's log-variances sit at their upper bound, max_std is one value for all rows)
    threshold = float(np.median(u0))
    penalty = hipets.UncertaintyPenalty("disagreement", coef=0.5, halt_threshold=threshold, halt_reward=halt_reward)
    counts, want = expected(steps, penalty)
    got_counts, got = populate(engine, on_device, uncertainty=penalty)
    halted0 = u0 > np.float32(threshold)
    done0 = steps[0][4] != 0
    print(f"halted at step 0: {int(halted0.sum())} of {N}; done by the model: {int(done0.sum())}; rows per step {got_counts}")
    assert 0 < halted0.sum() < N and got_counts == counts
    assert counts[0] == N and counts[1] == N - int((halted0 | done0).sum())  # a halted row is stored once ...
    same(got, want, "halt")
    assert got[4][:N][halted0].all()  # ... with done = 1
    if halt_reward is not None:
        assert (got[3][:N][halted0] == np.float32(halt_reward)).all()
    later = got[0][N:]  # ... and its successor observations appear in no later step
    gone = {steps[0][2][i].tobytes() for i in np.flatnonzero(halted0)}
    assert not any(row.tobytes() in gone for row in later)


def test_penalised_view_is_made_once_and_leaves_the_environment_alone(engine):
    from hipets import mbpo

    env, _ = fresh(engine)
    a, b = hipets.UncertaintyPenalty("max_std", 1.0), hipets.UncertaintyPenalty("max_std", 2.0)
    va = mbpo._penalised(env, a)
    assert mbpo._penalised(env, hipets.UncertaintyPenalty("max_std", 1.0)) is va and mbpo._penalised(env, b) is not va
    assert env.uncertainty is None and va.env is env
    own = hipets.ModelEnv(model_spec(), engine=engine, mode="device", seed=13, uncertainty=a)
    assert mbpo._penalised(own, a) is own
    # an environment built with the penalty steps what the view of a plain one steps, and a plain step beside them is unpenalised
    action = torch.from_numpy(trajectory(engine)[0][1]).to(DEV)
    outs = []
    for stepper, base in ((own, own), (va, env), (None, fresh(engine)[0])):
        state = base.reset(initial_obs(), return_as_np=False)
        outs.append((stepper or base).step(action, state, sample=True)[:3])
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y)
    assert torch.equal(outs[0][0], outs[2][0]) and not torch.equal(outs[0][1], outs[2][1])
    want = er.penalty_np(trajectory(engine)[0][5][True], 0, 1.0, outs[2][1].cpu().numpy().reshape(-1), outs[2][2].cpu().numpy().reshape(-1))[0]
    assert np.array_equal(outs[0][1].cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32))


class _Lin(torch.nn.Module):  # EnsembleLinearLayer's parameters (models/util.py:31-65)
    def __init__(self, w, b):
        super().__init__()
        self.weight, self.bias, self.use_bias = torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone()), True

    def forward(self, x):
        return x.matmul(self.weight) + self.bias


class _SoftsignMLP(torch.nn.Module):
    """shaped like a GaussianMLP, with an activation module no kernel covers"""

    def __init__(self, spec):
        super().__init__()
        self.hidden_layers = torch.nn.Sequential(*[torch.nn.Sequential(_Lin(w, b), torch.nn.Softsign()) for w, b in zip(spec.weights[:-1], spec.biases[:-1])])
        self.mean_and_logvar = _Lin(spec.weights[-1], spec.biases[-1])
        self.min_logvar, self.max_logvar = torch.nn.Parameter(spec.min_logvar.clone()), torch.nn.Parameter(spec.max_logvar.clone())
        self.elite_models, self.propagation_method, self.deterministic, self.out = None, "random_model", False, spec.out_dim

    def forward(self, x, use_propagation=True):
        assert not use_propagation
        h = self.mean_and_logvar(self.hidden_layers(x))
        lv = self.max_logvar - torch.nn.functional.softplus(self.max_logvar - h[..., self.out:])
        return h[..., :self.out], self.min_logvar + torch.nn.functional.softplus(lv - self.min_logvar)


class _LiveEnv(pr.StubModelEnv):
    """a live ModelEnv as far as the populate call reads one: the stub's reset / step over torch states, a dynamics model"""

    def __init__(self, spec):
        import types

        mlp = _SoftsignMLP(spec)
        self.dynamics_model = types.SimpleNamespace(model=mlp, input_normalizer=None, obs_process_fn=None, target_is_delta=True, no_delta_list=[],
                                                    learned_rewards=True, _get_model_input=lambda obs, act: torch.cat([obs, act], dim=1))
        self.reward_fn = self.termination_fn = None
        self.observation_space, self.action_space = types.SimpleNamespace(shape=(3,)), types.SimpleNamespace(shape=(2,))

    def reset(self, initial_obs_batch, return_as_np=True):
        super().reset(initial_obs_batch)
        return {"obs": torch.from_numpy(self.obs)}

    def step(self, action, model_state, sample=False):
        nxt, rew, done, _ = super().step(action, model_state, sample)
        return nxt, rew, done, {"obs": torch.from_numpy(nxt)}


def test_a_model_the_predictor_refuses_runs_the_reference_loop_with_one_warning(engine):
    from hipets.ensemble import reference_statistics

    case = er.make_case("small_silu")  # obs 3 / act 2 / learned reward; the normaliser is left out
    spec = er.case_spec(dict(case, normalizer="none"))
    live = _LiveEnv(spec)
    with pytest.raises(hipets.UnsupportedModelError):
        hipets.EnsemblePredictor(live, engine=engine)
    c = pr.POPULATE_CASE
    first = np.random.default_rng(1).uniform(-1.0, 1.4, (c["batch_size"], 3)).astype(np.float32)
    penalty = hipets.UncertaintyPenalty("disagreement", coef=0.5, halt_threshold=1e9, only_elite=False)
    agent = type("Agent", (), {"act": staticmethod(pr.stub_act)})()
    runs = []
    for kw in ({}, {"uncertainty": penalty}):
        sac = pr.MiniReplayBuffer(64, 3, 2)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            hipets.rollout_model_and_populate_sac_buffer(_LiveEnv(spec), pr.MiniReplayBuffer(len(first), 3, 2, first), agent, sac, True, 3, len(first), **kw)
        assert len([r for r in rec if "reference's loop" in str(r.message)]) == 1
        runs.append(sac)
    plain, pen = runs
    n = plain.num_stored
    assert pen.num_stored == n > len(first) and [b[0] for b in pen.batches] == [b[0] for b in plain.batches]
    for key in ("obs", "action", "next_obs", "terminated"):
        assert np.array_equal(getattr(pen, key)[:n], getattr(plain, key)[:n])
    with torch.no_grad():
        x = torch.from_numpy(np.concatenate([plain.obs[:n], plain.action[:n]], axis=1))
        stats = reference_statistics(*live.dynamics_model.model.forward(x, use_propagation=False)).numpy()
    # (the loop ran the forward on each step's full batch, this line on the stored rows at once: torch's CPU GEMM may round a row
    # differently in another batch, hence T1 and not the bits; a penalty on the wrong rows misses by orders of magnitude)
    want = er.penalty_np(stats, 1, 0.5, plain.reward[:n], plain.terminated[:n])[0]
    assert (er.t1_share(pen.reward[:n], want) <= 1.0).all() and np.abs(want - plain.reward[:n]).min() > 1e-3
    # reference_statistics against the float64 restatement of the same four numbers
    mean, logvar = (t.detach().double().numpy() for t in live.dynamics_model.model.forward(x, use_propagation=False))
    assert (er.t1_share(stats, er.statistics_f64(mean, logvar)) <= 1.0).all()
