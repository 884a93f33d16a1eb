"""hipets.rollout_model_and_populate_sac_buffer on the GPU against the test's own loop of mbpo.py:40-63 over the parts tested one by one
(SACActor.act in numpy, hipets.ModelEnv.step with numpy returns, numpy masks, add_batch): same seeds, two fresh ModelEnvs, two actors
and two buffers; every array of the SAC buffer bit for bit.

The model: 3 members, hid 200, obs 11 / act 3, the hopper termination.  A GaussianMLP ensemble refuses a batch that is no multiple of its
active members (gaussian_mlp.py:195-200), so the N = 48 cases run all three members and the N = 1 and N = 257 (a prime) cases one elite
member of the same ensemble.  A run in which no row terminates would hide a broken mask: the synthetic model's output layer is scaled to
0.2 and its noise cut (max_logvar -5), the rows start around height 0.80 +- 0.1 and the output bias of the height's delta is -0.03 per
step, so rows cross the 0.7 threshold (or the 0.2 angle bound) at every step -- chosen with the CPU oracle (four draw seeds, both action
kinds): for N >= 48 it leaves between a third and a half of the rows alive before the last of L = 3 steps.  The test asserts 0 < kept < N there."""
import numpy as np
import pytest
import torch

import hipets
import policy_restatement as pr
from conftest import to_spec
from oracle import pets_oracle as po
from test_gpu_policy import BarePolicy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, ACT, L = 11, 3, 3
DRIFT = -0.03


def hopper_model(prop, elite):
    om = po.make_synthetic_model(OBS, ACT, ensemble_size=3, hid=200, seed=21, termination="hopper", propagation=prop, elite=elite)
    om.weights[-1] = om.weights[-1] * 0.2
    om.max_logvar = torch.full_like(om.max_logvar, -5.0)
    om.biases[-1][:, 0, 0] = DRIFT
    return om


def initial_obs(N, seed=0):
    x = (np.random.default_rng(seed).standard_normal((N, OBS)) * 0.1).astype(np.float32)
    x[:, 0] += np.float32(0.80)
    return x


class SacLike:  # .policy, as pytorch_sac_pranz24.SAC carries it
    def __init__(self, policy):
        self.policy = policy


class AgentLike:  # .sac_agent, as mbrl.planning.SACAgent carries it
    def __init__(self, policy):
        self.sac_agent = SacLike(policy)


def own_loop(env, source, actor, sac, sample_action, horizon, batch_size):
    """mbpo.py:40-63 with the pieces at hand"""
    first, *_ = source.sample(batch_size).astuple()
    state = {"s": env.reset(first, return_as_np=True)}

    def step(action):
        nobs, rew, done, state["s"] = env.step(action, state["s"], sample=True)
        assert isinstance(nobs, np.ndarray) and done.dtype == bool and rew.shape == (len(first), 1)
        return nobs, rew, done

    pr.populate_loop(first, lambda o: actor.act(o, sample=sample_action, batched=True), step, sac.add_batch, horizon)


CASES = [  # name, N, propagation, mode, sac_samples_action, the SAC buffer wraps?, agent given as
    ("n1_sample", 1, "random_model", "device", True, False, "actor"),
    ("n1_mean", 1, "random_model", "device", False, False, "actor"),
    ("n48_sample", 48, "random_model", "device", True, False, "actor"),
    ("n48_mean", 48, "random_model", "device", False, False, "agent"),
    ("n257_sample", 257, "random_model", "device", True, False, "agent"),
    ("n257_mean", 257, "random_model", "device", False, False, "actor"),
    ("n48_fixed_sample", 48, "fixed_model", "device", True, False, "actor"),
    ("n48_fixed_mean", 48, "fixed_model", "device", False, False, "actor"),
    ("n48_exact_sample", 48, "random_model", "exact", True, False, "actor"),
    ("n48_wraps", 48, "random_model", "device", True, True, "actor"),
    ("n257_wraps", 257, "fixed_model", "device", True, True, "actor"),
]


@pytest.mark.parametrize("name,N,prop,mode,sample_action,wraps,given", CASES, ids=[c[0] for c in CASES])
def test_populate_equals_the_loop_over_its_parts(engine, name, N, prop, mode, sample_action, wraps, given):
    om = hopper_model(prop, None if N % 3 == 0 else [1])
    spec = to_spec(om, OBS, ACT)
    w, _, _ = pr.make_case("populate", OBS, 64, ACT)
    policy = BarePolicy(w)
    first = initial_obs(N, seed=N)
    cap = N + N // 2 if wraps else 3 * N + 5
    results = []
    for fused in (True, False):
        torch.manual_seed(3)  # ('exact' mode draws its permutations from the global generator, its eps from the env's own)
        env = hipets.ModelEnv(spec, engine=engine, mode=mode, seed=13, generator=torch.Generator().manual_seed(7))
        source, sac = pr.MiniReplayBuffer(N, OBS, ACT, first), pr.MiniReplayBuffer(cap, OBS, ACT)
        if fused:
            agent = AgentLike(policy) if given == "agent" else hipets.SACActor(policy, engine=engine, seed=0)
            hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sac, sample_action, L, N)
            assert env._return_as_np is True  # (as the reference's reset(return_as_np=True) leaves it)
        else:
            own_loop(env, source, hipets.SACActor(policy, engine=engine, seed=0), sac, sample_action, L, N)
        # interleaving: a plain reset + step afterwards draws what it would have drawn after the loop
        state = env.reset(first)
        after = env.step(np.zeros((N, ACT), np.float32), state, sample=True)[:3]
        assert all(isinstance(a, np.ndarray) for a in after)
        results.append((sac, after, env._steps, env._resets, torch.get_rng_state()))
    (fa, fafter, fsteps, fresets, frng), (la, lafter, lsteps, lresets, lrng) = results
    assert (fsteps, fresets) == (lsteps, lresets) and fsteps == L + 1 and torch.equal(frng, lrng)
    for a, b in zip(fafter, lafter):
        assert np.array_equal(a, b)
    kept = [b[0] for b in la.batches]
    print(f"{name}: kept per step {kept} of {N}; stored {la.num_stored}, cur_idx {la.cur_idx}, capacity {cap}")
    assert len(kept) == L and kept[0] == N
    if N >= 48:
        assert 0 < kept[-1] < N, "the mask was never exercised"
    assert wraps == (sum(kept) > cap)
    assert [b[0] for b in fa.batches] == kept
    for (n, dtypes, shapes) in fa.batches:  # reward / terminated / truncated (n,); float32 rows, bool flags
        assert shapes == [(n, OBS), (n, ACT), (n, OBS), (n,), (n,), (n,)]
        assert dtypes == [np.float32] * 4 + [np.bool_] * 2
    want, got = la.arrays(), fa.arrays()
    for key in ("obs", "action", "next_obs", "reward"):
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
    for key in ("terminated", "truncated", "cur_idx", "num_stored"):
        assert np.array_equal(got[key], want[key]), key
    assert not got["truncated"].any() and (N < 48 or got["terminated"].any())


def test_populate_refreshes_the_actor_and_falls_back_for_a_deterministic_policy(engine):
    """SAC updates run between rollouts: the second call sees the new weights.  A DeterministicPolicy-shaped agent runs the
    reference's loop over the same environment, with one warning."""
    N = 48
    spec = to_spec(hopper_model("random_model", None), OBS, ACT)
    w, _, _ = pr.make_case("populate", OBS, 64, ACT)
    policy = BarePolicy(w)
    agent = AgentLike(policy)
    first = initial_obs(N, seed=1)
    env = hipets.ModelEnv(spec, engine=engine, seed=2)
    out = []
    for _ in range(2):
        sac = pr.MiniReplayBuffer(4 * N, OBS, ACT)
        hipets.rollout_model_and_populate_sac_buffer(env, pr.MiniReplayBuffer(N, OBS, ACT, first), agent, sac, False, 1, N)
        out.append(sac.action[:N].copy())
        with torch.no_grad():
            policy.mean_linear.bias.add_(0.3)
    assert not np.array_equal(out[0], out[1])

    class Deterministic(torch.nn.Module):  # pytorch_sac_pranz24/model.py:116-141
        def __init__(self):
            super().__init__()
            self.linear1, self.linear2, self.mean = torch.nn.Linear(OBS, 8), torch.nn.Linear(8, 8), torch.nn.Linear(8, ACT)

    class Agent:
        def __init__(self):
            self.sac_agent = SacLike(Deterministic())
            self.calls = 0

        def act(self, obs, sample=False, batched=False):
            self.calls += 1
            return np.zeros((len(obs), ACT), np.float32)

    with pytest.raises(hipets.UnsupportedModelError):
        hipets.SACActor(Agent(), engine=engine)
    stock, sac = Agent(), pr.MiniReplayBuffer(4 * N, OBS, ACT)
    steps = env._steps
    with pytest.warns(UserWarning, match="reference's loop") as rec:
        hipets.rollout_model_and_populate_sac_buffer(env, pr.MiniReplayBuffer(N, OBS, ACT, first), stock, sac, True, 2, N)
    assert len([r for r in rec if "reference's loop" in str(r.message)]) == 1 and stock.calls == 2 and env._steps == steps + 2 and sac.batches[0][0] == N
