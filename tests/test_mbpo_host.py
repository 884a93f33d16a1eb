"""hipets/mbpo.py on the host, no GPU: the restatements the GPU tests lean on against what the reference itself computed
(tests/golden/sac_policy_cases.npz, recorded by tests/make_policy_golden.py; re-derived live where the reference is importable), the
Python side of the populate call over a stub engine and a stub model environment against the recorded run of the reference's own
function, the Engine binding of the new entry points, argument refusal and the fallback warning."""
import os
import warnings

import numpy as np
import pytest
import torch

import hipets
import policy_restatement as pr
from conftest import GOLDEN
from hipets import mbpo
from oracle import ref_bridge
from test_engine_binding_host import ANY, check, eng, take  # noqa: F401  (eng: the Engine over a recording library)

GOLD = dict(np.load(os.path.join(GOLDEN, "sac_policy_cases.npz")))
POLICY_CASES = [(0, 5, 64, 2), (1, 11, 200, 3)]
KEYS = ("w1", "b1", "w2", "b2", "wm", "bm", "ws", "bs", "action_scale", "action_bias")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("i,obs_dim,hid,act", POLICY_CASES)
def test_f32_restatement_is_the_recorded_policy_to_the_bit(i, obs_dim, hid, act):
    w = {k: GOLD[f"p{i}_{k}"] for k in KEYS}
    assert w["w1"].shape == (hid, obs_dim) and w["ws"].shape == (act, hid)
    if i == 1:
        assert len(set(w["action_scale"].tolist())) > 1 and np.any(w["action_bias"] != 0)  # an action_space of unequal low / high
    obs, eps = GOLD[f"p{i}_obs"], GOLD[f"p{i}_eps"]
    assert np.array_equal(bits(pr.actor_f32(w, obs, True, eps)[0]), bits(GOLD[f"p{i}_action_sample"]))
    assert np.array_equal(bits(pr.actor_f32(w, obs)[0]), bits(GOLD[f"p{i}_action_eval"]))
    for sample, key in ((True, "action_sample"), (False, "action_eval")):
        share = pr.t1_share(GOLD[f"p{i}_{key}"], pr.actor_f64(w, obs, sample, eps)[0])
        print(f"policy {i} {key}: torch CPU f32 uses {share.max():.3f} of T1 against the f64 restatement")
        assert share.max() < 1.0


@pytest.mark.skipif(not ref_bridge.reference_available(), reason="needs the reference checkout")
@pytest.mark.parametrize("i,obs_dim,hid,act", POLICY_CASES)
def test_f32_restatement_against_the_live_reference(i, obs_dim, hid, act):
    ref_bridge.import_reference()
    from mbrl.third_party.pytorch_sac_pranz24.model import GaussianPolicy

    w = {k: GOLD[f"p{i}_{k}"] for k in KEYS}
    policy = GaussianPolicy(obs_dim, act, hid)
    with torch.no_grad():
        for lin, k in ((policy.linear1, "1"), (policy.linear2, "2"), (policy.mean_linear, "m"), (policy.log_std_linear, "s")):
            lin.weight.copy_(torch.from_numpy(w["w" + k]))
            lin.bias.copy_(torch.from_numpy(w["b" + k]))
        policy.action_scale, policy.action_bias = torch.from_numpy(w["action_scale"]), torch.from_numpy(w["action_bias"])
        torch.manual_seed(77)
        obs = torch.randn(29, obs_dim) * 3
        state = torch.get_rng_state()
        action, _, mean_action = policy.sample(obs)
        torch.set_rng_state(state)
        eps = torch.normal(torch.zeros(29, act), torch.ones(29, act))
    assert np.array_equal(bits(pr.actor_f32(w, obs.numpy(), True, eps.numpy())[0]), bits(action.numpy()))
    assert np.array_equal(bits(pr.actor_f32(w, obs.numpy())[0]), bits(mean_action.numpy()))
    (dims, tensors) = hipets._pack.pack_policy(policy)
    assert dims == (obs_dim, hid, act) and list(tensors) == list(KEYS)
    assert all(np.array_equal(tensors[k].numpy(), w[k]) for k in KEYS)


def recorded_buffer():
    return {k[4:]: GOLD[k] for k in GOLD if k.startswith("pop_") and k != "pop_initial_obs"}


def assert_buffer_is_the_recorded_run(buf):
    want, got = recorded_buffer(), buf.arrays()
    assert sorted(want) == sorted(got)
    for k in want:
        assert got[k].dtype == want[k].dtype or k in ("cur_idx", "num_stored"), k
        assert np.array_equal(got[k], want[k]), k


def test_populate_restatement_is_the_recorded_run_of_the_reference():
    """mbpo.py:46-63 restated, over the stub act / step the generator gave the reference's own function; the SAC buffer wraps (capacity
    20) and rows terminate at different steps"""
    c = pr.POPULATE_CASE
    first = GOLD["pop_initial_obs"]
    assert first.shape == (c["batch_size"], c["obs_dim"])
    env, sac = pr.StubModelEnv(), pr.MiniReplayBuffer(c["sac_capacity"], c["obs_dim"], c["act_dim"])
    state = env.reset(first)
    pr.populate_loop(first, lambda o: pr.stub_act(o, True), lambda a: env.step(a, state, sample=True)[:3], sac.add_batch, c["horizon"])
    kept = [b[0] for b in sac.batches]
    assert kept[0] == c["batch_size"] and 0 < kept[-1] < kept[0] and len(set(kept)) > 2 and sum(kept) > c["sac_capacity"]
    assert_buffer_is_the_recorded_run(sac)


class TinyPolicy(torch.nn.Module):
    def __init__(self, obs_dim=3, hid=4, act=2, heads=True):
        super().__init__()
        self.linear1, self.linear2 = torch.nn.Linear(obs_dim, hid), torch.nn.Linear(hid, hid)
        if heads:
            self.mean_linear, self.log_std_linear = torch.nn.Linear(hid, act), torch.nn.Linear(hid, act)
        else:
            self.mean = torch.nn.Linear(hid, act)  # DeterministicPolicy (pytorch_sac_pranz24/model.py:116-141)
        self.action_scale, self.action_bias = torch.tensor(1.0), torch.tensor(0.0)


class StubEngine:
    """The four Engine methods hipets/mbpo.py calls, on CPU tensors: the actor is policy_restatement.stub_act, the compaction numpy's
    boolean indexing written into the staging area's five arrays (include/hipets.h)"""
    device = torch.device("cpu")

    def __init__(self):
        self.sets, self.acts = 0, []

    def policy_set(self, policy):
        self.sets += 1
        return hipets._pack.pack_policy(policy)[0]

    def policy_act(self, obs, *, sample=False, seed=0, stream_id=0, eps=None):
        self.acts.append((bool(sample), seed, stream_id))
        return torch.from_numpy(pr.stub_act(obs.numpy(), sample))

    def compact_transitions(self, obs, action, next_obs, rewards, dones, accum, staging, cap, offset, count_out):
        keep = ~accum.numpy().astype(bool)
        o, n = int(offset), int(keep.sum())
        parts = (obs, action, next_obs, rewards, dones.to(torch.float32))
        for view, src in zip(mbpo.staging_views(staging, cap, obs.shape[1], action.shape[1]), parts):
            view[o:o + n] = src[torch.from_numpy(keep)]
        offset += n
        count_out[0] = n
        accum |= dones.to(torch.uint8)


class StubHipEnv:
    """What hipets/mbpo.py needs of a hipets.ModelEnv, over policy_restatement.StubModelEnv"""

    def __init__(self):
        self.engine, self.device, self._return_as_np, self._steps, self._resets = StubEngine(), torch.device("cpu"), True, 0, 0
        self._inner = pr.StubModelEnv()

    def reset(self, initial_obs_batch, return_as_np=True):
        self._return_as_np, self._resets = return_as_np, self._resets + 1
        return {"obs": torch.from_numpy(self._inner.reset(initial_obs_batch)["obs"])}

    def step(self, actions, model_state, sample=False):
        self._steps += 1
        a = actions if isinstance(actions, np.ndarray) else actions.numpy()
        nobs, rew, done, _ = self._inner.step(a, None, sample=sample)
        if self._return_as_np:
            return nobs, rew, done, model_state
        return torch.from_numpy(nobs), torch.from_numpy(rew), torch.from_numpy(done), {"obs": torch.from_numpy(nobs)}


def test_populate_over_a_stub_engine_is_the_recorded_run():
    """the Python side of the fused call: one reset, per step one actor call / one step / one compaction, one copy, one add_batch per
    step over views of it -- the SAC buffer of the reference's own run"""
    c = pr.POPULATE_CASE
    env = StubHipEnv()
    agent = TinyPolicy()
    sac = pr.MiniReplayBuffer(c["sac_capacity"], c["obs_dim"], c["act_dim"])
    source = pr.MiniReplayBuffer(1, c["obs_dim"], c["act_dim"], GOLD["pop_initial_obs"])
    hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sac, True, c["horizon"], c["batch_size"])
    assert_buffer_is_the_recorded_run(sac)
    assert env._steps == c["horizon"] and env._resets == 1 and env._return_as_np is True
    assert env.engine.sets == 2  # the actor's construction, and the refresh of the call
    assert env.engine.acts == [(True, 0, t + 1) for t in range(c["horizon"])]  # one draw stream per sampling call
    for n, dtypes, shapes in sac.batches:
        assert shapes[3:] == [(n,), (n,), (n,)] and dtypes[3:] == [np.float32, np.bool_, np.bool_]
    # a second call: the cached actor, refreshed again; evaluate actions consume no draw stream
    hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sac, False, 2, c["batch_size"])
    assert env.engine.sets == 3 and env.engine.acts[-2:] == [(False, 0, 0)] * 2 and env._steps == c["horizon"] + 2


def test_unsupported_policies_are_refused_and_the_populate_call_falls_back():
    e = StubEngine()
    with pytest.raises(hipets.UnsupportedModelError, match="not shaped like a GaussianPolicy"):
        hipets.SACActor(TinyPolicy(heads=False), engine=e)
    with pytest.raises(hipets.UnsupportedModelError, match="outside the actor kernel's"):
        hipets.SACActor(TinyPolicy(obs_dim=513), engine=e)
    with pytest.raises(hipets.UnsupportedModelError, match="outside the actor kernel's"):
        hipets.SACActor(TinyPolicy(hid=1025), engine=e)
    with pytest.raises(hipets.UnsupportedModelError, match="outside the actor kernel's"):
        hipets.SACActor(TinyPolicy(act=33), engine=e)
    bad = TinyPolicy()
    bad.action_scale = torch.ones(3)
    with pytest.raises(hipets.UnsupportedModelError, match="action_scale"):
        hipets.SACActor(bad, engine=e)
    assert e.sets == 0
    actor = hipets.SACActor(TinyPolicy(), engine=e, seed=4)
    with pytest.raises(ValueError, match=r"obs must be \[B, 3\]"):
        actor.act(np.zeros((5, 4), np.float32), batched=True)
    assert actor.act(np.zeros(3, np.float32)).shape == (2,) and actor.act(np.zeros((5, 3)), sample=True, batched=True).shape == (5, 2)
    assert e.acts == [(False, 4, 0), (True, 4, 1)]

    class Agent:  # a DeterministicPolicy behind the SACAgent seam: the reference's loop over the same environment, one warning
        def __init__(self):
            self.sac_agent = type("Sac", (), {"policy": TinyPolicy(heads=False)})()

        def act(self, obs, sample=False, batched=False):
            return pr.stub_act(obs, sample, batched)

    c = pr.POPULATE_CASE
    env, sac = StubHipEnv(), pr.MiniReplayBuffer(c["sac_capacity"], c["obs_dim"], c["act_dim"])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        hipets.rollout_model_and_populate_sac_buffer(env, pr.MiniReplayBuffer(1, c["obs_dim"], c["act_dim"], GOLD["pop_initial_obs"]), Agent(), sac,
                                                     True, c["horizon"], c["batch_size"])
    assert len(rec) == 1 and "reference's loop" in str(rec[0].message) and "GaussianPolicy" in str(rec[0].message)
    assert_buffer_is_the_recorded_run(sac)
    assert env.engine.sets == 0 and env._steps == c["horizon"]


def test_engine_binding_of_the_policy_and_compaction_entry_points(eng):  # noqa: F811
    policy = TinyPolicy(obs_dim=5, hid=8, act=2)
    assert eng.policy_set(policy) == (5, 8, 2)
    rec = take(eng, "hipets_policy_set")
    check(rec, "hipets_policy_set", obs_dim=5, hidden=8, act_dim=2, w1=policy.linear1.weight, b1=policy.linear1.bias, w2=policy.linear2.weight,
          b2=policy.linear2.bias, wm=policy.mean_linear.weight, bm=policy.mean_linear.bias, ws=policy.log_std_linear.weight,
          bs=policy.log_std_linear.bias, action_scale=ANY, action_bias=ANY)
    obs, eps = torch.zeros(7, 5), torch.zeros(7, 2)
    out = eng.policy_act(obs, sample=True, seed=2**40 + 1, stream_id=9, eps=eps)
    check(take(eng, "hipets_policy_act"), "hipets_policy_act", obs=obs, batch=7, sample=1, seed=2**40 + 1, stream_id=9, eps=eps, actions=out,
          mean_out=None, log_std_out=None)
    a, mean, ls = eng.policy_act(obs, taps=True)
    check(take(eng, "hipets_policy_act"), "hipets_policy_act", obs=obs, batch=7, sample=0, seed=0, stream_id=0, eps=None, actions=a, mean_out=mean,
          log_std_out=ls)
    n = eng.policy_normals(7, 2, 3, 4)
    check(take(eng, "hipets_policy_normals"), "hipets_policy_normals", batch=7, act_dim=2, seed=3, stream_id=4, out=n)
    with pytest.raises(ValueError, match="obs must have shape"):
        eng.policy_act(torch.zeros(7, 4))
    with pytest.raises(ValueError, match="eps must have shape"):
        eng.policy_act(obs, sample=True, eps=torch.zeros(7, 3))
    t = dict(obs=torch.zeros(6, 5), action=torch.zeros(6, 2), next_obs=torch.zeros(6, 5), rewards=torch.zeros(6, 1), dones=torch.zeros(6, 1, dtype=torch.bool),
             accum_dones=torch.zeros(6, dtype=torch.uint8), staging=torch.zeros(18 * 14), cap=18, offset=torch.zeros(1, dtype=torch.int64),
             count_out=torch.zeros(1, dtype=torch.int32))
    eng.compact_transitions(*t.values())
    check(take(eng, "hipets_compact_transitions"), "hipets_compact_transitions", n=6, obs_dim=5, act_dim=2, **t)
    with pytest.raises(ValueError, match="staging must hold"):
        eng.compact_transitions(*{**t, "staging": torch.zeros(18 * 14 - 1)}.values())
    with pytest.raises(hipets.HipetsError, match="policy_set"):
        type(eng).policy_act(object.__new__(type(eng)), obs)
    assert eng._lib.calls == []
