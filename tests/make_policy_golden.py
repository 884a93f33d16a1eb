"""Records tests/golden/sac_policy_cases.npz on the CPU from the reference's own code (needs the reference checkout; run by hand:
`python tests/make_policy_golden.py`).  Holds
  p{i}_*        two GaussianPolicy cases -- (obs 5, hid 64, act 2) without an action space, (obs 11, hid 200, act 3) with an action_space of
                unequal low / high: the weights, obs, the eps torch drew, the `sample` and evaluate actions of GaussianPolicy.sample
  u_{case}      per row of every case of policy_restatement.GPU_CASES: the largest share of T1 that torch CPU's float32 forward of
                the reference's GaussianPolicy uses against the float64 restatement (mean, log_std, evaluate and sample actions)
  pop_*         a run of the reference's rollout_model_and_populate_sac_buffer on a tiny buffer that wraps around, rows terminating at
                different steps: the initial observations it sampled and every array of the SAC buffer afterwards
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import policy_restatement as pr  # noqa: E402
from oracle import ref_bridge  # noqa: E402

OUT = os.path.join(HERE, "golden", "sac_policy_cases.npz")
NAMES = {"w1": "linear1.weight", "b1": "linear1.bias", "w2": "linear2.weight", "b2": "linear2.bias", "wm": "mean_linear.weight",
         "bm": "mean_linear.bias", "ws": "log_std_linear.weight", "bs": "log_std_linear.bias"}


def policy_weights(policy, act_dim):
    sd = policy.state_dict()
    w = {k: sd[v].numpy().copy() for k, v in NAMES.items()}
    for k in ("action_scale", "action_bias"):
        w[k] = np.broadcast_to(getattr(policy, k).numpy().astype(np.float32).reshape(-1), (act_dim,)).copy()
    return w


def sample_with_eps(policy, obs):
    """GaussianPolicy.sample(obs) and the eps its Normal.rsample drew (torch.normal over zeros / ones of the mean's shape)"""
    state = torch.get_rng_state()
    with torch.no_grad():
        action, _, mean_action = policy.sample(obs)
        torch.set_rng_state(state)
        mean, log_std = policy.forward(obs)
        eps = torch.normal(torch.zeros_like(mean), torch.ones_like(mean))
        assert torch.equal(torch.tanh(mean + eps * log_std.exp()) * policy.action_scale + policy.action_bias, action)
    return action.numpy(), mean_action.numpy(), eps.numpy()


def main():
    ref_bridge.import_reference()
    import gymnasium as gym
    from mbrl.third_party.pytorch_sac_pranz24.model import GaussianPolicy

    out = {}
    torch.manual_seed(1234)
    spaces = [None, gym.spaces.Box(np.array([-1.0, -0.5, 0.0], np.float32), np.array([2.0, 0.5, 3.0], np.float32), shape=(3,))]
    for i, ((obs_dim, hid, act), space) in enumerate(zip([(5, 64, 2), (11, 200, 3)], spaces)):
        policy = GaussianPolicy(obs_dim, act, hid, space)
        with torch.no_grad():
            for lin in (policy.linear1, policy.linear2, policy.mean_linear, policy.log_std_linear):
                lin.bias.uniform_(-0.1, 0.1)  # (weights_init_ leaves zeros: a restatement that drops a bias would pass)
        obs = torch.randn(37, obs_dim) * 3
        action, mean_action, eps = sample_with_eps(policy, obs)
        for k, v in policy_weights(policy, act).items():
            out[f"p{i}_{k}"] = v
        out[f"p{i}_obs"], out[f"p{i}_eps"], out[f"p{i}_action_sample"], out[f"p{i}_action_eval"] = obs.numpy(), eps, action, mean_action

    for name, obs_dim, hid, act, _ in pr.GPU_CASES:
        w, obs, eps = pr.make_case(name, obs_dim, hid, act)
        policy = GaussianPolicy(obs_dim, act, hid)
        policy.load_state_dict({v: torch.from_numpy(w[k]) for k, v in NAMES.items()})
        policy.action_scale, policy.action_bias = torch.from_numpy(w["action_scale"]), torch.from_numpy(w["action_bias"])
        with torch.no_grad():
            x = torch.from_numpy(obs)
            mean, log_std = policy.forward(x)
            a_eval = torch.tanh(mean) * policy.action_scale + policy.action_bias
            a_smp = torch.tanh(mean + torch.from_numpy(eps) * log_std.exp()) * policy.action_scale + policy.action_bias
        r_eval, r_mean, r_ls = pr.actor_f64(w, obs)
        r_smp = pr.actor_f64(w, obs, True, eps)[0]
        u = np.max(np.concatenate([pr.t1_share(mean.numpy(), r_mean), pr.t1_share(log_std.numpy(), r_ls), pr.t1_share(a_eval.numpy(), r_eval),
                                   pr.t1_share(a_smp.numpy(), r_smp)], axis=1), axis=1)
        out[f"u_{name}"] = u.astype(np.float32)
        print(f"{name}: torch CPU f32 uses at most {u.max():.3f} of T1 (median row {np.median(u):.3f})")

    import types

    sys.modules.setdefault("imageio", types.ModuleType("imageio"))  # (mbpo.py imports a video recorder this run never touches)
    import mbrl.util
    from mbrl.algorithms.mbpo import rollout_model_and_populate_sac_buffer

    c = pr.POPULATE_CASE
    env_buffer = pr.populate_case_env_buffer(mbrl.util.ReplayBuffer)

    class Agent:
        def act(self, obs, sample=False, batched=False):
            return pr.stub_act(obs, sample, batched)

    sac = mbrl.util.ReplayBuffer(c["sac_capacity"], (c["obs_dim"],), (c["act_dim"],))
    for name in ("obs", "next_obs", "action", "reward", "terminated", "truncated"):
        getattr(sac, name)[...] = 0  # (np.empty storage: the rows never written must compare equal)
    state = env_buffer._rng.bit_generator.state
    initial_obs = env_buffer.sample(c["batch_size"]).astuple()[0]
    env_buffer._rng.bit_generator.state = state
    rollout_model_and_populate_sac_buffer(pr.StubModelEnv(), env_buffer, Agent(), sac, True, c["horizon"], c["batch_size"])
    out["pop_initial_obs"] = initial_obs
    for name in ("obs", "next_obs", "action", "reward", "terminated", "truncated"):
        out["pop_" + name] = getattr(sac, name)
    out["pop_cur_idx"], out["pop_num_stored"] = np.int64(sac.cur_idx), np.int64(sac.num_stored)
    print("populate run: stored", sac.num_stored, "cur_idx", sac.cur_idx)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
