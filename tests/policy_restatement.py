"""TEST INFRASTRUCTURE: numpy restatements of what hipets/mbpo.py replaces, and the cases the actor tests share.

  actor_f64 / actor_f32   GaussianPolicy.forward / sample (mbrl/third_party/pytorch_sac_pranz24/model.py:88-108) as SAC.select_action
                          hands them out.  actor_f64 is the GPU tests' reference.  actor_f32 follows torch CPU's op order in float32 and
                          is pinned to the bit against the reference's own GaussianPolicy (tests/golden/sac_policy_cases.npz, recorded by
                          tests/make_policy_golden.py): that is what makes the restatement the reference.  Its GEMMs, exp and tanh go
                          through torch's CPU kernels: numpy's BLAS and libm-style float32 exp / tanh differ from torch's in the last
                          places (measured: a third of all exp / tanh arguments, and the hid-64 products), so no numpy-only float32
                          restatement can be bit-equal to torch -- the formula and its op ORDER are what is restated, from explicit
                          weight arrays; the kernels that have more than one valid float32 answer are torch's.
  populate_loop           mbpo.py:46-63 over `act` / `step` callables and an `add_batch` callable.
  GPU_CASES / make_case   the shapes of tests/test_gpu_policy.py and their seeded weights, shared with the golden generator, which records
                          per row how much of T1 torch CPU's float32 forward itself uses against actor_f64 (`u`).
"""
import numpy as np

LOG_SIG_MIN, LOG_SIG_MAX = -20.0, 2.0
T1 = dict(rtol=1e-5, atol=2e-6)  # tests/test_gpu_step.py


def actor_f64(w, obs, sample=False, eps=None):
    """(action, mean, log_std) in float64; `w` = dict of w1 b1 w2 b2 wm bm ws bs action_scale action_bias"""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    h1 = np.maximum(f(obs) @ f(w["w1"]).T + f(w["b1"]), 0.0)
    h2 = np.maximum(h1 @ f(w["w2"]).T + f(w["b2"]), 0.0)
    mean = h2 @ f(w["wm"]).T + f(w["bm"])
    log_std = np.clip(h2 @ f(w["ws"]).T + f(w["bs"]), LOG_SIG_MIN, LOG_SIG_MAX)
    x = mean + np.exp(log_std) * f(eps) if sample else mean
    return np.tanh(x) * f(w["action_scale"]) + f(w["action_bias"]), mean, log_std


def _torch_unary(name, x):
    import torch

    return getattr(torch, name)(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def _torch_linear(x, w, b):
    import torch

    c = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return torch.nn.functional.linear(c(x), c(w), c(b)).numpy()


def actor_f32(w, obs, sample=False, eps=None):
    """(action, mean, log_std) in float32, torch CPU's op order: F.linear, relu, clamp, std = exp(log_std), x_t = mean + eps * std
    (Normal.rsample), tanh(x_t) * action_scale + action_bias.  The kernels with more than one valid float32 answer -- the GEMM of
    F.linear, exp, tanh -- are torch's own (see the module docstring); the rest is numpy."""
    f = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    h1 = np.maximum(_torch_linear(obs, w["w1"], w["b1"]), np.float32(0))
    h2 = np.maximum(_torch_linear(h1, w["w2"], w["b2"]), np.float32(0))
    mean = _torch_linear(h2, w["wm"], w["bm"])
    log_std = np.clip(_torch_linear(h2, w["ws"], w["bs"]), np.float32(LOG_SIG_MIN), np.float32(LOG_SIG_MAX))
    x = mean + f(eps) * _torch_unary("exp", log_std) if sample else mean
    return _torch_unary("tanh", x) * f(w["action_scale"]) + f(w["action_bias"]), mean, log_std


def t1_share(got, ref64):
    """per element, the share of T1 that `got` uses against the float64 `ref64`: |got - ref| / (atol + rtol |ref|)"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref64) / (T1["atol"] + T1["rtol"] * np.abs(ref64))


def populate_loop(initial_obs, act, step, add_batch, rollout_horizon):
    """mbpo.py:46-63: `act(obs) -> action`, `step(action) -> (next_obs, rewards [N, 1], dones [N, 1] bool)`, `add_batch(obs, action,
    next_obs, reward, terminated, truncated)`"""
    accum_dones = np.zeros(initial_obs.shape[0], dtype=bool)
    obs = initial_obs
    for _ in range(rollout_horizon):
        action = act(obs)
        pred_next_obs, pred_rewards, pred_dones = step(action)
        truncateds = np.zeros_like(pred_dones, dtype=bool)
        keep = ~accum_dones
        add_batch(obs[keep], action[keep], pred_next_obs[keep], pred_rewards[keep, 0], pred_dones[keep, 0], truncateds[keep, 0])
        obs = pred_next_obs
        accum_dones |= pred_dones.squeeze()


# ---- the stub agent / model environment of the recorded populate run (deterministic functions of their inputs) ----
def stub_act(obs, sample=False, batched=True):
    obs = np.asarray(obs, dtype=np.float32)
    return np.tanh(obs[:, :2] * np.float32(0.5) + (np.float32(0.25) if sample else np.float32(0))).astype(np.float32)


class StubModelEnv:
    """reset / step with the reference's signatures: rows drift upwards and terminate when dim 0 passes 1 (at different steps)"""

    def reset(self, initial_obs_batch, return_as_np=True):
        self.obs = np.asarray(initial_obs_batch, dtype=np.float32)
        return {"obs": self.obs}

    def step(self, action, model_state, sample=False):
        nxt = (self.obs * np.float32(0.9) + np.float32(0.3) + action.sum(1, keepdims=True) * np.float32(0.1)).astype(np.float32)
        rew = (nxt[:, 1:2] - np.float32(0.5)).astype(np.float32)
        done = nxt[:, 0:1] > np.float32(1.0)
        self.obs = nxt
        return nxt, rew, done, {"obs": nxt}


POPULATE_CASE = dict(obs_dim=3, act_dim=2, n_env=23, batch_size=9, horizon=4, sac_capacity=20, seed=5)


def populate_case_env_buffer(ReplayBuffer):
    """the environment buffer of the recorded run, filled from a seeded generator; `ReplayBuffer` = the class to build it with"""
    c = POPULATE_CASE
    rng = np.random.default_rng(c["seed"])
    buf = ReplayBuffer(c["n_env"] + 5, (c["obs_dim"],), (c["act_dim"],), rng=np.random.default_rng(c["seed"] + 1))
    for _ in range(c["n_env"]):
        o = rng.uniform(-1.0, 1.4, c["obs_dim"]).astype(np.float32)
        buf.add(o, rng.uniform(-1, 1, c["act_dim"]).astype(np.float32), o, 0.0, False, False)
    return buf


# ---- the actor cases of the GPU tests: (name, obs, hidden, act, batch); a batch "R-1" / "R+1" is 16 R -/+ 1 with R the row tiles per
# workgroup of that policy (Engine.policy_geometry).  Hidden widths below, at and past a 16-column tile and at the shipped sizes; (obs,
# act) pairs with every kind of k-chunk remainder; one ragged tile, a workgroup edge, a ragged last workgroup. ----
GPU_CASES = [
    ("o1_h1_a1_b1", 1, 1, 1, 1),
    ("o5_h15_a2_b15", 5, 15, 2, 15),
    ("o5_h16_a2_b16", 5, 16, 2, 16),
    ("o17_h16_a6_b17", 17, 16, 6, 17),
    ("o5_h1_a2_b17", 5, 1, 2, 17),
    ("o23_h15_a6_b1000", 23, 15, 6, 1000),
    ("o23_h72_a6_bRm1", 23, 72, 6, "R-1"),
    ("o23_h72_a6_bRp1", 23, 72, 6, "R+1"),
    ("o17_h200_a6_b1", 17, 200, 6, 1),
    ("o17_h200_a6_bRp1", 17, 200, 6, "R+1"),
    ("o17_h200_a6_b1000", 17, 200, 6, 1000),
    ("o376_h200_a17_b17", 376, 200, 17, 17),
    ("o376_h200_a17_bRm1", 376, 200, 17, "R-1"),
    ("o17_h512_a6_bRm1", 17, 512, 6, "R-1"),
    ("o17_h512_a6_bRp1", 17, 512, 6, "R+1"),
    ("o17_h512_a6_b1000", 17, 512, 6, 1000),
    ("o512_h512_a32_b17", 512, 512, 32, 17),
    ("o512_h512_a32_bRp1", 512, 512, 32, "R+1"),
    ("o1_h1024_a1_b1", 1, 1024, 1, 1),
    ("o17_h1024_a6_b16", 17, 1024, 6, 16),
    ("o376_h1024_a17_bRm1", 376, 1024, 17, "R-1"),
    ("o376_h1024_a17_b17", 376, 1024, 17, 17),
    ("o376_h1024_a17_b1000", 376, 1024, 17, 1000),
    ("o512_h1024_a32_b17", 512, 1024, 32, 17),
]
CASE_ROWS = 1000  # every case draws this many rows; a test uses the first `batch` of them


def make_case(name, obs_dim, hidden, act_dim, rows=CASE_ROWS):
    """(weights dict, obs [rows, obs], eps [rows, act]) of a case: xavier-uniform weights (gain 1) from a generator seeded by the case's
    name, small biases, per-dimension action scale / bias, obs ~ 3 N(0, 1)"""
    rng = np.random.default_rng([ord(c) for c in name])

    def xavier(n_out, n_in):
        a = np.sqrt(6.0 / (n_in + n_out))
        return rng.uniform(-a, a, (n_out, n_in)).astype(np.float32)

    bias = lambda n: rng.uniform(-0.1, 0.1, n).astype(np.float32)  # noqa: E731
    w = {"w1": xavier(hidden, obs_dim), "b1": bias(hidden), "w2": xavier(hidden, hidden), "b2": bias(hidden),
         "wm": xavier(act_dim, hidden), "bm": bias(act_dim), "ws": xavier(act_dim, hidden), "bs": bias(act_dim),
         "action_scale": rng.uniform(0.5, 2.0, act_dim).astype(np.float32), "action_bias": rng.uniform(-1.0, 1.0, act_dim).astype(np.float32)}
    obs = (3.0 * rng.standard_normal((rows, obs_dim))).astype(np.float32)
    eps = rng.standard_normal((rows, act_dim)).astype(np.float32)
    return w, obs, eps


class MiniReplayBuffer:
    """mbrl.util.ReplayBuffer's storage and add_batch (replay_buffer.py:430-460, 553-599) for tests that run without the reference:
    the circular order and the wrap-around.  `sample` returns the rows a test hands it (`initial_obs`), as a TransitionBatch would."""

    def __init__(self, capacity, obs_dim, act_dim, initial_obs=None):
        self.cur_idx, self.capacity, self.num_stored = 0, capacity, 0
        self.obs = np.zeros((capacity, obs_dim), np.float32)
        self.next_obs = np.zeros((capacity, obs_dim), np.float32)
        self.action = np.zeros((capacity, act_dim), np.float32)
        self.reward = np.zeros(capacity, np.float32)
        self.terminated = np.zeros(capacity, bool)
        self.truncated = np.zeros(capacity, bool)
        self.initial_obs = initial_obs
        self.batches = []  # (rows, dtypes, shapes) of every add_batch

    def add_batch(self, obs, action, next_obs, reward, terminated, truncated):
        self.batches.append((len(obs), [np.asarray(a).dtype for a in (obs, action, next_obs, reward, terminated, truncated)],
                             [np.asarray(a).shape for a in (obs, action, next_obs, reward, terminated, truncated)]))

        def copy_from_to(buffer_start, batch_start, how_many):
            b, s = slice(buffer_start, buffer_start + how_many), slice(batch_start, batch_start + how_many)
            for dst, src in ((self.obs, obs), (self.action, action), (self.reward, reward), (self.next_obs, next_obs),
                             (self.terminated, terminated), (self.truncated, truncated)):
                np.copyto(dst[b], src[s])

        batch_start = 0
        if self.cur_idx + len(obs) > self.capacity:
            copy_from_to(self.cur_idx, 0, self.capacity - self.cur_idx)
            batch_start = self.capacity - self.cur_idx
            self.cur_idx, self.num_stored = 0, self.capacity
        how_many = len(obs) - batch_start
        copy_from_to(self.cur_idx, batch_start, how_many)
        self.cur_idx = (self.cur_idx + how_many) % self.capacity
        self.num_stored = min(self.num_stored + how_many, self.capacity)

    def sample(self, batch_size):
        class _Batch:
            def __init__(self, obs):
                self.obs = obs

            def astuple(self):
                return self.obs, None, None, None, None, None

        assert len(self.initial_obs) == batch_size
        return _Batch(self.initial_obs)

    def arrays(self):
        return {"obs": self.obs, "action": self.action, "next_obs": self.next_obs, "reward": self.reward, "terminated": self.terminated,
                "truncated": self.truncated, "cur_idx": np.int64(self.cur_idx), "num_stored": np.int64(self.num_stored)}
