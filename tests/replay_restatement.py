"""mbrl.util.ReplayBuffer as MBPO uses it for its SAC buffer (replay_buffer.py:430-460, 521-614, 646-707) and
mbrl.algorithms.mbpo.maybe_replace_sac_buffer (mbpo.py:88-113), restated in numpy for tests that run without the reference; and the
scripted sequence tests/golden/replay_buffer_cases.npz records from the reference itself (tests/make_replay_golden.py), written once
so that the recording, this restatement and hipets.DeviceReplayBuffer are all driven by the same lines.
policy_restatement.MiniReplayBuffer stays what it is (add_batch only, with its call log)."""
import json
import os
import tempfile
from types import SimpleNamespace

import numpy as np

FIELDS = ("obs", "action", "next_obs", "reward", "terminated", "truncated")
SCRIPT = dict(capacity=37, obs_dim=3, act_dim=2, seed=5, data_seed=100, batches=(10, 20, 15, 37), sample=8, grow=50, shrink=30)


class HostRingBuffer:
    def __init__(self, capacity, obs_shape, action_shape, rng=None):
        self.cur_idx, self.capacity, self.num_stored = 0, capacity, 0
        self.obs = np.zeros((capacity, *obs_shape), np.float32)
        self.next_obs = np.zeros((capacity, *obs_shape), np.float32)
        self.action = np.zeros((capacity, *action_shape), np.float32)
        self.reward = np.zeros(capacity, np.float32)
        self.terminated = np.zeros(capacity, bool)
        self.truncated = np.zeros(capacity, bool)
        self._rng = np.random.default_rng() if rng is None else rng

    @property
    def rng(self):
        return self._rng

    def __len__(self):
        return self.num_stored

    def add(self, obs, action, next_obs, reward, terminated, truncated):
        i = self.cur_idx
        self.obs[i], self.next_obs[i], self.action[i], self.reward[i] = obs, next_obs, action, reward
        self.terminated[i], self.truncated[i] = terminated, truncated
        self.cur_idx = (self.cur_idx + 1) % self.capacity
        self.num_stored = min(self.num_stored + 1, self.capacity)

    def add_batch(self, obs, action, next_obs, reward, terminated, truncated):
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

    def _batch_from_indices(self, idx):
        tup = (self.obs[idx], self.action[idx], self.next_obs[idx], self.reward[idx], self.terminated[idx], self.truncated[idx])
        return SimpleNamespace(astuple=lambda: tup)

    def sample(self, batch_size):
        return self._batch_from_indices(self._rng.choice(self.num_stored, size=batch_size))

    def get_all(self, shuffle=False):
        return self._batch_from_indices(self._rng.permutation(self.num_stored) if shuffle else slice(0, self.num_stored))

    def save(self, save_dir):
        n = self.num_stored
        np.savez(os.path.join(save_dir, "replay_buffer.npz"), obs=self.obs[:n], next_obs=self.next_obs[:n], action=self.action[:n],
                 reward=self.reward[:n], terminated=self.terminated[:n], truncated=self.truncated[:n], trajectory_indices=[])

    def load(self, load_dir):
        data = np.load(os.path.join(load_dir, "replay_buffer.npz"))
        n = len(data["obs"])
        for k in FIELDS:
            getattr(self, k)[:n] = data[k]
        self.num_stored, self.cur_idx = n, n % self.capacity


def maybe_replace(sac_buffer, obs_shape, act_shape, new_capacity, seed, make=HostRingBuffer):
    """mbpo.py:88-113 over ``make(capacity, obs_shape, act_shape, rng=...)``"""
    if sac_buffer is None or new_capacity != sac_buffer.capacity:
        rng = np.random.default_rng(seed=seed) if sac_buffer is None else sac_buffer.rng
        new_buffer = make(new_capacity, obs_shape, act_shape, rng=rng)
        if sac_buffer is None:
            return new_buffer
        new_buffer.add_batch(*sac_buffer.get_all().astuple())
        return new_buffer
    return sac_buffer


def script_inputs():
    """The rows the script adds: one batch per entry of SCRIPT["batches"], then the single transition of ``add``"""
    c = SCRIPT
    g = np.random.default_rng(c["data_seed"])
    out = []
    for n in c["batches"] + (1,):
        out.append((g.standard_normal((n, c["obs_dim"])).astype(np.float32), g.standard_normal((n, c["act_dim"])).astype(np.float32),
                    g.standard_normal((n, c["obs_dim"])).astype(np.float32), g.standard_normal(n).astype(np.float32), g.random(n) < 0.3,
                    np.zeros(n, dtype=bool)))
    return out


def rng_state(rng):
    return json.dumps(rng.bit_generator.state, sort_keys=True)


def state_of(buf):
    """What the golden records of a buffer: its stored rows (the rows past num_stored are unwritten memory in the reference), its
    cursor and its generator's state"""
    arrays = buf.get_all().astuple()
    out = {k: np.array(v) for k, v in zip(FIELDS, arrays)}
    out.update(cur_idx=np.int64(buf.cur_idx), num_stored=np.int64(buf.num_stored), rng=np.array(rng_state(buf.rng)))
    return out


def run_script(make, replace):
    """The scripted sequence over ``make(capacity, obs_shape, act_shape, rng=...)`` / ``replace(buffer, obs_shape, act_shape,
    new_capacity, seed)``: {"<step>_<field>": array}.  Also returns the buffers for checks of the caller's own."""
    c = SCRIPT
    shapes = ((c["obs_dim"],), (c["act_dim"],))
    buf = make(c["capacity"], *shapes, rng=np.random.default_rng(c["seed"]))
    rec, inputs = {}, script_inputs()

    def record(step, state):
        rec.update({f"{step}_{k}": v for k, v in state.items()})

    for i, rows in enumerate(inputs[:-1]):
        buf.add_batch(*rows)
        record(f"add_batch{i}", state_of(buf))
    one = inputs[-1]
    buf.add(one[0][0], one[1][0], one[2][0], float(one[3][0]), bool(one[4][0]), bool(one[5][0]))
    record("add", state_of(buf))
    for i in range(2):
        batch = buf.sample(c["sample"]).astuple()
        record(f"sample{i}", dict({"batch_" + k: np.array(v) for k, v in zip(FIELDS, batch)}, rng=np.array(rng_state(buf.rng))))
    batch = buf.get_all(shuffle=True).astuple()
    record("shuffle", dict({"batch_" + k: np.array(v) for k, v in zip(FIELDS, batch)}, rng=np.array(rng_state(buf.rng))))
    with tempfile.TemporaryDirectory() as d:
        buf.save(d)
        loaded = make(c["capacity"], *shapes, rng=np.random.default_rng(0))
        loaded.load(d)
    record("load", {k: v for k, v in state_of(loaded).items() if k != "rng"})
    grown = replace(buf, *shapes, c["grow"], 123)
    record("grow", state_of(grown))
    shrunk = replace(grown, *shapes, c["shrink"], 123)
    record("shrink", state_of(shrunk))
    return rec, dict(buf=buf, loaded=loaded, grown=grown, shrunk=shrunk)
