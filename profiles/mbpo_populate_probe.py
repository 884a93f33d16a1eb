"""MBPO's model rollouts at the mbpo_halfcheetah shape (N = 100 000 rows, obs 17, act 6, policy 17-512-512-(6+6), model 7 members /
5 elites, hid 200): what hipets.rollout_model_and_populate_sac_buffer costs against the route a user had before it -- the reference's
loop text (hipets.mbpo.reference_populate_loop) over the same hipets.ModelEnv with a torch GaussianPolicy on the same GPU.

    python profiles/mbpo_populate_probe.py [--out profiles/mbpo_populate.json] [--rows 100000] [--reps 20]

Writes one JSON file and prints the DESIGN.md section 22 table.  Call times: a host clock around calls that end in a device -> host
copy (both routes synchronise by construction), 3 warm-up calls, then the median of --reps (min and p90 next to it).  Kernel times:
device events around one launch, median of --reps, in windows of their own (nothing else enqueued in between).  No profiler runs here;
for a kernel trace run this script under `rocprofv3 --kernel-trace --stats` in a run of its own (its end-to-end numbers then do not count).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mbrl-lib_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hipets  # noqa: E402
from hipets import mbpo  # noqa: E402

OBS, ACT, HID = 17, 6, 512


class TorchGaussianPolicy(torch.nn.Module):
    """The SAC actor as torch runs it: two hidden layers, two heads, clamp, reparameterised sample, tanh squashing"""

    def __init__(self, obs_dim, act_dim, hid):
        super().__init__()
        self.linear1, self.linear2 = torch.nn.Linear(obs_dim, hid), torch.nn.Linear(hid, hid)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(hid, act_dim), torch.nn.Linear(hid, act_dim)
        for lin in (self.linear1, self.linear2, self.mean_linear, self.log_std_linear):
            torch.nn.init.xavier_uniform_(lin.weight, gain=1)
            torch.nn.init.constant_(lin.bias, 0)
        self.action_scale, self.action_bias = torch.tensor(1.0), torch.tensor(0.0)

    def to(self, device):
        self.action_scale, self.action_bias = self.action_scale.to(device), self.action_bias.to(device)
        return super().to(device)

    def sample(self, state):
        x = torch.relu(self.linear2(torch.relu(self.linear1(state))))
        mean, log_std = self.mean_linear(x), torch.clamp(self.log_std_linear(x), -20, 2)
        normal = torch.distributions.Normal(mean, log_std.exp())
        x_t = normal.rsample()
        y_t = torch.tanh(x_t)
        log_prob = normal.log_prob(x_t) - torch.log(self.action_scale * (1 - y_t.pow(2)) + 1e-6)
        return y_t * self.action_scale + self.action_bias, log_prob.sum(1, keepdim=True), torch.tanh(mean) * self.action_scale + self.action_bias


class TorchAgent:
    """SACAgent.act over a policy on the GPU: numpy in, numpy out"""

    def __init__(self, policy, device):
        self.policy, self.device = policy, device

    def act(self, obs, sample=False, batched=False):
        with torch.no_grad():
            state = torch.FloatTensor(obs)
            if not batched:
                state = state.unsqueeze(0)
            action, _, mean = self.policy.sample(state.to(self.device))
            out = (action if sample else mean).detach().cpu().numpy()
        return out if batched else out[0]


class Buffer:
    """A replay buffer's storage: circular add_batch, sample of `rows` stored observations"""

    def __init__(self, capacity, obs_dim, act_dim, rng):
        self.capacity, self.cur, self.stored, self.rng = capacity, 0, 0, rng
        self.obs, self.next_obs = np.zeros((capacity, obs_dim), np.float32), np.zeros((capacity, obs_dim), np.float32)
        self.action, self.reward = np.zeros((capacity, act_dim), np.float32), np.zeros(capacity, np.float32)
        self.terminated, self.truncated = np.zeros(capacity, bool), np.zeros(capacity, bool)

    def add_batch(self, obs, action, next_obs, reward, terminated, truncated):
        done = 0
        while done < len(obs):
            n = min(len(obs) - done, self.capacity - self.cur)
            b, s = slice(self.cur, self.cur + n), slice(done, done + n)
            for dst, src in ((self.obs, obs), (self.action, action), (self.next_obs, next_obs), (self.reward, reward), (self.terminated, terminated),
                             (self.truncated, truncated)):
                np.copyto(dst[b], src[s])
            self.cur, done, self.stored = (self.cur + n) % self.capacity, done + n, min(self.stored + n, self.capacity)

    def sample(self, rows):
        class Batch:
            def __init__(self, obs):
                self.obs = obs

            def astuple(self):
                return self.obs, None, None, None, None, None

        return Batch(self.obs[self.rng.choice(self.stored, size=rows)])


def synthetic_spec(device):
    """the model of bench.py's model_env_step workload: 7 members / 5 elites, 4 hidden layers of 200, SiLU, halfcheetah reward"""
    import bench

    return bench.synthetic_spec(device, ensemble=7, elite=[0, 1, 2, 3, 4])


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": ms[0], "p90_ms": ms[int(0.9 * (len(ms) - 1))], "n": len(ms)}


def wall(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return stats(out)


def events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbpo_populate.json"))
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU: no GPU, no numbers"
    dev = torch.device("cuda:0")
    N = args.rows
    torch.manual_seed(0)
    engine = hipets.get_engine(dev)
    env = hipets.ModelEnv(synthetic_spec(dev), engine=engine, seed=1)
    policy = TorchGaussianPolicy(OBS, ACT, HID).to(dev)
    torch_agent = TorchAgent(policy, dev)
    rng = np.random.default_rng(0)
    source = Buffer(N, OBS, ACT, rng)
    source.add_batch(*(lambda o: (o, np.zeros((N, ACT), np.float32), o, np.zeros(N, np.float32), np.zeros(N, bool), np.zeros(N, bool)))(
        (rng.standard_normal((N, OBS)) * 0.1).astype(np.float32)))
    res = {"shape": {"rows": N, "obs": OBS, "act": ACT, "policy_hidden": HID, "model": "7 members / 5 elites, 4 x 200, SiLU"},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "populate": {}}
    for L in (1, 5):
        sac = Buffer(2 * N * L, OBS, ACT, rng)
        fused = wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, torch_agent, sac, True, L, N), args.reps)
        loop = wall(lambda: mbpo.reference_populate_loop(env, source, torch_agent, sac, True, L, N), args.reps)
        res["populate"][f"L{L}"] = {"fused": fused, "reference_loop_over_hipets_env_and_torch_policy": loop,
                                    "speedup_median": loop["median_ms"] / fused["median_ms"]}
    # ---- the pieces, device events around one launch each ----
    obs = torch.from_numpy(source.obs).to(dev)
    actor = hipets.SACActor(policy, engine=engine)
    res["row_tiles"], res["actor_lds_bytes"] = engine.policy_geometry(N)
    res["actor_kernel"] = events(lambda: actor.act_device(obs, sample=True), args.reps)
    with torch.no_grad():
        res["torch_policy_sample"] = events(lambda: policy.sample(obs), args.reps)
    flops = 2.0 * N * (OBS * HID + HID * HID + HID * 2 * ACT)
    res["actor_kernel"]["tflops"] = flops / (res["actor_kernel"]["median_ms"] * 1e-3) / 1e12
    res["torch_policy_sample"]["tflops"] = flops / (res["torch_policy_sample"]["median_ms"] * 1e-3) / 1e12
    res["actor_kernel"]["weight_stream_bytes_per_launch"] = 4.0 * (16 * HID + HID * HID + HID * 16) * -(-N // (16 * res["row_tiles"]))
    action = actor.act_device(obs, sample=True)
    state = env.reset(source.obs, return_as_np=False)
    res["model_step"] = events(lambda: env.step(action, state, sample=True), args.reps)
    nobs, rew, done, _ = env.step(action, state, sample=True)
    width = 2 * OBS + ACT + 2
    staging = torch.empty(N * width, device=dev)
    offset, count = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    accum = torch.zeros(N, dtype=torch.uint8, device=dev)

    def compact():
        offset.zero_()
        accum.zero_()
        engine.compact_transitions(obs, action, nobs, rew.reshape(-1), done.reshape(-1), accum, staging, N, offset, count)

    res["compaction_step_with_two_resets"] = events(compact, args.reps)
    res["resets_alone"] = events(lambda: (offset.zero_(), accum.zero_()), args.reps)
    bufs = {L: torch.empty(4 + N * L * width, device=dev) for L in (1, 5)}
    res["final_copy"] = {f"L{L}": wall(lambda: mbpo._host_copy(env, bufs[L]), args.reps) for L in (1, 5)}  # (into the pinned buffer)
    res["final_copy_pageable"] = {f"L{L}": wall(lambda: bufs[L].cpu().numpy(), args.reps) for L in (1, 5)}
    res["final_copy"]["bytes"] = {f"L{L}": 4 * (4 + N * L * width) for L in (1, 5)}
    env._return_as_np = True
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    print("\n| what | median ms | min | p90 |\n|---|---|---|---|")
    rows = [(f"populate L={L}, fused", res["populate"][f"L{L}"]["fused"]) for L in (1, 5)]
    rows += [(f"populate L={L}, reference loop + torch policy", res["populate"][f"L{L}"]["reference_loop_over_hipets_env_and_torch_policy"]) for L in (1, 5)]
    rows += [("actor kernel", res["actor_kernel"]), ("torch policy.sample", res["torch_policy_sample"]), ("hipets_step", res["model_step"]),
             ("compaction (+ 2 resets)", res["compaction_step_with_two_resets"]), ("the 2 resets alone", res["resets_alone"]),
             ("final copy L=1 (pinned)", res["final_copy"]["L1"]), ("final copy L=5 (pinned)", res["final_copy"]["L5"]),
             ("the same copy into fresh pageable memory, L=1", res["final_copy_pageable"]["L1"]),
             ("the same copy into fresh pageable memory, L=5", res["final_copy_pageable"]["L5"])]
    for name, s in rows:
        print(f"| {name} | {s['median_ms']:.3f} | {s['min_ms']:.3f} | {s['p90_ms']:.3f} |")


if __name__ == "__main__":
    main()
