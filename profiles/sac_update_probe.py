"""SAC's updates at the mbpo_halfcheetah shape (obs 17, act 6, hidden 512, batch 256) and at a 1024-wide shape (obs 376, act 17): what
hipets.SACUpdater costs per update against the route a user had before it -- SAC.update_parameters in stock torch (torch.optim.Adam,
autograd) on the same GPU over the same buffers.  The torch route is tests/sac_restatement.TinySAC, whose update_parameters runs the
reference's op sequence (tests/test_sac_update_host.py pins it to the recording of the reference's own code bit for bit).

    python profiles/sac_update_probe.py [--out profiles/sac_update.json] [--reps 20]

Writes one JSON file and prints the DESIGN.md section 23 table.  Times per update: a host clock around calls that end in a device ->
host copy (both routes synchronise by construction), 3 warm-up calls, then the median of --reps (min and p90 next to it); the launch
sequence alone: device events around 20 queued hipets_sac_update calls; the host's share: sample + pack, upload and read-back timed on
their own.  The iteration share: one populate call at rollout length 1 (100 000 rows) plus 20 updates, before and after.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mbrl-lib_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hipets  # noqa: E402
import mbpo_populate_probe as pp  # noqa: E402
import sac_restatement as sr  # noqa: E402
from hipets import mbpo  # noqa: E402

SHAPES = {"mbpo_halfcheetah": (17, 6, 512, 256), "wide_1024": (376, 17, 1024, 256)}
N_UPDATES = 20


class ReplayBuffer:
    """mbrl.util.ReplayBuffer's sample: ``rng.choice`` of the stored rows, fancy-indexed copies of the six arrays"""

    def __init__(self, n, obs, act, rng):
        self.rng, self.n = rng, n
        self.arrays = ((rng.standard_normal((n, obs)) * 0.5).astype(np.float32), rng.uniform(-1, 1, (n, act)).astype(np.float32),
                       (rng.standard_normal((n, obs)) * 0.5).astype(np.float32), rng.standard_normal(n).astype(np.float32),
                       rng.random(n) < 0.05, np.zeros(n, dtype=bool))

    def sample(self, batch_size):
        idx = self.rng.choice(self.n, size=batch_size)
        tup = tuple(a[idx] for a in self.arrays)

        class Batch:
            def astuple(self):
                return tup

        return Batch()

    def __len__(self):
        return self.n


def per_update(stat, n):
    return {k: (v / n if k.endswith("_ms") else v) for k, v in stat.items()}


def measure_shape(engine, dev, shape, reps):
    obs, act, hid, B = shape
    rng = np.random.default_rng(0)
    memory = ReplayBuffer(100_000, obs, act, rng)
    torch.manual_seed(0)
    sac_t = sr.TinySAC(obs, act, hid, device=dev)
    sac_h = sr.TinySAC(obs, act, hid, device=dev)
    up = hipets.SACUpdater(sac_h, engine=engine)
    res = {"shape": dict(obs=obs, act=act, hidden=hid, batch=B)}
    count = [0]

    def single():
        up.update_parameters(memory, B, count[0], None, reverse_mask=True)
        count[0] += 1

    def many():
        up.update_many([memory] * N_UPDATES, B, count[0], None, reverse_mask=True)
        count[0] += N_UPDATES

    def stock():
        for _ in range(N_UPDATES):
            sac_t.update_parameters(memory, B, count[0], None, reverse_mask=True)
            count[0] += 1

    res["update_parameters"] = pp.wall(single, reps)
    res["update_many_20_per_update"] = per_update(pp.wall(many, reps), N_UPDATES)
    res["torch_update_parameters"] = per_update(pp.wall(stock, reps), N_UPDATES)
    # ---- the launch sequence alone: 20 queued updates, everything already on the device ----
    width = 2 * obs + act + 2
    batch = torch.from_numpy(np.stack([mbpo.pack_sac_batch(memory.sample(B).astuple(), True) for _ in range(N_UPDATES)])).to(dev)
    eps = torch.randn(N_UPDATES, 2, B, act, device=dev)
    result = torch.empty(N_UPDATES, 8, device=dev)
    steps = [0]

    def launches():
        for i in range(N_UPDATES):
            engine.sac_update(batch[i], eps[i, 0], eps[i, 1], i, (steps[0], steps[0], steps[0]), (3e-4, 3e-4, 3e-4), result[i])
            steps[0] += 1

    up._bind()
    res["launch_sequence_device_per_update"] = per_update(pp.events(launches, reps), N_UPDATES)
    # ---- the host's share of one update ----
    host = torch.empty(B, width, pin_memory=True)
    host_res = torch.empty(8, pin_memory=True)

    def t_host(fn):
        out = []
        for _ in range(reps + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return pp.stats(out[3:])

    res["host_sample_and_pack"] = t_host(lambda: mbpo.pack_sac_batch(memory.sample(B).astuple(), True, out=host.numpy()))
    res["host_upload"] = t_host(lambda: host.to(dev, non_blocking=True))
    res["host_read_back"] = t_host(lambda: host_res.copy_(result[0], non_blocking=True))
    res["speedup_update_parameters"] = res["torch_update_parameters"]["median_ms"] / res["update_parameters"]["median_ms"]
    res["speedup_update_many"] = res["torch_update_parameters"]["median_ms"] / res["update_many_20_per_update"]["median_ms"]
    return res, (sac_t, sac_h, up, memory)


def iteration_share(engine, dev, agents, reps):
    """populate at rollout length 1 (100 000 rows) + 20 updates at the mbpo_halfcheetah shape: the update loop's share, both routes"""
    sac_t, sac_h, up, memory = agents
    obs, act, hid, B = SHAPES["mbpo_halfcheetah"]
    N = 100_000
    rng = np.random.default_rng(1)
    env = hipets.ModelEnv(pp.synthetic_spec(dev), engine=engine, seed=1)
    source = pp.Buffer(N, obs, act, rng)
    o = (rng.standard_normal((N, obs)) * 0.1).astype(np.float32)
    source.add_batch(o, np.zeros((N, act), np.float32), o, np.zeros(N, np.float32), np.zeros(N, bool), np.zeros(N, bool))
    sink = pp.Buffer(2 * N, obs, act, rng)
    agent = pp.TorchAgent(sac_h.policy, dev)
    populate = pp.wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sink, True, 1, N), reps)
    env._return_as_np = True
    count = [10_000]

    def loop_torch():
        for _ in range(N_UPDATES):
            sac_t.update_parameters(memory, B, count[0], None, reverse_mask=True)
            count[0] += 1

    def loop_hip():
        up.update_many([memory] * N_UPDATES, B, count[0], None, reverse_mask=True)
        count[0] += N_UPDATES

    before, after = pp.wall(loop_torch, reps), pp.wall(loop_hip, reps)
    p = populate["median_ms"]
    return {"populate_L1_100000_rows": populate, "update_loop_torch_20": before, "update_loop_hipets_20": after,
            "share_before": before["median_ms"] / (before["median_ms"] + p), "share_after": after["median_ms"] / (after["median_ms"] + p),
            "iteration_ms_before": before["median_ms"] + p, "iteration_ms_after": after["median_ms"] + p}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_update.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU: no GPU, no numbers"
    dev = torch.device("cuda:0")
    engine = hipets.get_engine(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "updates_per_many_call": N_UPDATES,
           "torch_route": "tests/sac_restatement.TinySAC.update_parameters (sac.py:76-173's op sequence, torch.optim.Adam)", "shapes": {}}
    keep = None
    for name, shape in SHAPES.items():
        res["shapes"][name], agents = measure_shape(engine, dev, shape, args.reps)
        if name == "mbpo_halfcheetah":
            keep = agents
    res["iteration"] = iteration_share(engine, dev, keep, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    print("\n| shape | what, per update | median ms | min | p90 |\n|---|---|---|---|---|")
    for name, r in res["shapes"].items():
        for key in ("torch_update_parameters", "update_parameters", "update_many_20_per_update", "launch_sequence_device_per_update",
                    "host_sample_and_pack", "host_upload", "host_read_back"):
            s = r[key]
            print(f"| {name} | {key} | {s['median_ms']:.3f} | {s['min_ms']:.3f} | {s['p90_ms']:.3f} |")


if __name__ == "__main__":
    main()
