"""The wide form of the SAC actor's and critic's forward (kernel="wide", csrc/agent_wide.hip) against the tile form and the live torch
modules on one MI355X:
    python profiles/agent_wide_probe.py --out profiles/agent_wide.json
Three routes take turns in one process, sample by sample (value_objective_probe.measure: warm-up rounds, then samples of the
device-event time of `reps` back-to-back calls / reps; median, min, p90 in ms per call):
  actor    100 000 rows, obs / act / hidden 17 / 6 / 512, 17 / 6 / 1024, 376 / 17 / 1024: SACActor.act_device(sample=True) under both
           forms, torch's policy.sample (mbpo_populate_probe.TorchGaussianPolicy);
  critic   10 000 rows, 17 / 6 / 256, 17 / 6 / 512, 376 / 17 / 1024 (DESIGN.md section 24's rows): SACCritic.q under both forms, the
           live module's torch.min(*critic(s, a)).
Then one hipets.rollout_model_and_populate_sac_buffer call (rollout length 1, 100 000 rows, the populate probe's model) with a policy
of hidden 1024 under agent_kernel="tile" and "wide": a host clock around calls that end in a device -> host copy.
`wide_wins` of a shape: the wide median is below the tile median and the [min, p90] ranges do not overlap -- the rule that sets
hipets.sac.AGENT_WIDE_MIN_HIDDEN."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "mbrl-lib_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hipets  # noqa: E402
import mbpo_populate_probe as pop  # noqa: E402
from value_objective_probe import make_agent, measure  # noqa: E402

ACTOR_SHAPES = ((17, 6, 512), (17, 6, 1024), (376, 17, 1024))
CRITIC_SHAPES = ((17, 6, 256), (17, 6, 512), (376, 17, 1024))


def verdict(ms):
    tile, wide = ms["tile"], ms["wide"]
    return bool(wide["median"] < tile["median"] and wide["p90"] < tile["min"])


def actor_piece(obs, act, hid, rows, eng, a):
    dev = eng.device
    torch.manual_seed(0)
    policy = pop.TorchGaussianPolicy(obs, act, hid).to(dev)
    actors = {k: hipets.SACActor(policy, engine=eng, kernel=k) for k in ("tile", "wide")}
    x = torch.randn(rows, obs, generator=torch.Generator().manual_seed(1)).to(dev)
    eps = torch.randn(rows, act, generator=torch.Generator().manual_seed(2)).to(dev)
    got = {k: v.act_device(x, sample=True, eps=eps) for k, v in actors.items()}

    def torch_route():
        with torch.no_grad():
            return policy.sample(x)

    ms = measure({"tile": lambda: actors["tile"].act_device(x, sample=True), "wide": lambda: actors["wide"].act_device(x, sample=True),
                  "torch_policy_sample": torch_route}, a)
    return {"shape": dict(obs=obs, act=act, hidden=hid, rows=rows), "geometry": {k: eng.policy_geometry(rows, kernel=k) for k in actors},
            "max_abs_diff_wide_vs_tile": float((got["wide"] - got["tile"]).abs().max()), "ms": ms, "wide_wins": verdict(ms),
            "wide_over_tile": ms["wide"]["median"] / ms["tile"]["median"], "wide_over_torch": ms["wide"]["median"] / ms["torch_policy_sample"]["median"]}


def critic_piece(obs, act, hid, rows, eng, a):
    dev = eng.device
    agent = make_agent(obs, act, hid, dev)
    critics = {k: hipets.SACCritic(agent, engine=eng, kernel=k) for k in ("tile", "wide")}
    g = torch.Generator().manual_seed(1)
    s, u = torch.randn(rows, obs, generator=g).to(dev), (torch.rand(rows, act, generator=g) * 2 - 1).to(dev)
    got = {k: v.q(s, u)[2] for k, v in critics.items()}

    def torch_route():
        with torch.no_grad():
            return torch.min(*agent.critic(s, u))

    ms = measure({"tile": lambda: critics["tile"].q(s, u), "wide": lambda: critics["wide"].q(s, u), "torch_live_critic_min": torch_route}, a)
    return {"shape": dict(obs=obs, act=act, hidden=hid, rows=rows), "geometry": {k: eng.critic_geometry(rows, kernel=k) for k in critics},
            "max_abs_diff_wide_vs_tile": float((got["wide"] - got["tile"]).abs().max()), "ms": ms, "wide_wins": verdict(ms),
            "wide_over_tile": ms["wide"]["median"] / ms["tile"]["median"], "wide_over_torch": ms["wide"]["median"] / ms["torch_live_critic_min"]["median"]}


def populate_piece(rows, eng, reps):
    dev = eng.device
    env = hipets.ModelEnv(pop.synthetic_spec(dev), engine=eng, seed=1)
    torch.manual_seed(0)
    policy = pop.TorchGaussianPolicy(pop.OBS, pop.ACT, 1024).to(dev)
    rng = np.random.default_rng(0)
    source = pop.Buffer(rows, pop.OBS, pop.ACT, rng)
    o = (rng.standard_normal((rows, pop.OBS)) * 0.1).astype(np.float32)
    source.add_batch(o, np.zeros((rows, pop.ACT), np.float32), o, np.zeros(rows, np.float32), np.zeros(rows, bool), np.zeros(rows, bool))
    sac = pop.Buffer(2 * rows, pop.OBS, pop.ACT, rng)
    out = {k: pop.wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, policy, sac, True, 1, rows, agent_kernel=k), reps)
           for k in ("tile", "wide")}
    return {"shape": dict(rows=rows, obs=pop.OBS, act=pop.ACT, policy_hidden=1024, rollout_length=1), "ms": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("agent_wide_probe.py needs a GPU: nothing measured", file=sys.stderr)
        return 1
    eng = hipets.get_engine(torch.device("cuda:0"))
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"{a.warmup} warm-up rounds, then {a.samples} samples of the device-event time of {a.reps} back-to-back calls / {a.reps}, "
                     "the three routes interleaved; median, min, p90 in ms per call; wide_wins: wide median < tile median and wide p90 < tile min"}
    res["actor"] = [actor_piece(o, c, h, 100_000, eng, a) for o, c, h in ACTOR_SHAPES]
    res["critic"] = [critic_piece(o, c, h, 10_000, eng, a) for o, c, h in CRITIC_SHAPES]
    res["populate"] = populate_piece(100_000, eng, 10)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print("\n| kernel | obs / act / hidden | tile (median, min..p90) | wide | torch | wide wins |\n|---|---|---|---|---|---|")
    cell = lambda s: f"{s['median']:.3f} ({s['min']:.3f}..{s['p90']:.3f})"  # noqa: E731
    for who, other in (("actor", "torch_policy_sample"), ("critic", "torch_live_critic_min")):
        for r in res[who]:
            sh = r["shape"]
            print(f"| {who} | {sh['obs']} / {sh['act']} / {sh['hidden']} | {cell(r['ms']['tile'])} | {cell(r['ms']['wide'])} | {cell(r['ms'][other])} | {r['wide_wins']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
