"""What policy-guided planning costs on one MI355X:
    python profiles/policy_rollout_probe.py --out profiles/policy_rollout.json
Kernel: hipets_policy_rollout (one launch) for mbpo_halfcheetah's pair -- the model 23-200x4-36 with 7 members / 5 elites, the SAC policy
17-512-512-6 -- at n in {24, 256} rows and H in {5, 10, 30}, against the two routes that existed before it on the same GPU:
  composed  per step hipets_policy_act + hipets_ensemble_predict + torch's mean over the members and add (2 H launches and torch glue)
  torch     the live modules: the policy's forward, the ensemble's matmuls over the elite members, mean(dim=0), add
Plan: a cfg2 CEM plan (BASELINE.json configs[1]: pop 500, P 20, 5 iterations) under hipets.ValueTrajectoryEvalFn (discount 0.99, a SAC
agent of hidden 256) at H = 5 and 10 through a TrajectoryOptimizerAgent, with and without a PolicyPrior of 24 rows; and what leaving the
one-call fused plan costs by itself: a plain hipets.HipTrajectoryEvalFn plan as the fused call against the same plan with
`callback=lambda *a: None`.  Plans end in their device -> host copy: a host clock around `agent.plan`.
Every kernel figure: 3 warm-up rounds, then 20 samples, each the device-event time of `reps` back-to-back calls / reps, the routes of a
group interleaved sample by sample in one process; median, min, p90 (value_objective_probe.measure).  Planning QUALITY with a prior is
not measured here."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "mbrl-lib_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import value_objective_probe as vp  # noqa: E402  (measure, make_agent)


def kernel_group(n, H, a):
    import torch
    import torch.nn.functional as F

    import bench
    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    spec = bench.synthetic_spec(dev, ensemble=7, elite=[0, 1, 2, 3, 4], learned_rewards=True)
    agent = vp.make_agent(17, 6, 512, dev)
    ro = hipets.PolicyRollout(spec, agent, engine=eng, seed=1)
    g = torch.Generator().manual_seed(4)
    s0 = (0.5 * torch.randn(n, 17, generator=g)).to(dev)
    eps = torch.randn(H, n, 6, generator=g).to(dev)
    members = list(spec.members)
    ws, bs = [w[members] for w in spec.weights], [b[members] for b in spec.biases]
    pol = agent.policy

    def fused():
        return ro.sequences(s0, horizon=H, mean_rows=1, eps=eps)

    def composed():
        s, out = s0, []
        for t in range(H):
            act = ro.actor.act_device(s, sample=True, eps=eps[t])
            act[:1] = ro.actor.act_device(s[:1], sample=False)
            mean = ro.predictor.predict(s, act, only_elite=True)[0]
            s = s + mean.mean(dim=0)[:, :17]
            out.append(act)
        return torch.stack(out, dim=1)

    @torch.no_grad()
    def torch_route():
        s, out = s0, []
        for t in range(H):
            h = F.relu(pol.linear2(F.relu(pol.linear1(s))))
            mean, log_std = pol.mean_linear(h), pol.log_std_linear(h).clamp(-20.0, 2.0)
            act = torch.tanh(mean + eps[t] * log_std.exp())
            act[:1] = torch.tanh(mean[:1])
            x = torch.cat([s, act], dim=1)  # (the synthetic normaliser is mean 0 / std 1)
            for l, (w, b) in enumerate(zip(ws, bs)):
                x = x.matmul(w) + b
                if l < len(ws) - 1:
                    x = F.silu(x)
            s = s + x[..., :17].mean(dim=0)
            out.append(act)
        return torch.stack(out, dim=1)

    diff = float((fused() - composed()).abs().max()), float((fused() - torch_route()).abs().max())
    assert diff[0] < 1e-3 and diff[1] < 1e-3, diff  # (a loose sanity bound on the three routes; the tests hold the real ones)
    res = vp.measure({"fused_policy_rollout": fused, "composed_2H_launches": composed, "torch_live_modules": torch_route}, a)
    r, lds = ro.geometry(n)
    return {"n": n, "H": H, "row_tiles": r, "lds_bytes": lds, "workgroups": -(-n // (16 * r)), "max_abs_diff_vs_torch": diff[1], "ms": res,
            "composed_over_fused": res["composed_2H_launches"]["median"] / res["fused_policy_rollout"]["median"],
            "torch_over_fused": res["torch_live_modules"]["median"] / res["fused_policy_rollout"]["median"]}


def wall_ms(f, samples, warmup):
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(samples):
        t = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t) * 1e3)
    s = sorted(ms)
    return {"median": statistics.median(s), "min": s[0], "p90": s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))], "samples": len(s)}


def plan_costs(a):
    import numpy as np
    import torch

    import bench
    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    spec = bench.synthetic_spec(dev)
    agent_sac = vp.make_agent(spec.obs_dim, spec.act_dim, 256, dev)
    obs = np.zeros(spec.obs_dim, np.float32)
    cfg = {"_target_": "hipets.CEMOptimizer", "num_iterations": bench.ITERS, "elite_ratio": bench.ELITE_RATIO, "population_size": bench.POP,
           "alpha": bench.ALPHA, "device": str(dev), "seed": 0}
    out = {"shape": dict(pop=bench.POP, P=bench.PARTICLES, iterations=bench.ITERS, agent_hidden=256, prior_rows=24), "ms_per_plan": {}}
    for H in (5, 10):
        planner = hipets.TrajectoryOptimizerAgent(cfg, [-1.0] * spec.act_dim, [1.0] * spec.act_dim, planning_horizon=H)
        planner.set_trajectory_eval_fn(hipets.ValueTrajectoryEvalFn(spec, bench.PARTICLES, agent=agent_sac, discount=0.99, engine=eng, seed=1))
        prior = hipets.PolicyPrior(spec, agent_sac, num=24, seed=2, engine=eng)
        out["ms_per_plan"][f"value_H{H}_no_prior"] = wall_ms(lambda: planner.plan(obs), a.samples, a.warmup)
        planner.set_policy_prior(prior)
        out["ms_per_plan"][f"value_H{H}_prior_24"] = wall_ms(lambda: planner.plan(obs), a.samples, a.warmup)
        plain = hipets.TrajectoryOptimizerAgent(cfg, [-1.0] * spec.act_dim, [1.0] * spec.act_dim, planning_horizon=H)
        plain.set_trajectory_eval_fn(hipets.HipTrajectoryEvalFn(spec, bench.PARTICLES, engine=eng, seed=1))
        out["ms_per_plan"][f"plain_H{H}_fused_one_call"] = wall_ms(lambda: plain.plan(obs), a.samples, a.warmup)
        loop = lambda: plain.optimizer.optimize(hipets.planning._BoundObjective(plain.trajectory_eval_fn, obs), callback=lambda *x: None)  # noqa: E731
        out["ms_per_plan"][f"plain_H{H}_per_iteration_loop"] = wall_ms(loop, a.samples, a.warmup)
        plain.set_policy_prior(hipets.PolicyPrior(spec, agent_sac, num=24, seed=2, engine=eng))
        out["ms_per_plan"][f"plain_H{H}_prior_24"] = wall_ms(lambda: plain.plan(obs), a.samples, a.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("policy_rollout_probe.py needs a GPU: nothing measured", file=sys.stderr)
        return 1
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"kernel: {a.warmup} warm-up rounds, then {a.samples} samples of the device-event time of {a.reps} back-to-back calls / {a.reps}, "
                     "routes interleaved; plans: a host clock around agent.plan (ends in its device -> host copy); median, min, p90 in ms"}
    res["kernel"] = [kernel_group(n, H, a) for n in (24, 256) for H in (5, 10, 30)]
    for k in res["kernel"]:
        print(json.dumps(k), flush=True)
    res["plan"] = plan_costs(a)
    print(json.dumps(res["plan"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
