"""What value-bootstrapped planning costs on one MI355X, piece by piece and as a whole evaluation:
    python profiles/value_objective_probe.py --out profiles/value_objective.json
Pieces, at 10 000 rows (cfg2: pop 500 x P 20), device events:
  critic      hipets_critic_q (one launch: q1, q2, qmin) against the live torch module's `torch.min(*critic(s, a))` -- the only route
              the library had before -- for obs 17 / act 6 with hidden 256 and 512, and obs 376 / act 17 with hidden 1024;
  returns     hipets_discounted_returns against a torch discounted sum with the same termination select and bootstrap over the same
              [H, rows] buffers, H in {5, 10, 30}.
Whole evaluation at cfg2 (BASELINE.json configs[1]: obs 17, act 6, E 5, hid 200 x 4, pop 500, P 20), DEVICE mode: one
hipets.ValueTrajectoryEvalFn call with a SAC agent of hidden 256 at H in {5, 10, 30}, the same without an agent (discounting alone),
and hipets.HipTrajectoryEvalFn at the same horizons -- H = 30 is what the short-horizon-plus-value route replaces.
Every figure: 3 warm-up rounds, then 20 samples, each the device-event time of `reps` back-to-back calls divided by `reps`, the variants
of a group interleaved sample by sample in one process; median, min, p90.  Planning quality at short horizons is not measured here."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "mbrl-lib_amd"))
sys.path.insert(0, ROOT)


def event_ms(f, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(variants, a):
    """{name: {median, min, p90, samples}} in ms per call, the variants interleaved"""
    import torch

    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.samples):
        for k, f in variants.items():
            ms[k].append(event_ms(f, a.reps))
    out = {}
    for k, v in ms.items():
        s = sorted(v)
        out[k] = {"median": statistics.median(s), "min": s[0], "p90": s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))], "samples": len(s)}
    return out


def make_agent(obs, act, hid, dev, seed=0):
    """A SAC-shaped agent (Gaussian policy, twin critic and its target) with torch's default initialisation"""
    import torch
    from types import SimpleNamespace

    torch.manual_seed(seed)

    class Twin(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for j in (1, 4):
                setattr(self, f"linear{j}", torch.nn.Linear(obs + act, hid))
                setattr(self, f"linear{j + 1}", torch.nn.Linear(hid, hid))
                setattr(self, f"linear{j + 2}", torch.nn.Linear(hid, 1))

        def forward(self, state, action):
            xu = torch.cat([state, action], 1)
            relu = torch.nn.functional.relu
            return (self.linear3(relu(self.linear2(relu(self.linear1(xu))))), self.linear6(relu(self.linear5(relu(self.linear4(xu))))))

    policy = torch.nn.Module()
    policy.linear1, policy.linear2 = torch.nn.Linear(obs, hid), torch.nn.Linear(hid, hid)
    policy.mean_linear, policy.log_std_linear = torch.nn.Linear(hid, act), torch.nn.Linear(hid, act)
    policy.action_scale, policy.action_bias = torch.ones(act, device=dev), torch.zeros(act, device=dev)
    return SimpleNamespace(policy=policy.to(dev), critic=Twin().to(dev), critic_target=Twin().to(dev))


def critic_piece(obs, act, hid, rows, a):
    import torch

    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    agent = make_agent(obs, act, hid, dev)
    crit = hipets.SACCritic(agent, engine=eng)
    g = torch.Generator().manual_seed(1)
    s, u = torch.randn(rows, obs, generator=g).to(dev), (torch.rand(rows, act, generator=g) * 2 - 1).to(dev)

    def torch_route():
        with torch.no_grad():
            return torch.min(*agent.critic(s, u))

    q_hip, q_torch = crit.q(s, u)[2], torch_route().reshape(-1)
    res = measure({"hip_critic_q": lambda: crit.q(s, u), "hip_critic_q_qmin_only": lambda: crit.q(s, u, q1=False, q2=False),
                   "torch_live_critic_min": torch_route}, a)
    r, lds = eng.critic_geometry(rows)
    return {"shape": dict(obs=obs, act=act, hidden=hid, rows=rows), "row_tiles": r, "lds_bytes": lds, "workgroups": -(-rows // (16 * r)),
            "max_abs_diff_hip_vs_torch": float((q_hip - q_torch).abs().max()), "ms": res,
            "hip_over_torch": res["hip_critic_q"]["median"] / res["torch_live_critic_min"]["median"]}


def returns_piece(H, pop, P, a):
    import torch

    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    eng.set_particle_reduce(hipets.ParticleReduce.mean())
    B, gamma = pop * P, 0.99
    g = torch.Generator().manual_seed(2)
    rewards = torch.randn(H, B, generator=g).to(dev)
    dones = (torch.rand(H, B, generator=g) < 0.02).to(dev)
    values = torch.randn(B, generator=g).to(dev)
    disc = (gamma ** torch.arange(H, dtype=torch.float32)).to(dev)[:, None]
    zero = torch.zeros((), device=dev)

    def torch_route():
        before = (dones.cumsum(0) - dones.to(torch.int64)) > 0  # terminated at an earlier step
        tot = (torch.where(before, zero, rewards) * disc).sum(0) + torch.where(dones.any(0), zero, (gamma ** H) * values)
        return tot.view(pop, P).mean(1)

    hip = lambda: eng.discounted_returns(rewards, dones, pop, P, gamma=gamma, terminal_values=values)  # noqa: E731
    diff = float((hip() - torch_route()).abs().max())
    res = measure({"hip_discounted_returns": hip, "torch_discounted_sum": torch_route,
                   "hip_trajectory_returns": lambda: eng.trajectory_returns(rewards, dones, pop, P)}, a)
    return {"shape": dict(H=H, pop=pop, P=P, rows=B), "max_abs_diff_hip_vs_torch": diff, "ms": res,
            "hip_over_torch": res["hip_discounted_returns"]["median"] / res["torch_discounted_sum"]["median"]}


def whole_evaluation(a):
    import numpy as np
    import torch

    import bench
    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    spec = bench.synthetic_spec(dev)
    obs, act, pop, P = spec.obs_dim, spec.act_dim, bench.POP, bench.PARTICLES
    agent = make_agent(obs, act, 256, dev)
    s0 = np.zeros(obs, np.float32)
    out = {"shape": dict(obs=obs, act=act, pop=pop, P=P, agent_hidden=256, mode="device", discount=0.99), "ms_per_evaluation": {}}
    g = torch.Generator().manual_seed(3)
    # one group per horizon: a group holds ONE objective with the agent, so its actor and critic stay the engine's owners (two of
    # them taking turns would re-snapshot the weights at every call, which no planner does)
    for H in (5, 10, 30):
        actions = (torch.rand(pop, H, act, generator=g) * 2 - 1).to(dev)
        value = hipets.ValueTrajectoryEvalFn(spec, P, agent=agent, discount=0.99, engine=eng, seed=1)
        disc_only = hipets.ValueTrajectoryEvalFn(spec, P, discount=0.99, engine=eng, seed=1)
        fused = hipets.HipTrajectoryEvalFn(spec, P, engine=eng, seed=1)
        out["ms_per_evaluation"].update(measure({f"value_objective_H{H}": lambda: value(s0, actions),
                                                 f"discount_only_H{H}": lambda: disc_only(s0, actions),
                                                 f"fused_undiscounted_H{H}": lambda: fused(s0, actions)}, a))
    med = {k: v["median"] for k, v in out["ms_per_evaluation"].items()}
    out["value_H5_over_fused_H30"] = med["value_objective_H5"] / med["fused_undiscounted_H30"]
    out["value_H10_over_fused_H30"] = med["value_objective_H10"] / med["fused_undiscounted_H30"]
    out["value_H30_over_fused_H30"] = med["value_objective_H30"] / med["fused_undiscounted_H30"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("value_objective_probe.py needs a GPU: nothing measured", file=sys.stderr)
        return 1
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"{a.warmup} warm-up rounds, then {a.samples} samples of the device-event time of {a.reps} back-to-back calls / {a.reps}, "
                     "variants interleaved; median, min, p90 in ms per call"}
    res["critic"] = [critic_piece(o, c, h, 10000, a) for o, c, h in ((17, 6, 256), (17, 6, 512), (376, 17, 1024))]
    res["discounted_returns"] = [returns_piece(H, 500, 20, a) for H in (5, 10, 30)]
    res["whole_evaluation_cfg2"] = whole_evaluation(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
