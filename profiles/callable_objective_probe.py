"""What one objective evaluation costs when the reward (and termination) are Python callables, on one MI355X:
    python profiles/callable_objective_probe.py --out profiles/callable_objective.json
Shapes: cfg2 (BASELINE.json configs[1]: obs 17, act 6, E 5, hid 200 x 4 SiLU, pop 500, P 20, H 30; the halfcheetah reward as a Python
callable) and the one-tile cfg1 (configs[0]: obs 4, act 1, pop 100, P 5, H 15; the cartpole reward and termination as Python callables),
DEVICE mode.  Per shape, ms per objective evaluation:
  (a) hipets.UnfusedTrajectoryEvalFn: H hipets_step launches with the callables and the masking as torch ops in between (the baseline);
  (b) hipets.CallableTrajectoryEvalFn: one tapped rollout launch, the callables once over H * B rows, hipets_trajectory_returns --
      the whole call, and its three parts on their own;
  (c) hipets.HipTrajectoryEvalFn on the same model with the closed forms fused (what a RewardTerms table would buy);
  and the rollout launch on the hidden-static / generic instance (generic_kernel=2) with and without the two taps: the taps' stores.
Every figure: device events around `reps` back-to-back evaluations after a warm-up (the events see the gaps a host-bound loop leaves
on the stream, so for (a) they equal the wall time), the variants interleaved over `repeats` rounds in one process; median, min, max."""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "mbrl-lib_amd"))
sys.path.insert(0, ROOT)


def halfcheetah_reward(act, next_obs):  # mbrl/env/reward_fns.py:33-38 as a user would write it
    return (next_obs[:, 0] - 0.1 * act.square().sum(dim=1)).unsqueeze(1)


def cartpole_termination(act, next_obs):  # mbrl/env/termination_fns.py:29-44
    x, theta = next_obs[:, 0], next_obs[:, 2]
    thr = 12 * 2 * 3.141592653589793 / 360
    return ~((x > -2.4) & (x < 2.4) & (theta > -thr) & (theta < thr)).unsqueeze(1)


def cartpole_reward(act, next_obs):  # mbrl/env/reward_fns.py:10-13
    return (~cartpole_termination(act, next_obs)).float()


def time_ms(f, reps, warmup):
    """(device-event ms, wall ms) per call of f over `reps` back-to-back calls"""
    import torch

    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3 / reps


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": len(v)}


def shape(name, spec_kw, reward_fn, termination_fn, pop, P, H, a):
    import numpy as np
    import torch

    import bench
    import hipets
    from hipets.objectives import closed_form_dones

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    fused_spec = bench.synthetic_spec(dev, **spec_kw)
    obs, act = fused_spec.obs_dim, fused_spec.act_dim
    py_spec = dataclasses.replace(fused_spec, reward="none", termination="no_termination")
    B = pop * P
    g = torch.Generator().manual_seed(0)
    actions = (torch.rand(pop, H, act, generator=g) * 2 - 1).to(dev)
    s0 = np.zeros(obs, np.float32)
    unfused = hipets.UnfusedTrajectoryEvalFn(py_spec, P, reward_fn=reward_fn, termination_fn=termination_fn, engine=eng, seed=1)
    new = hipets.CallableTrajectoryEvalFn(py_spec, P, reward_fn=reward_fn, termination_fn=termination_fn, engine=eng, seed=1)
    fused = hipets.HipTrajectoryEvalFn(fused_spec, P, engine=eng, seed=1)
    # the parts of (b) on buffers of their own
    tno = torch.empty(H, B, obs, device=dev)
    trw = torch.empty(H, B, device=dev)
    rewards = torch.randn(H, B, device=dev)
    dones = torch.rand(H, B, device=dev) < 0.02
    act_rows = actions.transpose(0, 1).unsqueeze(2).expand(H, pop, P, act).reshape(H * B, act)
    stream = [100]

    def rollout(spec, **kw):
        def f():
            if eng.spec is not spec:
                eng.set_model(spec)
            stream[0] += 1
            eng.rollout(actions, s0, P, mode="device", seed=1, stream_id=stream[0], **kw)
        return f

    def callables():
        rows = tno.view(H * B, obs)
        actions.transpose(0, 1).unsqueeze(2).expand(H, pop, P, act).reshape(H * B, act)  # (the objective builds act_rows per call)
        r = reward_fn(act_rows, rows).reshape(H, B).contiguous()
        d = (termination_fn(act_rows, rows) if termination_fn is not None else closed_form_dones(py_spec, rows)).reshape(H, B).contiguous()
        return r, d

    variants = {
        "a_unfused_objective": lambda: unfused(s0, actions),
        "b_callable_objective": lambda: new(s0, actions),
        "b1_tapped_rollout_launch": rollout(py_spec, trace_next_obs=tno, trace_rewards=trw),
        "b2_callables_over_all_rows": callables,
        "b3_trajectory_returns": lambda: eng.trajectory_returns(rewards, dones, pop, P),
        "c_fused_objective": lambda: fused(s0, actions),
        "rollout_generic_kernel_2_untapped": rollout(fused_spec, generic_kernel=2),
        "rollout_generic_kernel_2_tapped": rollout(fused_spec, generic_kernel=2, trace_next_obs=tno, trace_rewards=trw),
    }
    ev = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            e, w = time_ms(f, a.reps, a.warmup)
            ev[k].append(e)
            wall[k].append(w)
    med = {k: statistics.median(v) for k, v in ev.items()}
    res = {"shape": dict(name=name, obs=obs, act=act, pop=pop, P=P, H=H, rows=B, trajectory_bytes=H * B * (obs + 1) * 4, model=spec_kw),
           "kernel_class_of_a_default_call": eng.kernel_class(pop, P, H, "device")[0],
           "device_event_ms_per_evaluation": {k: stats(v) for k, v in ev.items()},
           "wall_ms_per_evaluation": {k: stats(v) for k, v in wall.items()},
           "b_over_a": med["b_callable_objective"] / med["a_unfused_objective"],
           "b_over_c": med["b_callable_objective"] / med["c_fused_objective"],
           "sum_of_b_parts_ms": med["b1_tapped_rollout_launch"] + med["b2_callables_over_all_rows"] + med["b3_trajectory_returns"],
           "tap_stores_share_of_launch": (med["rollout_generic_kernel_2_tapped"] - med["rollout_generic_kernel_2_untapped"]) / med["rollout_generic_kernel_2_tapped"]}
    return res


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower()][:16]
    except Exception as exc:  # the tool is optional
        return [f"not available: {exc}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import bench

    if not torch.cuda.is_available():
        print("callable_objective_probe.py needs a GPU: nothing measured", file=sys.stderr)
        return 1
    res = {"device": torch.cuda.get_device_name(0), "clocks_before": clocks(),
           "method": f"device events around {a.reps} back-to-back evaluations after {a.warmup} warm-up calls, variants interleaved, {a.repeats} rounds"}
    res["cfg2"] = shape("cfg2", {}, halfcheetah_reward, None, bench.POP, bench.PARTICLES, bench.HORIZON, a)
    c1 = bench.OTHER_CONFIGS["configs[0] cfg1 cartpole"]
    res["cfg1"] = shape("cfg1", dict(c1["model"]), cartpole_reward, cartpole_termination, c1["pop"], c1["P"], c1["H"], a)
    res["clocks_after"] = clocks()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
