"""What a reduction over the particles other than the mean costs a plan, on one MI355X:
    python profiles/particle_reduce_probe.py --out profiles/particle_reduce.json
The cfg2 CEM plan of bench.py (obs 17, act 6, E 5, hid 200 x 4 SiLU, pop 500, P 20, H 30, 5 iterations; the default DEVICE mode, the fused
hipets_plan_cem) under each kind of hipets.ParticleReduce against `mean` on this build, and the rule alone (Engine.particle_reduce at
pop 500, P 20: one particle_mean_kernel launch).  Every (kind, round) is a child process of its own under its own `timeout`, the kinds
interleaved over `rounds` rounds, so a drift of the machine hits every kind alike; a child times `steps` back-to-back plans (and
`steps * 20` launches of the rule) between device events after a warm-up.  Median, min and max over the rounds, and the ratio of the
medians to the mean's."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "mbrl-lib_amd"))
sys.path.insert(0, ROOT)

KINDS = ["mean", "mean_std", "min", "max", "worst_k_1", "worst_k_4", "worst_k_10", "worst_k_20"]


def reduction(name):
    import hipets

    R = hipets.ParticleReduce
    if name.startswith("worst_k_"):
        return R.worst_k(int(name[8:]))
    return {"mean": R.mean(), "mean_std": R.mean_std(1.0), "min": R.worst_case(), "max": R.best_case()}[name]


def child(a):
    import numpy as np
    import torch

    import bench
    import hipets
    from hipets.planning import _BoundObjective

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    spec = bench.synthetic_spec(dev)
    red = reduction(a.kind)
    fn = hipets.make_eval_fn(spec, bench.PARTICLES, engine=eng, seed=0, particle_reduce=red)
    lb, ub = [[-1.0] * spec.act_dim] * bench.HORIZON, [[1.0] * spec.act_dim] * bench.HORIZON
    opt = hipets.CEMOptimizer(bench.ITERS, bench.ELITE_RATIO, bench.POP, lb, ub, bench.ALPHA, dev, return_mean_elites=True, seed=0)
    obj = _BoundObjective(fn, np.zeros(spec.obs_dim, np.float32))
    x0 = torch.zeros(bench.HORIZON, spec.act_dim, device=dev)
    totals = torch.randn(bench.POP * bench.PARTICLES, device=dev) * 100

    def timed(f, reps, warmup):
        for _ in range(warmup):
            f()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / reps

    plan_ms = timed(lambda: opt.optimize(obj, x0=x0), a.steps, a.warmup)
    assert eng.reduce == red
    rule_us = 1e3 * timed(lambda: eng.particle_reduce(totals, bench.POP, bench.PARTICLES), a.steps * 20, a.warmup * 20)
    print(json.dumps({"kind": a.kind, "plan_ms": plan_ms, "rule_launch_us": rule_us}))
    return 0


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=120, help="seconds; a child that exceeds it ends the probe")
    ap.add_argument("--kind", default="", help="(child processes) the one reduction to time")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.kind:
        return child(a)
    plan, rule = {k: [] for k in KINDS}, {k: [] for k in KINDS}
    for _ in range(a.rounds):
        for k in KINDS:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--kind", k, "--steps", str(a.steps),
                   "--warmup", str(a.warmup)]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:  # nothing more is started on the GPU after a child that failed or ran out of time
                print(proc.stdout[-2000:], proc.stderr[-2000:], file=sys.stderr)
                return proc.returncode
            rec = json.loads(proc.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), file=sys.stderr, flush=True)  # (progress)
            plan[k].append(rec["plan_ms"])
            rule[k].append(rec["rule_launch_us"])
    base = statistics.median(plan["mean"])
    res = {"workload": "bench.py cfg2 CEM plan (pop 500, P 20, H 30, 5 iterations), default DEVICE mode, fused hipets_plan_cem",
           "method": f"{a.rounds} rounds, the kinds interleaved, one child process per (kind, round); device events around {a.steps} plans after "
                     f"{a.warmup} warm-up plans, and around {a.steps * 20} Engine.particle_reduce launches (pop 500, P 20)",
           "plan_ms": {k: stats(v) for k, v in plan.items()},
           "plan_ms_median_over_mean": {k: statistics.median(v) / base for k, v in plan.items()},
           "mean_run_to_run_spread": (max(plan["mean"]) - min(plan["mean"])) / base,
           "rule_launch_us": {k: stats(v) for k, v in rule.items()}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
