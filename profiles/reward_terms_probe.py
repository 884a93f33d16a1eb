"""What a reward term table / healthy box (hipets.RewardTerms, hipets.BoxTermination) costs, at the cfg2 shape on one MI355X:
    python profiles/reward_terms_probe.py --out profiles/reward_terms.json [--parent-tree <checkout of the parent commit, built>]
(a) rollout   one DEVICE rollout on the hidden-static instance (generic_kernel=2), the library's hipEvent timing: reward="halfcheetah"
              (the enum), the same reward as a 7-term table, and a stress table (64 terms + a 64-interval box that every row passes);
              the variants interleaved in ONE process (clock and thermal drift hit all alike).  With --parent-tree the enum variant is
              also measured on that tree's library, in child processes alternating with this tree's: the enum cases compile to the same
              code, so the two must agree within the box-to-box spread.
(b) plan      the cfg2 CEM plan (bench.py's: 5 iterations) with the reward as a RewardTerms object (fused: one hipets_plan_cem call) and
              as an ordinary Python callable through UnfusedTrajectoryEvalFn (one hipets_step launch + torch ops per horizon step);
              host clock around synchronised plans.
(c) headline  bench.py, run not edited, on this tree and on --parent-tree, alternating.
--enum-only --tree DIR: the enum variant of (a) alone with the package of DIR (what the parent tree is asked to run)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def use_tree(tree):
    sys.path.insert(0, os.path.join(tree, "mbrl-lib_amd"))
    sys.path.insert(0, tree)


def measure(eng, spec, actions, reps, warmup=3, stream0=10):
    """rollout-kernel ms per DEVICE rollout on the hidden-static instance, from the library's hipEvents"""
    import numpy as np
    import torch

    import bench

    s0 = np.zeros(bench.OBS, np.float32)
    eng.set_model(spec)
    eng.timing_enable(False)
    for i in range(warmup):
        eng.rollout(actions, s0, bench.PARTICLES, mode="device", seed=1, stream_id=i, generic_kernel=2)
    eng.timing_enable(True)
    eng.timing_read(reset=True)
    for i in range(reps):
        eng.rollout(actions, s0, bench.PARTICLES, mode="device", seed=1, stream_id=stream0 + i, generic_kernel=2)
    n, ms = eng.timing_read(reset=True)
    eng.timing_enable(False)
    torch.cuda.synchronize()
    return ms / reps


def stats(ms):
    lo, med, hi = min(ms), statistics.median(ms), max(ms)
    return {"min": lo, "median": med, "max": hi, "spread_rel": (hi - lo) / med, "samples": len(ms)}


def rollout_block(a, enum_only):
    import torch

    import bench
    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    g = torch.Generator().manual_seed(0)
    actions = (torch.rand(bench.POP, bench.HORIZON, bench.ACT, generator=g) * 2 - 1).to(dev)
    specs = {"enum": bench.synthetic_spec(dev)}
    if not enum_only:
        import dataclasses
        import math

        from hipets import BoxTermination, Interval, RewardTerm, RewardTerms

        table = [RewardTerm("linear", 0)] + [RewardTerm("square", i, w=-0.1, source="act") for i in range(bench.ACT)]
        specs["table_7_terms"] = dataclasses.replace(specs["enum"], reward=RewardTerms(table))
        stress = table + [RewardTerm("abs", i % bench.OBS, w=0.0, j=(i + 1) % bench.OBS) for i in range(64 - len(table))]
        box = BoxTermination([Interval(i % bench.OBS, -math.inf, math.inf) for i in range(64)], require_finite=True)
        specs["table_64_terms_box_64_intervals"] = dataclasses.replace(specs["enum"], reward=RewardTerms(stress), termination=box)
    ms = {k: [] for k in specs}
    for r in range(a.repeats):
        for k, spec in specs.items():
            ms[k].append(measure(eng, spec, actions, a.reps, stream0=100 * r + 10))
    eng.set_model(specs["enum"])
    cls = list(eng.kernel_class(bench.POP, bench.PARTICLES, bench.HORIZON, mode="device"))
    out = {"workload": f"cfg2: obs {bench.OBS}, act {bench.ACT}, E {bench.ENSEMBLE}, pop {bench.POP} x {bench.PARTICLES} particles, H {bench.HORIZON}, "
                       "one DEVICE rollout, generic_kernel=2 (hidden-static instance)", "default_call_kernel_class": cls,
           "repeats": a.repeats, "rollouts_per_repeat": a.reps, "rollout_kernel_ms": {k: stats(v) for k, v in ms.items()}}
    if not enum_only:
        e = out["rollout_kernel_ms"]["enum"]["median"]
        out["ratio_over_enum"] = {k: out["rollout_kernel_ms"][k]["median"] / e for k in specs if k != "enum"}
    return out, specs


def plan_block(a, spec_table):
    """ms per cfg2 CEM plan: the term table fused, against the same reward as a Python callable on the unfused path"""
    import dataclasses

    import numpy as np
    import torch

    import bench
    import hipets
    from hipets.planning import _BoundObjective

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    lb, ub = [[-1.0] * bench.ACT] * bench.HORIZON, [[1.0] * bench.ACT] * bench.HORIZON
    obs = np.zeros(bench.OBS, np.float32)
    x0 = torch.zeros(bench.HORIZON, bench.ACT)

    def halfcheetah(act, next_obs):  # an ordinary user function: nothing the library recognises
        return (next_obs[:, 0] - 0.1 * act.square().sum(dim=1)).view(-1, 1)

    fns = {"fused_reward_terms": hipets.make_eval_fn(spec_table, bench.PARTICLES, engine=eng, seed=3, mode="device"),
           "unfused_python_callable": hipets.UnfusedTrajectoryEvalFn(dataclasses.replace(spec_table, reward="none"), bench.PARTICLES, reward_fn=halfcheetah,
                                                                     engine=eng, seed=3)}
    out = {}
    for name, fn in fns.items():
        opt = hipets.CEMOptimizer(bench.ITERS, bench.ELITE_RATIO, bench.POP, lb, ub, bench.ALPHA, dev, seed=5)
        obj = _BoundObjective(fn, obs)
        n = a.plans if name.startswith("fused") else max(3, a.plans // 5)
        for _ in range(2):
            opt.optimize(obj, x0=x0)
        torch.cuda.synchronize()
        times = []
        for _ in range(n):
            t0 = time.perf_counter()
            plan = opt.optimize(obj, x0=x0)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        assert torch.isfinite(plan).all()
        out[name] = {"ms_per_plan": stats(times), "objective": type(fn).__name__}
    out["workload"] = f"cfg2 CEM plan: {bench.ITERS} iterations, pop {bench.POP} x {bench.PARTICLES} particles, H {bench.HORIZON}, hipets.CEMOptimizer"
    out["unfused_over_fused"] = out["unfused_python_callable"]["ms_per_plan"]["median"] / out["fused_reward_terms"]["ms_per_plan"]["median"]
    return out


def child_json(cmd, cwd):
    """the last JSON line a fresh child process prints"""
    proc = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)
    if proc.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({proc.returncode}): {proc.stderr[-2000:]}")
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--plans", type=int, default=30)
    ap.add_argument("--bench-steps", type=int, default=50)
    ap.add_argument("--bench-runs", type=int, default=2)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package runs (default: this one)")
    ap.add_argument("--enum-only", action="store_true", help="(a) with the enum reward alone: what a tree without the classes can run")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: the yardstick of (a)'s enum run and of (c)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    use_tree(os.path.abspath(a.tree))
    if a.enum_only:
        blk, _ = rollout_block(a, True)
        print(json.dumps(blk))
        return 0
    res = {}
    res["rollout"], specs = rollout_block(a, False)
    res["plan"] = plan_block(a, specs["table_7_terms"])
    if a.parent_tree:
        parent = os.path.abspath(a.parent_tree)
        me = [sys.executable, os.path.abspath(__file__), "--enum-only", "--repeats", str(a.repeats), "--reps", str(a.reps)]
        bench_cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "5", "--no-cpu-baseline", "--no-extras"]
        enum, head = {"this_tree": [], "parent_commit": []}, {"this_tree": [], "parent_commit": []}
        for _ in range(a.bench_runs):  # fresh child processes, the two trees alternating
            for who, tree in (("parent_commit", parent), ("this_tree", ROOT)):
                enum[who].append(child_json(me + ["--tree", tree], tree)["rollout_kernel_ms"]["enum"]["median"])
                line = child_json(bench_cmd, tree)
                head[who].append({"value": line["value"], "unit": line["unit"]})
        e_new, e_old = statistics.median(enum["this_tree"]), statistics.median(enum["parent_commit"])
        res["rollout"]["enum_in_child_processes_ms"] = dict(enum, this_over_parent=e_new / e_old)
        v_new, v_old = (statistics.median(h["value"] for h in head[k]) for k in ("this_tree", "parent_commit"))
        res["headline"] = {"command": " ".join(bench_cmd[1:]), "runs": head, "this_over_parent": v_new / v_old}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
