"""What an observation column table (hipets.ObsColumns) costs, at the pets_halfcheetah-like cfg2 shape on one MI355X:
    python profiles/obs_columns_probe.py --out profiles/obs_columns.json [--parent-tree <checkout of the parent commit, built>]
(a) rollout   one DEVICE rollout on the hidden-static instance (generic_kernel=2), the library's hipEvent timing, obs 18 through the
              preprocessor: obs_process="halfcheetah" (the enum), the same preprocessor as an 18-column table, and two 64-column models
              (first layer 70 inputs wide instead of 24): every column id, and every column sin / cos (the stress table) -- their
              ratio is what 64 trig columns cost on top of a model of that width.  The variants interleaved in ONE process (clock and
              thermal drift hit all alike).  With --parent-tree the enum variant is also measured on that tree's library, in child
              processes alternating with this tree's: the enum path must agree within the box-to-box spread.
(b) headline  bench.py, run not edited, on this tree and on --parent-tree, alternating.
--enum-only --tree DIR: the enum variant of (a) alone with the package of DIR (what the parent tree is asked to run)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OBS = 18  # pets_halfcheetah: 18 observation dims through HalfCheetahEnv.preprocess_fn


def use_tree(tree):
    sys.path.insert(0, os.path.join(tree, "mbrl-lib_amd"))
    sys.path.insert(0, tree)


def measure(eng, spec, actions, reps, warmup=3, stream0=10):
    """rollout-kernel ms per DEVICE rollout on the hidden-static instance, from the library's hipEvents"""
    import numpy as np
    import torch

    import bench

    s0 = np.zeros(OBS, np.float32)
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


def widened(spec, table, dev):
    """`spec` with `table` as its preprocessor: a first layer (and normaliser) as wide as the table asks, same initialiser"""
    import dataclasses

    import numpy as np
    import torch

    E, n_in, hid = spec.ensemble_size, len(table.columns) + spec.act_dim, spec.hid
    std = 1.0 / (2.0 * np.sqrt(n_in))
    w = torch.empty(E, n_in, hid)
    torch.nn.init.trunc_normal_(w, mean=0.0, std=std, a=-2 * std, b=2 * std, generator=torch.Generator().manual_seed(1))
    return dataclasses.replace(spec, weights=[w.to(dev)] + list(spec.weights[1:]), obs_process=table,
                               norm_mean=torch.zeros(1, n_in, dtype=torch.float64), norm_std=torch.ones(1, n_in, dtype=torch.float64))


def rollout_block(a, enum_only):
    import torch

    import bench
    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    g = torch.Generator().manual_seed(0)
    actions = (torch.rand(bench.POP, bench.HORIZON, bench.ACT, generator=g) * 2 - 1).to(dev)
    specs = {"enum": bench.synthetic_spec(dev, obs=OBS, obs_process="halfcheetah")}
    if not enum_only:
        import dataclasses

        from hipets import ObsColumns

        specs["table_18_columns"] = dataclasses.replace(specs["enum"], obs_process=ObsColumns([(1, "id"), (2, "sin"), (2, "cos")] + [(d, "id") for d in range(3, OBS)]))
        specs["id_64_columns"] = widened(specs["enum"], ObsColumns([(k % OBS, "id") for k in range(64)]), dev)
        specs["trig_64_columns"] = widened(specs["enum"], ObsColumns([(k % OBS, ("sin", "cos")[(k // OBS) % 2]) for k in range(64)]), dev)
    ms = {k: [] for k in specs}
    for r in range(a.repeats):
        for k, spec in specs.items():
            ms[k].append(measure(eng, spec, actions, a.reps, stream0=100 * r + 10))
    eng.set_model(specs["enum"])
    cls = list(eng.kernel_class(bench.POP, bench.PARTICLES, bench.HORIZON, mode="device"))
    out = {"workload": f"cfg2-like halfcheetah: obs {OBS} through the preprocessor, act {bench.ACT}, E {bench.ENSEMBLE}, pop {bench.POP} x {bench.PARTICLES} particles, "
                       f"H {bench.HORIZON}, one DEVICE rollout, generic_kernel=2 (hidden-static instance)", "default_call_kernel_class": cls,
           "repeats": a.repeats, "rollouts_per_repeat": a.reps, "rollout_kernel_ms": {k: stats(v) for k, v in ms.items()}}
    if not enum_only:
        med = {k: out["rollout_kernel_ms"][k]["median"] for k in specs}
        out["ratios"] = {"table_18_columns_over_enum": med["table_18_columns"] / med["enum"],
                         "trig_64_columns_over_id_64_columns": med["trig_64_columns"] / med["id_64_columns"],
                         "trig_64_columns_over_enum": med["trig_64_columns"] / med["enum"]}
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
    ap.add_argument("--bench-steps", type=int, default=50)
    ap.add_argument("--bench-runs", type=int, default=2)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package runs (default: this one)")
    ap.add_argument("--enum-only", action="store_true", help="(a) with the enum preprocessor alone: what a tree without the class can run")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: the yardstick of (a)'s enum run and of (b)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    use_tree(os.path.abspath(a.tree))
    if a.enum_only:
        print(json.dumps(rollout_block(a, True)))
        return 0
    res = {"rollout": rollout_block(a, False)}
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
        res["rollout"]["enum_in_child_processes_ms"] = dict(enum, this_over_parent=e_new / e_old,
                                                            spread_rel={k: (max(v) - min(v)) / statistics.median(v) for k, v in enum.items()})
        v_new, v_old = (statistics.median(h["value"] for h in head[k]) for k in ("this_tree", "parent_commit"))
        res["headline"] = {"command": " ".join(bench_cmd[1:]), "runs": head, "this_over_parent": v_new / v_old,
                           "spread_rel": {k: (max(h["value"] for h in v) - min(h["value"] for h in v)) / statistics.median(h["value"] for h in v) for k, v in head.items()}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
