"""What reward tables with grouped terms (hipets.RewardTerms with level / op / 'group' / 'const' / sin, cos, exp, sqrt) cost, and that
a user of the flat ABI v9 table or of an enum reward does not pay for them, on one MI355X:
    python profiles/reward_groups_probe.py --out profiles/reward_groups.json --parent-tree <checkout of the parent commit, built>
(a) cfg2 shape, one DEVICE rollout on the hidden-static instance (generic_kernel=2), reward="halfcheetah" (the enum);
(b) the same reward as the v9 7-term table -- both on this tree and on --parent-tree, fresh child processes, the two trees alternating;
(c) bench.py headline, run not edited, on both trees, alternating.
    For (a)-(c) this / parent may exceed 1 by at most the parent's own run-to-run spread recorded here plus 1 % (the box-to-box spread
    DESIGN sections 15 / 16 report): "within_bound" in the output, exit status 1 otherwise.
(d) cartpole_pets as the enum against its grouped 9-entry table at the cfg1 shape (obs 4, act 1, pop 100 x 5, H 15) on the generic
    instance (generic_kernel=True);
(e) the custom form of tests/test_gpu_reward_groups.py (18 + 3 entries at act 6) at cfg2 against the enum -- (d) and (e) are reported only.
--child --tree DIR --variants a,b: the named variants of (a) / (b) with the package of DIR (what each child process runs)."""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def use_tree(tree):
    sys.path.insert(0, os.path.join(tree, "mbrl-lib_amd"))
    sys.path.insert(0, tree)


def measure(eng, spec, actions, s0, particles, reps, generic_kernel, warmup=3, stream0=10):
    """rollout-kernel ms per DEVICE rollout, from the library's hipEvents"""
    import torch

    eng.set_model(spec)
    eng.timing_enable(False)
    for i in range(warmup):
        eng.rollout(actions, s0, particles, mode="device", seed=1, stream_id=i, generic_kernel=generic_kernel)
    eng.timing_enable(True)
    eng.timing_read(reset=True)
    for i in range(reps):
        eng.rollout(actions, s0, particles, mode="device", seed=1, stream_id=stream0 + i, generic_kernel=generic_kernel)
    n, ms = eng.timing_read(reset=True)
    eng.timing_enable(False)
    torch.cuda.synchronize()
    return ms / reps


def stats(ms):
    lo, med, hi = min(ms), statistics.median(ms), max(ms)
    return {"min": lo, "median": med, "max": hi, "spread_rel": (hi - lo) / med, "samples": len(ms)}


def interleaved(a, specs, pop, horizon, particles, act, obs, generic_kernel):
    """the variants interleaved in ONE process (clock and thermal drift hit all alike) -> {variant: [ms per repeat]}"""
    import numpy as np
    import torch

    import hipets

    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    g = torch.Generator().manual_seed(0)
    actions = (torch.rand(pop, horizon, act, generator=g) * 2 - 1).to(dev)
    s0 = np.zeros(obs, np.float32)
    ms = {k: [] for k in specs}
    for r in range(a.repeats):
        for k, spec in specs.items():
            ms[k].append(measure(eng, spec, actions, s0, particles, a.reps, generic_kernel, stream0=100 * r + 10))
    return ms


def cfg2_specs(names):
    import torch

    import bench
    from hipets import RewardTerm, RewardTerms

    enum = bench.synthetic_spec(torch.device("cuda:0"))
    out = {}
    for n in names:
        if n == "enum":
            out[n] = enum
        elif n == "table_v9_7_terms":  # only the six v9 fields: what the parent commit's RewardTerm takes too
            out[n] = dataclasses.replace(enum, reward=RewardTerms([RewardTerm("linear", 0)] + [RewardTerm("square", i, w=-0.1, source="act") for i in range(bench.ACT)]))
        elif n == "custom_form":
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import reward_group_forms as forms

            body = [t for t in forms.CUSTOM_ENTRIES if t.source != "act"][:-1]
            table = body + [RewardTerm("square", i, source="act", level=1) for i in range(bench.ACT)] + [forms.CUSTOM_ENTRIES[-1]]
            out[n] = dataclasses.replace(enum, reward=RewardTerms(table, bias=forms.CUSTOM_BIAS))
        else:
            raise ValueError(n)
    return out


def child(a):
    import bench

    ms = interleaved(a, cfg2_specs(a.variants.split(",")), bench.POP, bench.HORIZON, bench.PARTICLES, bench.ACT, bench.OBS, 2)
    print(json.dumps({k: statistics.median(v) for k, v in ms.items()}))
    return 0


def child_json(cmd, cwd):
    """the last JSON line a fresh child process prints"""
    proc = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)
    if proc.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({proc.returncode}): {proc.stderr[-2000:]}")
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def against_parent(samples):
    """{this_tree: [..], parent_commit: [..]} -> the ratio of the medians, the parent's own spread, the bound and the verdict"""
    new, old = statistics.median(samples["this_tree"]), statistics.median(samples["parent_commit"])
    spread = (max(samples["parent_commit"]) - min(samples["parent_commit"])) / old
    return dict(samples, this_over_parent=new / old, parent_spread_rel=spread, bound=1.0 + spread + 0.01, within_bound=new / old <= 1.0 + spread + 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bench-steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3, help="child processes per tree for (a) / (b) and bench.py runs per tree for (c)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package runs (default: this one)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--variants", default="enum,table_v9_7_terms")
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: the yardstick of (a) - (c)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    use_tree(os.path.abspath(a.tree))
    if a.child:
        return child(a)
    import torch

    import bench
    from hipets import RewardTerms

    res = {"conditions": "(a)-(c): this / parent <= 1 + the parent's own run-to-run spread + 0.01"}
    ok = True
    if a.parent_tree:
        parent = os.path.abspath(a.parent_tree)
        me = [sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats), "--reps", str(a.reps)]
        bench_cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "5", "--no-cpu-baseline", "--no-extras"]
        roll = {v: {"this_tree": [], "parent_commit": []} for v in ("enum", "table_v9_7_terms")}
        head = {"this_tree": [], "parent_commit": []}
        for _ in range(a.runs):  # fresh child processes, the two trees alternating
            for who, tree in (("parent_commit", parent), ("this_tree", ROOT)):
                got = child_json(me + ["--tree", tree], tree)
                for v in roll:
                    roll[v][who].append(got[v])
                head[who].append(child_json(bench_cmd, tree)["value"])
        res["a_enum_rollout_ms"] = against_parent(roll["enum"])
        res["b_v9_table_rollout_ms"] = against_parent(roll["table_v9_7_terms"])
        res["c_headline"] = dict(against_parent({k: [1.0 / v for v in vs] for k, vs in head.items()}), command=" ".join(bench_cmd[1:]),
                                 values=head, note="samples are 1 / value, so that smaller is better as in (a) and (b)")
        res["workload_abc"] = (f"cfg2: obs {bench.OBS}, act {bench.ACT}, E {bench.ENSEMBLE}, pop {bench.POP} x {bench.PARTICLES} particles, H {bench.HORIZON}, one DEVICE "
                               f"rollout, generic_kernel=2 (hidden-static instance); median of {a.repeats} x {a.reps} rollouts per child process")
        ok = all(res[k]["within_bound"] for k in ("a_enum_rollout_ms", "b_v9_table_rollout_ms", "c_headline"))
    # (d) cartpole_pets: enum against its grouped table, cfg1 shape, generic instance
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import reward_group_forms as forms

    cfg1 = bench.OTHER_CONFIGS["configs[0] cfg1 cartpole"]
    enum = bench.synthetic_spec(torch.device("cuda:0"), obs=4, act=1, ensemble=5, reward="cartpole_pets")
    ms = interleaved(a, {"enum": enum, "grouped_table_9_entries": dataclasses.replace(enum, reward=forms.cartpole_pets_terms())},
                     cfg1["pop"], cfg1["H"], cfg1["P"], 1, 4, True)
    res["d_cartpole_pets_cfg1_generic_ms"] = {k: stats(v) for k, v in ms.items()}
    res["d_cartpole_pets_cfg1_generic_ms"]["table_over_enum"] = statistics.median(ms["grouped_table_9_entries"]) / statistics.median(ms["enum"])
    # (e) the custom form at cfg2, hidden-static instance
    ms = interleaved(a, cfg2_specs(["enum", "table_v9_7_terms", "custom_form"]), bench.POP, bench.HORIZON, bench.PARTICLES, bench.ACT, bench.OBS, 2)
    res["e_custom_form_cfg2_ms"] = {k: stats(v) for k, v in ms.items()}
    res["e_custom_form_cfg2_ms"]["custom_over_enum"] = statistics.median(ms["custom_form"]) / statistics.median(ms["enum"])
    res["e_custom_form_cfg2_ms"]["v9_table_over_enum"] = statistics.median(ms["table_v9_7_terms"]) / statistics.median(ms["enum"])
    assert isinstance(cfg2_specs(["custom_form"])["custom_form"].reward, RewardTerms)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
