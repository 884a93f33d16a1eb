"""precision='bf16' against 'bf16x3' and 'f32' on cfg2 at full size, both modes: the three arithmetic modes interleaved in ONE process
(round-robin, so clock and thermal drift hit all three alike), the library's hipEvent timing (profiles/precision_probe.py measure):
    python profiles/bf16_probe.py --repeats 5 --reps 10 --out profiles/bf16_rollout.json
Per (mode, precision): ms per rollout (minimum, median, spread over the repeats), candidate-steps/s, and for bf16 the TFLOP/s issued
against the 2.5 PFLOP/s dense bf16 peak.  The one gate: bf16 is faster per rollout than both other modes, in both modes."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import precision_probe as pp  # noqa: E402
from precision_probe import bench, hipets, torch  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    actions = pp.cfg2_actions(dev)
    specs = {p: bench.synthetic_spec(dev, precision=p) for p in pp.PRECISIONS}
    cand_steps = bench.POP * bench.PARTICLES * bench.HORIZON
    flops = specs["bf16"].flops_per_candidate_step() * cand_steps
    res = {"workload": f"cfg2: pop {bench.POP} x {bench.PARTICLES} particles, H {bench.HORIZON}, hid {bench.HID}",
           "lib": os.environ.get("HIPETS_LIB", "default"), "repeats": a.repeats, "rollouts_per_repeat": a.reps, "modes": {}}
    ok = True
    for mode in ("device", "fast"):
        ms = {p: [] for p in pp.PRECISIONS}
        cls = {}
        for r in range(a.repeats):
            for p in pp.PRECISIONS:
                ms[p].append(pp.measure(eng, specs[p], actions, mode, a.reps, warmup=2, stream0=100 * r + 10)[1])
                cls[p] = list(eng.kernel_class(bench.POP, bench.PARTICLES, bench.HORIZON, mode=mode))
        blk = {}
        for p in pp.PRECISIONS:
            lo, med, hi = min(ms[p]), statistics.median(ms[p]), max(ms[p])
            blk[p] = {"kernel_class": cls[p], "ms_per_rollout": {"min": lo, "median": med, "max": hi, "spread_rel": (hi - lo) / med},
                      "candidate_steps_per_s": cand_steps / (med * 1e-3)}
        tf = flops / (blk["bf16"]["ms_per_rollout"]["median"] * 1e-3) / 1e12
        blk["bf16"]["tflops_issued"] = tf
        blk["bf16"]["fraction_of_bf16_peak"] = tf / PEAK_BF16_TFLOPS
        blk["speedup_bf16_over"] = {p: blk[p]["ms_per_rollout"]["median"] / blk["bf16"]["ms_per_rollout"]["median"] for p in ("f32", "bf16x3")}
        blk["gate_bf16_fastest"] = all(blk["bf16"]["ms_per_rollout"]["median"] < blk[p]["ms_per_rollout"]["median"] and
                                       blk["bf16"]["ms_per_rollout"]["min"] < blk[p]["ms_per_rollout"]["min"] for p in ("f32", "bf16x3"))
        ok = ok and blk["gate_bf16_fastest"]
        res["modes"][mode] = blk
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
