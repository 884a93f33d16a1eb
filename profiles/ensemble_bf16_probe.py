"""The bf16 form of hipets_ensemble_predict (kernel="bf16", csrc/ensemble_bf16.hip) against the tile form, the wide form and torch's
float32 forward plus the same four statistics on one MI355X:
    python profiles/ensemble_bf16_probe.py --out profiles/ensemble_bf16.json
Four routes take turns in one process, sample by sample (value_objective_probe.measure: warm-up rounds, then samples of the
device-event time of `reps` back-to-back calls / reps; median, min, p90 in ms per call), at 23-200x4-36 and 393-200x4-754, 7 members,
100 000 and 256 rows -- once for the statistics alone and once for all outputs.  Per shape also the largest |bf16 - tile| of each
statistic relative to the statistic.  Then one penalised hipets.rollout_model_and_populate_sac_buffer call at mbpo_halfcheetah's shape at
rollout lengths 1 and 5 under every ensemble_kernel: a host clock around calls that end in a device -> host copy.
`bf16_wins` of a row: the bf16 median is below the median of the best fp32 route (tile, wide or torch) and bf16's p90 is below that
route's min."""
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

import bench  # noqa: E402
import hipets  # noqa: E402
import mbpo_populate_probe as mp  # noqa: E402
from ensemble_predict_probe import torch_forward  # noqa: E402
from hipets.ensemble import reference_statistics  # noqa: E402
from value_objective_probe import measure  # noqa: E402

KERNELS = ("tile", "wide", "bf16")


def verdict(ms):
    best = min((ms["tile"], ms["wide"], ms["torch_forward_and_stats"]), key=lambda s: s["median"])
    return bool(ms["bf16"]["median"] < best["median"] and ms["bf16"]["p90"] < best["min"])


def piece(engine, spec, rows, a, name):
    dev = engine.device
    g = torch.Generator().manual_seed(1)
    obs = (0.5 * torch.randn(rows, spec.obs_dim, generator=g)).to(dev)
    act = (torch.rand(rows, spec.act_dim, generator=g) * 2 - 1).to(dev)
    x = torch.cat([obs, act], dim=1)  # (the synthetic normaliser is mean 0 / std 1 and there is no obs_process: the model input itself)
    hipets.EnsemblePredictor(spec, engine=engine)
    res = {"rows": rows, "members": spec.ensemble_size, "layers": [int(w.shape[1]) for w in spec.weights] + [int(spec.weights[-1].shape[2])],
           "geometry": {k: engine.ensemble_geometry(rows, kernel=k) for k in KERNELS}}
    got = {k: engine.ensemble_predict(obs, act, mean=False, logvar=False, stats=True, kernel=k)[2] for k in KERNELS}
    rel = ((got["bf16"] - got["tile"]).abs() / got["tile"].abs().clamp_min(1e-30)).max(dim=0).values
    res["max_rel_stat_diff_bf16_vs_tile"] = dict(zip(("max_std", "disagreement", "total_std", "max_deviation"), (float(v) for v in rel)))

    def torch_route():
        with torch.no_grad():
            return reference_statistics(*torch_forward(spec, x))

    for what, kw in (("stats_only", dict(mean=False, logvar=False, stats=True)), ("all_outputs", dict(stats=True))):
        routes = {k: (lambda k=k: engine.ensemble_predict(obs, act, kernel=k, **kw)) for k in KERNELS}
        routes["torch_forward_and_stats"] = torch_route
        ms = measure(routes, a)
        res[what] = {"ms": ms, "bf16_wins": verdict(ms), "bf16_over_tile": ms["bf16"]["median"] / ms["tile"]["median"],
                     "bf16_over_wide": ms["bf16"]["median"] / ms["wide"]["median"],
                     "bf16_over_torch": ms["bf16"]["median"] / ms["torch_forward_and_stats"]["median"]}
    print(f"[{name}] {json.dumps(res)}", flush=True)
    return res


def populate_piece(engine, spec, rows, length, reps):
    dev = engine.device
    env = hipets.ModelEnv(spec, engine=engine, seed=1)
    rng = np.random.default_rng(0)
    source = mp.Buffer(rows, mp.OBS, mp.ACT, rng)
    first = (rng.standard_normal((rows, mp.OBS)) * 0.1).astype(np.float32)
    source.add_batch(first, np.zeros((rows, mp.ACT), np.float32), first, np.zeros(rows, np.float32), np.zeros(rows, bool), np.zeros(rows, bool))
    agent = mp.TorchAgent(mp.TorchGaussianPolicy(mp.OBS, mp.ACT, mp.HID).to(dev), dev)
    sac = mp.Buffer(2 * length * rows, mp.OBS, mp.ACT, rng)
    penalty = hipets.UncertaintyPenalty("max_std", coef=1.0)
    out = {k: mp.wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sac, True, length, rows, uncertainty=penalty, ensemble_kernel=k), reps)
           for k in KERNELS}
    return {"shape": dict(rows=rows, obs=mp.OBS, act=mp.ACT, rollout_length=length, penalty="max_std"), "ms": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("ensemble_bf16_probe.py needs a GPU: nothing measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    engine = hipets.get_engine(dev)
    half = bench.synthetic_spec(dev, ensemble=7, elite=[0, 1, 2, 3, 4], learned_rewards=True)  # 23-200x4-36
    humanoid = bench.synthetic_spec(dev, obs=376, act=17, ensemble=7, elite=[0, 1, 2, 3, 4], learned_rewards=True)  # 393-200x4-754
    res = {"device": torch.cuda.get_device_name(0),
           "method": f"{a.warmup} warm-up rounds, then {a.samples} samples of the device-event time of {a.reps} back-to-back calls / {a.reps}, "
                     "the four routes interleaved; median, min, p90 in ms per call; bf16_wins: bf16 median < the median of the best fp32 route "
                     "(tile, wide or torch) and bf16 p90 < that route's min"}
    res["mbpo_halfcheetah"] = piece(engine, half, 100_000, a, "23-200x4-36, 100 000 rows")
    res["mbpo_halfcheetah_256_rows"] = piece(engine, half, 256, a, "23-200x4-36, 256 rows")
    res["humanoid"] = piece(engine, humanoid, 100_000, a, "393-200x4-754, 100 000 rows")
    res["humanoid_256_rows"] = piece(engine, humanoid, 256, a, "393-200x4-754, 256 rows")
    res["populate_length_1"] = populate_piece(engine, half, 100_000, 1, 10)
    res["populate_length_5"] = populate_piece(engine, half, 100_000, 5, 5)
    print(json.dumps({k: res[k] for k in ("populate_length_1", "populate_length_5")}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print("\n| shape | outputs | tile (median, min..p90) | wide | bf16 | torch forward + stats | bf16 wins |\n|---|---|---|---|---|---|---|")
    cell = lambda s: f"{s['median']:.3f} ({s['min']:.3f}..{s['p90']:.3f})"  # noqa: E731
    for k in ("mbpo_halfcheetah", "mbpo_halfcheetah_256_rows", "humanoid", "humanoid_256_rows"):
        for what in ("stats_only", "all_outputs"):
            r = res[k][what]
            print(f"| {k} | {what} | {cell(r['ms']['tile'])} | {cell(r['ms']['wide'])} | {cell(r['ms']['bf16'])} | {cell(r['ms']['torch_forward_and_stats'])} | {r['bf16_wins']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
