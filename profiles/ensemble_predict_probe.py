"""Ensemble predictions and uncertainty at MBPO's shapes: what hipets_ensemble_predict costs against the route a user had before it --
torch's own ``GaussianMLP.forward(x, use_propagation=False)`` (EnsembleLinearLayer matmuls, SiLU, the two softplus clamps) plus the same
four statistics in torch, on the same GPU -- and what a penalised populate call costs against the reference's loop with that torch
ensemble computing the penalty.

    python profiles/ensemble_predict_probe.py [--out profiles/ensemble_predict.json] [--reps 20]

One process, its steps one after the other; run it under a time limit.  Launch times: device events around one call, 3 warm-up calls,
the median of --reps (min and p90 next to it).  Populate calls: a host clock around calls that end in a device -> host copy.  The share
of the fp32 MFMA peak is the algorithm's products (2 x rows x members x sum of in x out over the layers) over the median launch time
over 157.3 TFLOP/s.  No profiler runs here.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mbrl-lib_amd"), os.path.join(ROOT, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
import hipets  # noqa: E402
import mbpo_populate_probe as mp  # noqa: E402  (the torch policy, the host buffers and the timers of the populate probe)
from hipets import mbpo  # noqa: E402
from hipets.ensemble import ReferencePenalisedEnv, reference_statistics  # noqa: E402

FP32_MFMA_PEAK = 157.3e12


def torch_forward(spec, x, members=None):
    """gaussian_mlp.py:140-154 over the spec's tensors on their device"""
    pick = (lambda t: t) if members is None else (lambda t: t[members])
    h = x
    for l, (w, b) in enumerate(zip(spec.weights, spec.biases)):
        h = h.matmul(pick(w)) + pick(b)
        if l < len(spec.weights) - 1:
            h = F.silu(h)
    out = spec.out_dim
    lo, hi = spec.min_logvar.to(x.device), spec.max_logvar.to(x.device)
    lv = hi - F.softplus(hi - h[..., out:])
    return h[..., :out], lo + F.softplus(lv - lo)


def measure_shape(engine, spec, rows, reps, name):
    dev = engine.device
    g = torch.Generator().manual_seed(1)
    obs = (0.5 * torch.randn(rows, spec.obs_dim, generator=g)).to(dev)
    act = (torch.rand(rows, spec.act_dim, generator=g) * 2 - 1).to(dev)
    predictor = hipets.EnsemblePredictor(spec, engine=engine)
    x = torch.cat([obs, act], dim=1)  # (the synthetic normaliser is mean 0 / std 1 and there is no obs_process: the model input itself)
    res = {"rows": rows, "members": spec.ensemble_size, "layers": [int(w.shape[1]) for w in spec.weights] + [int(spec.weights[-1].shape[2])]}
    res["row_tiles"], res["lds_bytes"] = predictor.geometry(rows)
    res["hip_stats_only"] = mp.events(lambda: predictor.uncertainty(obs, act, only_elite=False), reps)
    res["hip_all_outputs"] = mp.events(lambda: engine.ensemble_predict(obs, act, stats=True), reps)
    res["hip_stats_only_elites"] = mp.events(lambda: predictor.uncertainty(obs, act, only_elite=True), reps)
    with torch.no_grad():
        res["torch_forward_and_stats"] = mp.events(lambda: reference_statistics(*torch_forward(spec, x)), reps)
        res["torch_forward"] = mp.events(lambda: torch_forward(spec, x), reps)
        # the two routes agree (float32 against float32: a loose sanity bound, the tests hold the real one)
        want = reference_statistics(*torch_forward(spec, x))
    got = predictor.uncertainty(obs, act, only_elite=False)
    res["max_abs_stat_difference_to_torch"] = float((got - want).abs().max())
    assert res["max_abs_stat_difference_to_torch"] < 1e-3, res
    flops = 2.0 * rows * spec.ensemble_size * sum(int(w.shape[1]) * int(w.shape[2]) for w in spec.weights)
    for k in ("hip_stats_only", "hip_all_outputs", "torch_forward_and_stats"):
        res[k]["tflops"] = flops / (res[k]["median_ms"] * 1e-3) / 1e12
        res[k]["share_of_fp32_mfma_peak"] = res[k]["tflops"] * 1e12 / FP32_MFMA_PEAK
    res["speedup_stats_only_vs_torch"] = res["torch_forward_and_stats"]["median_ms"] / res["hip_stats_only"]["median_ms"]
    res["speedup_all_outputs_vs_torch"] = res["torch_forward_and_stats"]["median_ms"] / res["hip_all_outputs"]["median_ms"]
    print(f"[{name}] {json.dumps(res)}", flush=True)
    return res


class TorchPenalisedEnv(ReferencePenalisedEnv):
    """the reference loop's penalised step over a hipets.ModelEnv with the TORCH ensemble computing the statistics (what a user could
    write before the kernel): numpy in, numpy out"""

    def __init__(self, env, penalty, spec):
        super().__init__(env, penalty)
        self.spec = spec

    @torch.no_grad()
    def step(self, actions, model_state, sample=False):
        p = self.penalty
        obs = model_state["obs"]
        act = torch.as_tensor(np.asarray(actions), dtype=torch.float32, device=obs.device)
        members = self.spec.members if p.only_elite else None
        u = reference_statistics(*torch_forward(self.spec, torch.cat([obs, act], dim=1), members))[:, p.stat].cpu().numpy()
        nobs, rew, done, state = self.env.step(actions, model_state, sample=sample)
        rew = np.asarray(rew, dtype=np.float32).copy()
        rew[:, 0] = rew[:, 0] - np.float32(p.coef) * u
        return nobs, rew, done, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_predict.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=100_000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU: no GPU, no numbers"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    engine = hipets.get_engine(dev)
    N = args.rows
    half = bench.synthetic_spec(dev, ensemble=7, elite=[0, 1, 2, 3, 4], learned_rewards=True)  # 23-200x4-36
    humanoid = bench.synthetic_spec(dev, obs=376, act=17, ensemble=7, elite=[0, 1, 2, 3, 4], learned_rewards=True)  # 393-200x4-754
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "fp32_mfma_peak_tflops": FP32_MFMA_PEAK / 1e12}
    res["mbpo_halfcheetah"] = measure_shape(engine, half, N, args.reps, "mbpo_halfcheetah")
    res["mbpo_halfcheetah_256_rows"] = measure_shape(engine, half, 256, args.reps, "256 rows")
    res["humanoid"] = measure_shape(engine, humanoid, N, args.reps, "humanoid")
    res["humanoid_256_rows"] = measure_shape(engine, humanoid, 256, args.reps, "humanoid 256 rows")
    # the model step over the same rows, for scale (the ensemble launch is E forwards of them)
    env = hipets.ModelEnv(half, engine=engine, seed=1)
    rng = np.random.default_rng(0)
    source = mp.Buffer(N, mp.OBS, mp.ACT, rng)
    first = (rng.standard_normal((N, mp.OBS)) * 0.1).astype(np.float32)
    source.add_batch(first, np.zeros((N, mp.ACT), np.float32), first, np.zeros(N, np.float32), np.zeros(N, bool), np.zeros(N, bool))
    state = env.reset(source.obs, return_as_np=False)
    action = (torch.rand(N, mp.ACT, device=dev) * 2 - 1)
    res["model_step_same_rows"] = mp.events(lambda: env.step(action, state, sample=True), args.reps)
    env._return_as_np = True
    # ---- one populate call, with and without a penalty, against the reference loop with the torch ensemble ----
    policy = mp.TorchGaussianPolicy(mp.OBS, mp.ACT, mp.HID).to(dev)
    agent = mp.TorchAgent(policy, dev)
    penalty = hipets.UncertaintyPenalty("max_std", coef=1.0)
    res["populate"] = {}
    for L in (1, 5):
        sac = mp.Buffer(2 * N * L, mp.OBS, mp.ACT, rng)
        plain = mp.wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sac, True, L, N), args.reps)
        pen = mp.wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sac, True, L, N, uncertainty=penalty), args.reps)
        ring = hipets.DeviceReplayBuffer(2 * N * L, (mp.OBS,), (mp.ACT,), engine=engine)
        pen_ring = mp.wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, agent, ring, True, L, N, uncertainty=penalty), args.reps)
        loop = mp.wall(lambda: mbpo.reference_populate_loop(TorchPenalisedEnv(env, penalty, half), source, agent, sac, True, L, N), max(5, args.reps // 2))
        res["populate"][f"L{L}"] = {"fused_no_penalty": plain, "fused_penalised": pen, "fused_penalised_device_ring": pen_ring,
                                    "reference_loop_torch_ensemble_penalty": loop, "penalty_cost_ms": pen["median_ms"] - plain["median_ms"],
                                    "speedup_median": loop["median_ms"] / pen["median_ms"]}
        print(f"[populate L={L}] {json.dumps(res['populate'][f'L{L}'])}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("\n| shape | rows | R | stats only ms | all outputs ms | torch forward + stats ms | share of fp32 MFMA peak (stats only) |\n|---|---|---|---|---|---|---|")
    for k in ("mbpo_halfcheetah", "mbpo_halfcheetah_256_rows", "humanoid", "humanoid_256_rows"):
        r = res[k]
        print(f"| {k} | {r['rows']} | {r['row_tiles']} | {r['hip_stats_only']['median_ms']:.3f} | {r['hip_all_outputs']['median_ms']:.3f} | "
              f"{r['torch_forward_and_stats']['median_ms']:.3f} | {r['hip_stats_only']['share_of_fp32_mfma_peak']:.3f} |")


if __name__ == "__main__":
    main()
