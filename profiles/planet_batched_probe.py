"""Batched PlaNet planning (hipets.BatchedCEMAgent over a PlaNetTrajectoryEvalFn: n_env latent start states per launch) at the PlaNet
conf shape: conf/overrides/planet_cheetah_run.yaml:29-35 (clipped-normal CEM, pop 1000 per environment, H 12, 10 iterations, alpha 0)
on conf/dynamics_model/planet.yaml sizes (latent 30, belief 200, hidden 200, action 6), one particle.  A single plan's rollout is
63 one-tile workgroups on 256 CUs; n_env environments give 63 n_env (n_env * 1000 rows, 16 rows per workgroup).

Per n_env in {1, 2, 4, 8}: ms per batched plan and per environment-plan, and the average hipets_planet_rollout call of one CEM
iteration's population (n_env * 1000 candidates: the rollout kernel plus the particle-mean launch, torch events around a burst of
calls on the launch stream, as bench.py's planet block).  ``--rollout-only N`` runs just the rollout burst for n_env = N (for a
``rocprofv3 --kernel-trace --stats`` run of its own).  Usage: python profiles/planet_batched_probe.py [--out FILE] [--rollout-only N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mbrl-lib_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import hipets  # noqa: E402

ITERS, POP, H, A, L, HB = 10, 1000, 12, 6, 30, 200


def rollout_ms(eng, n_env, reps=20):
    g = torch.Generator().manual_seed(n_env)
    acts = (torch.rand(n_env * POP, H, A, generator=g) * 2 - 1).to(eng.device)
    l0, b0 = (torch.randn(n_env, L, generator=g) * 0.3).to(eng.device), (torch.randn(n_env, HB, generator=g) * 0.3).to(eng.device)
    for _ in range(5):
        eng.planet_rollout(acts, l0, b0, 1, seed=1, n_env=n_env)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        out = eng.planet_rollout(acts, l0, b0, 1, seed=1, n_env=n_env)
    ev1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return ev0.elapsed_time(ev1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rollout-only", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = hipets.get_engine(dev)
    spec = bench.synthetic_planet_spec(dev)
    fn = hipets.make_eval_fn(spec, 1, engine=eng, seed=0)
    if args.rollout_only:
        eng.planet_set_model(spec)
        print(json.dumps({"n_env": args.rollout_only, "rollout_call_ms": rollout_ms(eng, args.rollout_only, reps=50)}))
        return
    res = {}
    for n_env in (1, 2, 4, 8):
        agent = hipets.BatchedCEMAgent(fn, n_env, [-1.0] * A, [1.0] * A, H, ITERS, 0.1, POP, 0.0, return_mean_elites=True, clipped_normal=True,
                                       seed=0)
        g = torch.Generator().manual_seed(0)
        lat, bel = (torch.randn(n_env, L, generator=g) * 0.3).to(dev), (torch.randn(n_env, HB, generator=g) * 0.3).to(dev)
        obs = np.zeros((n_env, 3, 64, 64), np.float32)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:
            agent.plan(obs, latent=lat, belief=bel)
        torch.cuda.synchronize()
        n = 20
        t0 = time.perf_counter()
        for _ in range(n):
            plans = agent.plan(obs, latent=lat, belief=bel)
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / n
        assert np.isfinite(plans).all()
        r_ms = rollout_ms(eng, n_env)
        res[f"n_env={n_env}"] = {"ms_per_batched_plan": 1e3 * el, "ms_per_environment_plan": 1e3 * el / n_env,
                                 "rollout_call_ms": r_ms, "rollout_call_ms_per_environment": r_ms / n_env,
                                 "rollout_workgroups": (n_env * POP + 15) // 16, "plans_timed": n,
                                 "candidate_steps_per_s": ITERS * POP * H * n_env / el}
    out = {"workload": "BatchedCEMAgent over PlaNetTrajectoryEvalFn: clipped-normal CEM, pop 1000 per environment, H 12, 10 iterations, "
                       "alpha 0, one particle; latent 30, belief 200, hidden 200, action 6 (STATIC kernel instance)",
           "rollout_call": "average hipets_planet_rollout call over n_env * 1000 candidates (planet_rollout_kernel + particle-mean launch), "
                           "20 back-to-back calls between two events on the launch stream",
           "device": torch.cuda.get_device_name(dev), "results": res}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
