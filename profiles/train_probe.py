"""Model-training probe (hipets.ModelTrainer's kernels): microseconds per minibatch step and milliseconds per
epoch over N = 100 k transitions at the pets_halfcheetah and mbpo_halfcheetah shapes, the evaluate pass over the same N, and
the same for our float32 restatement (tests/train_restatement.py) run eager on the same GPU with the reference's per-step host
synchronisations (loss.item() + one .item() per parameter tensor for grad_norm, model.py:153-167) as the baseline.

    python profiles/train_probe.py [--out profiles/train_epoch.json] [--steps 400]

Run under `rocprofv3 --kernel-trace --stats -- python profiles/train_probe.py` for the per-kernel summary."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mbrl-lib_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hipets  # noqa: E402
import train_restatement as tr  # noqa: E402

SHAPES = {  # E, B, in, hid, out, linear layers (conf/dynamics_model/gaussian_mlp_ensemble.yaml: 4 hidden layers of 200)
    "pets_halfcheetah": (7, 32, 24, 200, 18, 5),
    "mbpo_halfcheetah": (7, 256, 23, 200, 18, 5),
}
N = 100_000
DEV = "cuda:0"


def measure(name, steps, eager_steps):
    E, B, in_dim, hid, out, L = SHAPES[name]
    eng = hipets.get_engine(DEV)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, in_dim, generator=g).to(DEV)
    y = (torch.randn(N, out, generator=g) * 0.3).to(DEV)
    ws, bs = tr.random_model(E, in_dim, hid, out, L, 0, dtype=torch.float32)
    w = [t.to(DEV) for t in ws]
    b = [t.to(DEV) for t in bs]
    m = ([torch.zeros_like(t) for t in w], [torch.zeros_like(t) for t in b])
    v = ([torch.zeros_like(t) for t in w], [torch.zeros_like(t) for t in b])
    lo, hi = -10 * torch.ones(out, device=DEV), 0.5 * torch.ones(out, device=DEV)
    idx = torch.randint(0, N, (steps, E, B), generator=g, dtype=torch.int32).to(DEV)
    rows = torch.full((steps,), B, dtype=torch.int32, device=DEV)
    # warm-up, then the timed run
    eng.train_steps(w, b, m, v, lo, hi, x, y, idx[:8], rows[:8], 0, lr=1e-3, weight_decay=1e-5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.train_steps(w, b, m, v, lo, hi, x, y, idx, rows, 8, lr=1e-3, weight_decay=1e-5)
    torch.cuda.synchronize()
    us_step = (time.perf_counter() - t0) / steps * 1e6
    steps_per_epoch = (N - 1) // B + 1
    eng.train_eval(w, b, x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        eng.train_eval(w, b, x, y)
    torch.cuda.synchronize()
    eval_ms = (time.perf_counter() - t0) / 5 * 1e3
    # baseline: the float32 restatement eager on the GPU, with the reference's host synchronisations per step
    we = [t.clone() for t in w]
    be = [t.clone() for t in b]
    me = ([torch.zeros_like(t) for t in we], [torch.zeros_like(t) for t in be])
    ve = ([torch.zeros_like(t) for t in we], [torch.zeros_like(t) for t in be])
    lo2, hi2 = lo.reshape(1, -1), hi.reshape(1, -1)

    def eager(s):
        sel = idx[s].long()
        loss, dws, dbs = tr.nll_step(we, be, x[sel], y[sel], lo2, hi2, "silu")
        _ = loss.sum().item()
        _ = sum(gg.norm().item() ** 2 for gg in dws + dbs)
        for li in range(L):
            tr.adam_(we[li], dws[li], me[0][li], ve[0][li], s + 1, 1e-3, weight_decay=1e-5)
            tr.adam_(be[li], dbs[li], me[1][li], ve[1][li], s + 1, 1e-3, weight_decay=1e-5)

    for s in range(5):
        eager(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(eager_steps):
        eager(s)
    torch.cuda.synchronize()
    eager_us = (time.perf_counter() - t0) / eager_steps * 1e6
    return {"shape": dict(zip(("E", "B", "in", "hid", "out", "linear_layers"), SHAPES[name])), "N": N, "steps_timed": steps,
            "hip_us_per_step": round(us_step, 2), "hip_ms_per_epoch": round(us_step * steps_per_epoch / 1e3, 1),
            "hip_eval_ms": round(eval_ms, 3), "eager_us_per_step": round(eager_us, 1),
            "eager_ms_per_epoch": round(eager_us * steps_per_epoch / 1e3, 1), "speedup": round(eager_us / us_step, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_epoch.json"))
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--eager-steps", type=int, default=60)
    a = ap.parse_args()
    res = {name: measure(name, a.steps, a.eager_steps) for name in SHAPES}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
