"""Training probe for the loss kinds of hipets_train_steps_loss; writes profiles/train_kinds.json.

(a) The unchanged path: microseconds per minibatch step of hipets_train_steps (the old entry point) at the pets_halfcheetah shape
    (E 7, B 32, in 24, out 18, 5 linear layers of 200), for a library built at the parent commit and for this tree's, each in a
    fresh process through plain ctypes (the parent's library lacks the new symbols, so the package's loader would refuse it), in the
    order parent, this, parent.  The NLL instantiation is meant to be the same code: this tree's figure must lie within the parent's
    own two-run spread, or within 1 % of the parent's mean where that spread is smaller.

        python profiles/train_kinds_probe.py --parent-lib <libhipets.so built at the parent commit>

(b) The new kinds at the same widths: a BasicEnsemble of 5 members (NLL, per-member bounds, grad_scale 1 / 5) and a deterministic
    E 7 model (MSE), microseconds per step and milliseconds per epoch at N = 100 k, against the float32 restatement
    (tests/train_loss_restatement.py) run eager on the same GPU with the reference's host synchronisations (loss.item() and one
    .item() per parameter tensor for grad_norm, model.py:153-167); for the BasicEnsemble that restatement loops over the members,
    as BasicEnsemble.loss does.  Without --parent-lib only (b) runs."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mbrl-lib_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hipets  # noqa: E402
import train_loss_restatement as tlr  # noqa: E402
import train_restatement as tr  # noqa: E402
from hipets import _lib  # noqa: E402
from hipets._pack import pack_train_desc  # noqa: E402

B, IN, HID, OUT, L = 32, 24, 200, 18, 5
N = 100_000
DEV = "cuda:0"


def _inputs(kind, E, steps):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, IN, generator=g).to(DEV)
    y = (torch.randn(N, OUT, generator=g) * 0.3).to(DEV)
    ws, bs = tlr.random_model_kind(kind, E, IN, HID, OUT, L, 0, dtype=torch.float32)
    w, b = [t.to(DEV) for t in ws], [t.to(DEV) for t in bs]
    m = ([torch.zeros_like(t) for t in w], [torch.zeros_like(t) for t in b])
    v = ([torch.zeros_like(t) for t in w], [torch.zeros_like(t) for t in b])
    idx = torch.randint(0, N, (steps, E, B), generator=g, dtype=torch.int32).to(DEV)
    rows = torch.full((steps,), B, dtype=torch.int32, device=DEV)
    return x, y, w, b, m, v, idx, rows


def old_entry_child(lib_path, steps, reps):
    """One process, one library: the median over `reps` timed runs of `steps` steps through hipets_train_steps, after a warm-up."""
    lib = C.CDLL(lib_path)
    for name in ("hipets_create", "hipets_destroy", "hipets_train_steps", "hipets_last_error"):
        res, params = _lib.SYMBOLS[name]
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, [t for _, t in params]
    E = 7
    x, y, w, b, m, v, idx, rows = _inputs("nll", E, steps)
    lo, hi = -10 * torch.ones(OUT, device=DEV), 0.5 * torch.ones(OUT, device=DEV)
    loss, gsq = torch.empty(steps, E, device=DEV), torch.empty(steps, E, device=DEV)
    d, keep = pack_train_desc(torch.device(DEV), w, b, "silu", 0.01, OUT, B, adam=(m[0], m[1], v[0], v[1], lo, hi, 1e-3, 0.9, 0.999, 1e-8, 1e-5, 0))
    h = C.c_void_p()
    assert lib.hipets_create(0, C.byref(h)) == 0, lib.hipets_last_error()

    def run(n, step0):
        rc = lib.hipets_train_steps(h, C.byref(d), x.data_ptr(), y.data_ptr(), N, idx.data_ptr(), rows.data_ptr(), n, step0, loss.data_ptr(),
                                    gsq.data_ptr(), None)
        assert rc == 0, lib.hipets_last_error()
        torch.cuda.synchronize()

    run(8, 0)
    times = []
    for r in range(reps):
        t0 = time.perf_counter()
        run(steps, 8 + r * steps)
        times.append((time.perf_counter() - t0) / steps * 1e6)
    lib.hipets_destroy(h)
    del keep
    assert torch.isfinite(loss).all()
    print(json.dumps({"us_per_step": sorted(times)[len(times) // 2], "runs": [round(t, 2) for t in times], "loss_last": loss[-1].tolist()}))


def unchanged_path(parent_lib, steps, reps):
    runs = []
    for label, lib in (("parent", parent_lib), ("this", hipets.LIB_PATH), ("parent", parent_lib)):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--old-entry-child", lib, "--steps", str(steps), "--reps", str(reps)],
                             check=True, capture_output=True, text=True, timeout=600).stdout
        runs.append(dict(json.loads(out.strip().splitlines()[-1]), library=label))
    parent = [r["us_per_step"] for r in runs if r["library"] == "parent"]
    this = [r["us_per_step"] for r in runs if r["library"] == "this"][0]
    mean = sum(parent) / 2
    spread = abs(parent[0] - parent[1])
    if spread >= 0.01 * mean:
        allowed, within = spread, min(parent) <= this <= max(parent)
    else:
        allowed, within = 0.01 * mean, abs(this - mean) <= 0.01 * mean
    same_bits = all(r["loss_last"] == runs[0]["loss_last"] for r in runs)
    return {"shape": dict(E=7, B=B, **{"in": IN}, hid=HID, out=OUT, linear_layers=L), "steps_timed": steps, "repetitions": reps, "runs": runs,
            "parent_us_per_step": [round(p, 2) for p in parent], "this_us_per_step": round(this, 2), "parent_spread_us": round(spread, 2),
            "allowed_us": round(allowed, 2), "this_minus_parent_mean_us": round(this - mean, 2),
            "within_parent_spread_or_1_percent": bool(within), "losses_bit_identical": same_bits}


def new_kind(name, kind, E, basic, steps, eager_steps):
    eng = hipets.get_engine(DEV)
    x, y, w, b, m, v, idx, rows = _inputs(kind, E, steps)
    lo = hi = None
    kw = dict(loss=kind)
    if kind == "nll":
        lo, hi = (t.float().to(DEV).contiguous() for t in tlr.member_bounds(E, OUT))
        kw.update(bounds_per_member=True)
    scale = float(torch.tensor(1.0) / E) if basic else 1.0
    kw.update(grad_scale=scale)
    eng.train_steps(w, b, m, v, lo, hi, x, y, idx[:8], rows[:8], 0, lr=1e-3, weight_decay=1e-5, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.train_steps(w, b, m, v, lo, hi, x, y, idx, rows, 8, lr=1e-3, weight_decay=1e-5, **kw)
    torch.cuda.synchronize()
    us_step = (time.perf_counter() - t0) / steps * 1e6
    # baseline: the float32 restatement eager on the GPU with the reference's synchronisations; a BasicEnsemble member by member
    groups = [slice(e, e + 1) for e in range(E)] if basic else [slice(0, E)]
    we, be = [[t[s].clone() for t in w] for s in groups], [[t[s].clone() for t in b] for s in groups]
    me = [([torch.zeros_like(t) for t in ws_], [torch.zeros_like(t) for t in bs_]) for ws_, bs_ in zip(we, be)]
    ve = [([torch.zeros_like(t) for t in ws_], [torch.zeros_like(t) for t in bs_]) for ws_, bs_ in zip(we, be)]

    def eager(s):
        sel = idx[s].long()
        total, grads = 0.0, []
        for gi, sl in enumerate(groups):
            if kind == "mse":
                loss, dws, dbs = tlr.mse_step(we[gi], be[gi], x[sel[sl]], y[sel[sl]], "silu", grad_scale=scale)
            else:
                loss, dws, dbs = tlr.nll_step_kind(we[gi], be[gi], x[sel[sl]], y[sel[sl]], lo[sl].unsqueeze(1), hi[sl].unsqueeze(1), "silu",
                                                   grad_scale=scale)
            total = total + loss.sum()
            grads.append((dws, dbs))
        _ = (total * scale).item()
        _ = sum(gg.norm().item() ** 2 for dws, dbs in grads for gg in dws + dbs)
        for gi, (dws, dbs) in enumerate(grads):
            for li in range(L):
                tr.adam_(we[gi][li], dws[li], me[gi][0][li], ve[gi][0][li], s + 1, 1e-3, weight_decay=1e-5)
                tr.adam_(be[gi][li], dbs[li], me[gi][1][li], ve[gi][1][li], s + 1, 1e-3, weight_decay=1e-5)

    for s in range(5):
        eager(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(eager_steps):
        eager(s)
    torch.cuda.synchronize()
    eager_us = (time.perf_counter() - t0) / eager_steps * 1e6
    per_epoch = (N - 1) // B + 1
    return {"model": name, "loss": kind, "shape": dict(E=E, B=B, **{"in": IN}, hid=HID, out=OUT, linear_layers=L), "N": N, "steps_timed": steps,
            "hip_us_per_step": round(us_step, 2), "hip_ms_per_epoch": round(us_step * per_epoch / 1e3, 1), "eager_us_per_step": round(eager_us, 1),
            "eager_ms_per_epoch": round(eager_us * per_epoch / 1e3, 1), "speedup": round(eager_us / us_step, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_kinds.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eager-steps", type=int, default=60)
    ap.add_argument("--old-entry-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.old_entry_child:
        return old_entry_child(a.old_entry_child, a.steps, a.reps)
    res = {}
    if a.parent_lib:
        res["unchanged_path"] = unchanged_path(os.path.abspath(a.parent_lib), a.steps, a.reps)
    res["new_kinds"] = [new_kind("BasicEnsemble of 5 GaussianMLP members", "nll", 5, True, min(a.steps, 400), a.eager_steps),
                        new_kind("GaussianMLP(deterministic=True), 7 members", "mse", 7, False, min(a.steps, 400), a.eager_steps)]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
