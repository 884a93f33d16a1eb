"""Records tests/golden/sac_update_cases.npz from the reference's own SAC.update_parameters
(mbrl/third_party/pytorch_sac_pranz24/sac.py:76-173) on the CPU, for the small cases of tests/sac_restatement.py (RECORDED): the
parameters, the target network, log_alpha, the Adam moments and the 5-tuple after one update, and the two normal tables the update
drew (the global generator is reseeded and the draws of Normal.rsample are replayed, next state first).  Needs mbrl on the path:

    PYTHONPATH=<mbrl-lib checkout> python tests/make_sac_update_golden.py            # record
    python tests/make_sac_update_golden.py --search                                  # print, per case, the first seed check_kinks accepts

Per case it also records the calibration number of the GPU tests' rule: the largest distance between the float32 and the float64
restatement over all parameters after the update.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sac_restatement as sr  # noqa: E402

OUT = os.path.join(HERE, "golden", "sac_update_cases.npz")
SEED = 1234


def search():
    for name, spec in sr.CASES.items():
        for seed in range(2000):
            sr.CASES[name] = dict(spec, seed=seed)
            sr._BUILT.pop(name, None)
            try:
                sr.build_case(name)
            except AssertionError:
                continue
            print(f"{name}: seed={seed}", flush=True)
            break
        else:
            print(f"{name}: no seed below 2000", flush=True)


def record():
    from mbrl.third_party.pytorch_sac_pranz24.sac import SAC

    out = {}
    for name in sr.RECORDED:
        case = sr.build_case(name)
        obs, act, hid, B = case["shape"]
        p, batches, scale, bias = case["inputs"]
        args = SimpleNamespace(gamma=sr.HP["gamma"], tau=sr.HP["tau"], alpha=sr.HP["alpha"], policy="Gaussian", target_update_interval=case["interval"],
                               automatic_entropy_tuning=case["tuning"], device="cpu", hidden_size=hid, lr=sr.HP["lr"], target_entropy=None)
        space = SimpleNamespace(shape=(act,), high=np.ones(act, dtype=np.float32), low=-np.ones(act, dtype=np.float32))
        sac = SAC(obs, space, args)
        shim = sr.TinySAC.__new__(sr.TinySAC)  # (load / params walk the same attribute names on the reference's agent)
        shim.__dict__ = sac.__dict__
        shim.load(p, scale, bias)
        torch.manual_seed(SEED)
        res = sac.update_parameters(sr.FixedMemory(batches), B, case["first_update"], None, reverse_mask=True)
        torch.manual_seed(SEED)
        out[f"{name}/eps_next"] = torch.empty(B, act).normal_().numpy()
        out[f"{name}/eps_cur"] = torch.empty(B, act).normal_().numpy()
        out[f"{name}/result"] = np.asarray(res, dtype=np.float64)
        for n, t in shim.params().items():
            out[f"{name}/p/{n}"] = t.detach().numpy().copy()
            if n[0] != "t":
                st = shim.optimizer_of(n).state[t]
                out[f"{name}/m/{n}"] = st["exp_avg"].numpy().copy()
                out[f"{name}/v/{n}"] = st["exp_avg_sq"].numpy().copy()
                assert float(st["step"]) == 1.0
        out[f"{name}/calibration"] = np.asarray(max(tr_dist(case["f32"]["p"][n], case["f64"]["p"][n]) for n in case["f64"]["p"]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


def tr_dist(a, b):
    return (a.double() - b.double()).abs().max().item()


if __name__ == "__main__":
    search() if "--search" in sys.argv else record()
