"""Records tests/golden/sac_update_cases.npz from the reference's own SAC.update_parameters
(mbrl/third_party/pytorch_sac_pranz24/sac.py:76-173) on the CPU, for the small cases of tests/sac_restatement.py (RECORDED): the
parameters, the target network, log_alpha, the Adam moments and the 5-tuple after one update, and the two normal tables the update
drew (the global generator is reseeded and the draws of Normal.rsample are replayed, next state first).  A case with its own Adam
settings or a starting optimizer state ("resumed") has them written into the reference's optimizers before the update.  A recording
that would change an array the file already holds is refused.  Needs mbrl on the path:

    PYTHONPATH=<mbrl-lib checkout> python tests/make_sac_update_golden.py            # record
    python tests/make_sac_update_golden.py --search [case ...]                       # print, per case, the first seed check_kinks accepts
    python tests/make_sac_update_golden.py --search-hand-over                        # (on the GPU) the hand-over test's generator seeds

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


def search(only=()):
    for name, spec in sr.CASES.items():
        if only and name not in only:
            continue
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


def search_hand_over(K=3, name="s17_6_17_17", device="cuda:0"):
    """Generator seeds for tests/test_gpu_sac_update.py's hand-over test (HAND_OVER_SEEDS): K updates drawn behind the first seed, one
    behind the second, one behind the third, all on the case's one batch, such that check_kinks holds for the K + 2 updates.  The
    draws are the device generator's: needs the GPU."""
    case = sr.build_case(name)
    act, B = case["shape"][1], case["shape"][3]
    p, batches, scale, bias = case["inputs"]

    def draws(seed, n):
        torch.manual_seed(seed)
        return [(torch.empty(B, act, device=device).normal_().cpu(), torch.empty(B, act, device=device).normal_().cpu()) for _ in range(n)]

    def accepted(eps):
        chain = dict(case, inputs=(p, batches * len(eps), scale, bias))
        try:
            sr.check_kinks(sr.restate(chain, torch.float32, eps=eps)[1], sr.restate(chain, torch.float64, eps=eps)[1], name)
        except AssertionError:
            return False
        return True

    eps, seeds = [], []
    for n in (K, 1, 1):
        seed = next(s for s in range(1000) if s not in seeds and accepted(eps + draws(s, n)))
        eps, seeds = eps + draws(seed, n), seeds + [seed]
    print(f"HAND_OVER_SEEDS = {tuple(seeds)}", flush=True)


def record():
    from mbrl.third_party.pytorch_sac_pranz24.sac import SAC

    out = {}
    for name in sr.RECORDED:
        case = sr.build_case(name)
        obs, act, hid, B = case["shape"]
        p, batches, scale, bias = case["inputs"]
        args = SimpleNamespace(gamma=sr.HP["gamma"], tau=sr.HP["tau"], alpha=sr.HP["alpha"], policy="Gaussian", target_update_interval=case["interval"],
                               automatic_entropy_tuning=case["tuning"], device="cpu", hidden_size=hid, lr=sr.HP["lr"],
                               target_entropy=case["target_entropy"] if case["tuning"] else None)
        space = SimpleNamespace(shape=(act,), high=np.ones(act, dtype=np.float32), low=-np.ones(act, dtype=np.float32))
        sac = SAC(obs, space, args)
        shim = sr.TinySAC.__new__(sr.TinySAC)  # (load / load_start / params walk the same attribute names on the reference's agent)
        shim.__dict__ = sac.__dict__
        shim.load(p, scale, bias)
        for which, own in (case["adam"] or {}).items():  # the case's own settings and starting state into the reference's optimizers
            group = getattr(sac, which + "_optim").param_groups[0]
            group["lr"], group["betas"], group["eps"] = own["lr"], tuple(own["betas"]), own["eps"]
        if case["start"] is not None:
            shim.load_start(case["start"])
        steps = case["start"]["steps"] if case["start"] is not None else dict(critic=0, policy=0, alpha=0)
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
                which = "alpha" if n == "log_alpha" else ("policy" if n[0] == "p" else "critic")
                assert float(st["step"]) == steps[which] + 1.0
        out[f"{name}/calibration"] = np.asarray(max(tr_dist(case["f32"]["p"][n], case["f64"]["p"][n]) for n in case["f64"]["p"]))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    if os.path.exists(OUT):  # what the file already holds must come out of this recording byte for byte: only new arrays are added
        old = np.load(OUT)
        for key in old.files:
            assert key in out and out[key].dtype == old[key].dtype and out[key].tobytes() == old[key].tobytes(), f"{key} would change"
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


def tr_dist(a, b):
    return (a.double() - b.double()).abs().max().item()


if __name__ == "__main__":
    if "--search-hand-over" in sys.argv:
        search_hand_over()
    elif "--search" in sys.argv:
        search(sys.argv[sys.argv.index("--search") + 1:])
    else:
        record()
