"""precision='bf16' (a SEPARATELY reported, reduced-precision arithmetic mode, include/hipets.h HIPETS_PREC_BF16) on the GPU, with
its own parity: the kernel is compared with the oracle run through the bf16 restatement (tests/bf16_restatement.py: both operands of
every linear layer rounded to bf16 nearest-even, fp32 accumulation), on the draws the engine exports, with the weights scaled by 2
(tests/test_bf16_host.py shows that this case tells bf16 from fp32 by 33x the fp32 one-step tolerance).

Definitions: D = max |emu - f32| over candidates (both on the CPU, same draws); tol_i = max(1e-4 max(1, |emu_i|), D / 4).  A kernel
with another rounding rule (truncation, rounding before SiLU, an unrounded input layer) lands at about 1 x D; different fp32 summation
orders flip an occasional activation across a bf16 boundary, far below D / 4.

Measured on MI355X (profiles/bf16_parity.json holds every case and mode): max |hip - emu| / D = 0.06 / 0.07 at cfg2 H = 1 (DEVICE /
FAST), 0.14 / 0.16 at cfg5 H = 5, 0.22 / 0.19 at cfg2 H = 30, 0.003 / 0.0006 at cfg4 (where |hip - emu| <= 5e-5 is inside the fp32
mode's own T2 bound and D is dominated by candidates that terminate at different steps in bf16 and fp32).  The ratio grows with the
horizon: with weights x 2 the rollout amplifies a difference by ~1400x over 30 steps (D itself goes from 7e-5 to 0.10), and the
occasional activation that lands on the other side of a bf16 boundary under another fp32 summation order is amplified alike."""
import json

import numpy as np
import pytest
import torch

import hipets
from bf16_restatement import CFG2, T1_ATOL, T2_REL, emulated_rollout, scaled_case
from conftest import to_spec
from hipets.planning import _BoundObjective
from oracle import device_draws
from oracle import pets_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, SID = 31, 4
CFG4 = (45, 17, 1036, 20, dict(ensemble_size=7, hid=200, elite=[0, 1, 2, 3, 4], termination="humanoid"))
CFG5 = (17, 6, 2000, 20, dict(ensemble_size=5, hid=200))
REPLAY_CASES = [(CFG2, 30), (CFG2, 1), (CFG5, 5), (CFG4, 4)]


def _draws(engine, pop, P, H, mode):
    """The engine's own draws for (SEED, SID) as oracle arguments (of the model the engine holds: its FAST geometry)."""
    kw = dict(eps=engine.fast_normals(H, pop * P, SEED, SID).cpu())
    if mode == "device":
        kw["perms"] = engine.device_perms(H, pop * P, SEED, SID).cpu()
    else:
        nwg, r = engine.fast_geometry(pop, P, H)
        sched = engine.fast_schedule(H, nwg, SEED, SID).cpu()
        wg = device_draws.fast_row_workgroup(torch.arange(pop * P), P, r)
        kw["members"] = torch.stack([sched[t][wg].long() for t in range(H)])
    return kw


def _run(engine, monkeypatch, case, H, mode):
    """(hip, emu, f32, trace of the emulation) for one case: the bf16 kernel, the emulation and the fp32 oracle on the same draws."""
    obs, act, pop, P, mkw = case
    om, actions, s0, _, _ = scaled_case(obs, act, pop, P, H, **mkw)
    engine.set_model(to_spec(om, obs, act, precision="bf16"))
    hip = engine.rollout(actions.to(DEV), s0, P, mode=mode, seed=SEED, stream_id=SID).cpu()
    kw = _draws(engine, pop, P, H, mode)
    tr = {}
    emu = emulated_rollout(monkeypatch, om, actions, s0, P, trace=tr, **kw)
    f32 = po.rollout(om, actions, s0, P, **kw)
    return hip, emu, f32, tr


@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("case,H", REPLAY_CASES, ids=["cfg2_H30", "cfg2_H1", "cfg5_H5", "cfg4_H4"])
def test_bf16_rollouts_replayed_through_the_bf16_emulation(engine, monkeypatch, case, H, mode):
    """|hip_i - emu_i| <= tol_i, all values finite.  cfg4 (humanoid termination: the thresholds at heights 1.0 and 2.0 are
    discontinuities): candidates with any row whose EMULATED height is within 1e-4 of a threshold are not compared, and at most 2 % of
    the candidates may be dropped -- a kernel whose heights differ from the emulation by more than 1e-4 fails here, by design."""
    pop, P = case[2], case[3]
    hip, emu, f32, tr = _run(engine, monkeypatch, case, H, mode)
    assert torch.isfinite(hip).all() and torch.isfinite(emu).all()
    keep = torch.ones(pop, dtype=torch.bool)
    if case[4].get("termination") == "humanoid":
        z = torch.stack([n[:, 0] for n in tr["next_obs"]])
        keep = ~(torch.minimum((z - 1.0).abs(), (z - 2.0).abs()) < 1e-4).any(0).view(pop, P).any(1)
        assert int((~keep).sum()) <= 0.02 * pop, int((~keep).sum())
    D = (emu - f32).abs().max().item()
    err = (hip - emu).abs()
    tol = torch.maximum(T2_REL * torch.clamp(emu.abs(), min=1.0), torch.tensor(D / 4))
    print("BF16_PARITY " + json.dumps({"case": f"obs{case[0]}_pop{pop}x{P}_H{H}", "mode": mode, "max_hip_minus_emu": err[keep].max().item(), "D": D,
                                       "ratio": err[keep].max().item() / D, "dropped": int((~keep).sum())}))
    bad = (err > tol) & keep
    assert not bad.any(), f"max |hip - emu| {err[keep].max():.3e} (D {D:.3e}) at candidate {int(bad.nonzero()[0])}"


@pytest.mark.parametrize("mode", ["device", "fast"])
def test_bf16_keeps_the_elites_of_a_cfg2_iteration(engine, monkeypatch, mode):
    """cfg2, H = 30: the top 50 of the bf16 returns are the top 50 of the fp32 oracle's, candidates whose fp32 value lies within D of
    the 50th excepted."""
    obs, act, pop, P, mkw = CFG2
    hip, emu, f32, _ = _run(engine, monkeypatch, CFG2, 30, mode)
    D = (emu - f32).abs().max().item()
    k = 50
    top_f32 = set(torch.topk(f32, k).indices.tolist())
    top_hip = set(torch.topk(hip, k).indices.tolist())
    kth = torch.topk(f32, k).values[-1].item()
    unsure = set(((f32 - kth).abs() <= D).nonzero().flatten().tolist())
    assert (top_f32 ^ top_hip) <= unsure, sorted((top_f32 ^ top_hip) - unsure)


@pytest.mark.parametrize("mode", ["device", "fast"])
def test_bf16_is_really_bf16(engine, monkeypatch, mode):
    """cfg2, H = 1: the kernel differs from the fp32 oracle by more than 10 x the fp32 mode's one-step tolerance, and the instance
    that runs is the bf16 one at R = 3."""
    obs, act, pop, P, mkw = CFG2
    hip, emu, f32, _ = _run(engine, monkeypatch, CFG2, 1, mode)
    assert (hip - f32).abs().max().item() > 10 * T1_ATOL
    assert engine.kernel_class(pop, P, 30, mode=mode) == ("bf16", 3)
    assert engine.kernel_class(pop, P, 1, mode=mode) == ("bf16", 3)


def test_bf16_fused_plan_equals_per_iteration_path_and_needs_a_specialised_shape(engine):
    obs, act, H, P, pop = 17, 6, 10, 5, 120
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=200, seed=3)
    fn = hipets.make_eval_fn(to_spec(om, obs, act, precision="bf16"), P, engine=engine, seed=13, mode="device")
    obj = _BoundObjective(fn, (np.random.default_rng(1).standard_normal(obs) * 0.1).astype(np.float32))
    lb, ub = [[-1.0] * act] * H, [[1.0] * act] * H
    a = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    b = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    x0 = torch.zeros(H, act)
    assert torch.equal(a.optimize(obj, x0=x0), b.optimize(obj, x0=x0, callback=lambda *_: None))
    # no instance for other shapes / calls: fails loudly, never falls back to another arithmetic
    om2 = po.make_synthetic_model(obs, act, ensemble_size=5, hid=64, seed=3)
    engine.set_model(to_spec(om2, obs, act, precision="bf16"))
    with pytest.raises(hipets.HipetsError, match="precision bf16:"):
        engine.rollout(torch.zeros(40, 3, act, device=DEV), np.zeros(obs, np.float32), 5, mode="device")
    engine.set_model(to_spec(om, obs, act, precision="bf16"))
    with pytest.raises(hipets.HipetsError, match="precision bf16:"):  # injected eps need the generic kernel
        engine.rollout(torch.zeros(40, 3, act, device=DEV), np.zeros(obs, np.float32), 5, mode="exact",
                       perms=torch.stack([torch.randperm(200) for _ in range(3)]).to(DEV), eps=torch.zeros(3, 200, obs, device=DEV))


@pytest.mark.parametrize("mode", ["device", "fast"])
def test_bf16_rollouts_are_deterministic(engine, mode):
    obs, act, pop, P, mkw = CFG2
    om, actions, s0, _, _ = scaled_case(obs, act, pop, P, 30, **mkw)
    engine.set_model(to_spec(om, obs, act, precision="bf16"))
    a = engine.rollout(actions.to(DEV), s0, P, mode=mode, seed=7, stream_id=2).clone()
    b = engine.rollout(actions.to(DEV), s0, P, mode=mode, seed=7, stream_id=2).clone()
    assert torch.equal(a, b)
