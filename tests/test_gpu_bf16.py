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
from bf16_restatement import (CFG2, EDGE_CASES, T1_ATOL, T2_REL, edge_case, emulated_rollout, reference_rollout, scaled_case, threshold_margin,
                               tolerance)
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
    the candidates may be dropped -- a kernel whose heights differ from the emulation by more than 1e-4 fails here, by design.
    cfg2_H1: at H = 1 the return sees output columns 0 and obs only (the mean and log-variance of state dim 0); on the CPU, zeroing the
    last mean or log-variance column moves no emulated return, the last input row moves one by 26 x tol and the last hidden row of
    layer 1 by 10 x tol.  The other output columns are pinned by the edge cases below (H = 4, gained edge columns)."""
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
    that runs is the bf16 one at R = 3.  (At H = 1 the return sees output columns 0 and obs only -- the mean and log-variance of state
    dim 0: no other output column can move it.)"""
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


# ---------------------------------------------------------------------------------------------------------------------
# The edges of the two instance families (tests/bf16_restatement.py EDGE_CASES; tests/test_bf16_host.py holds the CPU conditions of
# every case: each single-column loss moves a return by >= 4 tol, the reference's own summation order uses <= tol / 4)
# ---------------------------------------------------------------------------------------------------------------------
KERNEL_CLASS = {"bf16": "bf16", "bf16x3": "fused"}


def edge_replay(engine, monkeypatch, case, prec, mode):
    """One edge case in arithmetic `prec`: (hip, ref, D, tol, om, actions, s0) -- the kernel's returns, the reference of `prec` on the
    draws the engine exports, D = max |emu - f32| and the tolerance (bf16_restatement.tolerance).  Asserts what does not depend on the
    arithmetic: the instance is the mode's own at three row tiles, everything is finite, no height is within 1e-4 of a threshold."""
    om, actions, s0, _, _ = edge_case(case.obs, case.act, case.pop, case.P, case.H, seed=case.seed, gain=case.gain, g_in=case.g_in,
                                      g_lv=case.g_lv, **case.mkw)
    engine.set_model(to_spec(om, case.obs, case.act, precision=prec))
    assert engine.kernel_class(case.pop, case.P, case.H, mode=mode) == (KERNEL_CLASS[prec], 3)
    hip = engine.rollout(actions.to(DEV), s0, case.P, mode=mode, seed=SEED, stream_id=SID).cpu()
    kw = _draws(engine, case.pop, case.P, case.H, mode)
    tr = {}
    ref = reference_rollout(monkeypatch, prec, om, actions, s0, case.P, trace=tr, **kw)
    f32 = po.rollout(om, actions, s0, case.P, **kw)
    emu = ref if prec == "bf16" else reference_rollout(monkeypatch, "bf16", om, actions, s0, case.P, **kw)
    assert torch.isfinite(hip).all() and torch.isfinite(ref).all()
    # the keep-mask of the replay tests above is empty here (cap: 0 candidates dropped)
    assert threshold_margin(om, tr) >= 1e-4, threshold_margin(om, tr)
    D = (emu - f32).abs().max().item()
    return hip, ref, D, tolerance(prec, ref, D), om, actions, s0


def edge_parity_line(tag, case, prec, mode, err, D, tol):
    print(tag + " " + json.dumps({"case": case.name, "precision": prec, "mode": mode, "max_hip_minus_ref": err.max().item(), "D": D,
                                  "ratio": err.max().item() / D, "of_tol": (err / tol).max().item()}))


@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: c.name)
def test_bf16_edge_cases_replayed_through_the_bf16_emulation(engine, monkeypatch, case, mode):
    """|hip_i - emu_i| <= tol_i = max(1e-4 max(1, |emu_i|), D / 4) for EVERY candidate (no candidate is masked), all values finite,
    the bf16 instance at three row tiles."""
    hip, emu, D, tol, *_ = edge_replay(engine, monkeypatch, case, "bf16", mode)
    err = (hip - emu).abs()
    edge_parity_line("BF16_PARITY", case, "bf16", mode, err, D, tol)
    bad = err > tol
    assert not bad.any(), f"max |hip - emu| {err.max():.3e} (D {D:.3e}, {(err / tol).max():.2f} x tol) at candidate {int(bad.nonzero()[0])}"


# models next to the two families: (obs, act, model kwargs).  None has an instance in this arithmetic
REFUSED = {
    "obs16": (16, 6, dict(hid=200)), "obs25": (25, 6, dict(hid=200)),
    "obs40_humanoid": (40, 17, dict(hid=200, termination="humanoid")), "obs49_humanoid": (49, 17, dict(hid=200, termination="humanoid")),
    "hid192": (17, 6, dict(hid=192)), "hid209": (17, 6, dict(hid=209)),
    "obs17_humanoid": (17, 6, dict(hid=200, termination="humanoid")),
    "obs_process": (17, 6, dict(hid=200, obs_process="halfcheetah")),
    "learned_rewards": (17, 6, dict(hid=200, learned_rewards=True, reward=None)),
    "relu": (17, 6, dict(hid=200, activation="relu")),
    "normalizer_f32": (17, 6, dict(hid=200, normalizer="f32")),
    "expectation": (17, 6, dict(hid=200, propagation="expectation")),
    "deterministic": (17, 6, dict(hid=200, deterministic=True)),
}
ACCEPTED = next(c for c in EDGE_CASES if c.name == "A_pop7")


def assert_refused_then_accepted(engine, prec, match, obs, act, mkw):
    """A model without an instance raises in both launch modes -- it never runs another arithmetic --, and the accepted model set
    right after it returns what it returned before."""
    c = ACCEPTED
    good, actions, s0, _, _ = edge_case(c.obs, c.act, c.pop, c.P, c.H, seed=c.seed, gain=c.gain, g_in=c.g_in, g_lv=c.g_lv, **c.mkw)
    engine.set_model(to_spec(good, c.obs, c.act, precision=prec))
    before = {m: engine.rollout(actions.to(DEV), s0, c.P, mode=m, seed=SEED, stream_id=SID).clone() for m in ("device", "fast")}
    om = po.make_synthetic_model(obs, act, ensemble_size=5, seed=3, **mkw)
    for m in ("device", "fast"):
        with pytest.raises(hipets.HipetsError, match=match):
            engine.set_model(to_spec(om, obs, act, precision=prec))
            engine.rollout(torch.zeros(40, 4, act, device=DEV), np.zeros(obs, np.float32), 5, mode=m, seed=SEED, stream_id=SID)
    engine.set_model(to_spec(good, c.obs, c.act, precision=prec))
    for m in ("device", "fast"):
        after = engine.rollout(actions.to(DEV), s0, c.P, mode=m, seed=SEED, stream_id=SID)
        assert torch.isfinite(after).all() and torch.equal(after, before[m])
        assert engine.kernel_class(c.pop, c.P, c.H, mode=m) == (KERNEL_CLASS[prec], 3)


@pytest.mark.parametrize("name", list(REFUSED))
def test_bf16_refuses_models_next_to_its_families(engine, name):
    assert_refused_then_accepted(engine, "bf16", "precision bf16:", *REFUSED[name])
