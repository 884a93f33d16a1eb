"""Reward tables with grouped terms (hipets.RewardTerms with level / op / 'group' / 'const' / sin, cos, exp, sqrt) ON THE GPU, in
the non-lean tail of the generic and hidden-static rollout kernels: a custom form with every construct against the oracle
evaluating the very same object, the three shipped closed-form rewards restated in the enum's op order against the enum path BIT
FOR BIT, every row-tile count, the persistent form, the fused plan, and what hipets_set_model refuses.  Observation / action
widths, the healthy box, the start state, the model seeds and the (seed, stream_id) of the in-kernel draws are those of
tests/test_gpu_reward_terms.py (imported, not copied): the dynamics do not depend on the reward, so the trajectories -- and the cap
of two candidates within 1e-4 of a box bound -- are that test's.  Tolerances: T1 (rtol 1e-5, atol 2e-6) for one step, T2
(1e-4 max(1, |ref|)) for returns."""
import dataclasses
import re

import numpy as np
import pytest
import torch

import hipets
import reward_group_forms as forms
from conftest import to_spec
from hipets import RewardTerms
from hipets import RewardTerm as T
from hipets.planning import _BoundObjective
from oracle import pets_oracle as po
from test_gpu_reward_terms import ACT, BOX, DRAWS, OBS, S0_FIX, assert_returns_close_nan_aware, box_margin, fast_members, make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
assert ACT == forms.CUSTOM_ACT and OBS >= 8
REWARD = forms.custom_terms(alive_bonus=0.5, termination_fn=BOX)
POP, P, H = 40, 5, 8
_REFERENCE = {}  # (mode, hid) -> (oracle returns, candidates to skip): computed once, shared by tests 1 and 4


def case_actions():
    g = torch.Generator().manual_seed(11)
    actions = torch.rand(POP, H, ACT, generator=g) * 2 - 1
    actions[3, 2:] = float("nan")  # candidate 3 from step 2 on, candidate 17 from step 5 on: their rows go non-finite
    actions[17, 5:] = float("nan")
    return actions, g


def reference(om, actions, s0, key, **kw):
    if key not in _REFERENCE:
        trace = {}
        ref = po.rollout(om, actions, s0, P, trace=trace, **kw)
        nobs = torch.stack(trace["next_obs"])        # [H, B, obs]
        dones = torch.stack(trace["dones"])[..., 0]  # [H, B]
        B = POP * P
        print("rows done per step", [int(d.sum()) for d in dones], "NaN returns", int(torch.isnan(ref).sum()))
        assert 0 < int(dones[0].sum()) < B or 0 < int(dones[1].sum()) < B, "degenerate case: no mix of terminated / alive rows"
        nonfinite_rows = ~torch.isfinite(nobs).all(-1)
        assert nonfinite_rows[2, 3 * P:(3 + 1) * P].all() and not nonfinite_rows[1].any()  # the NaN actions did their job
        assert torch.isnan(ref).any()  # NaN propagates through the groups
        skip = (box_margin(nobs) < 1e-4).any(0).view(POP, P).any(1)
        assert int(skip.sum()) <= 2, "too many candidates on a bound"
        _REFERENCE[key] = (ref, skip)
    return _REFERENCE[key]


# ---- 1. the custom form against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [40, 200])
@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
def test_rollouts_of_the_custom_form(engine, monkeypatch, mode, hid):
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, hid=hid, s0_fix=S0_FIX)
    engine.set_model(spec)
    B = POP * P
    assert engine.kernel_class(POP, P, H, "fast" if mode == "fast" else "device")[0] == ("hidden_static" if hid == 200 else "generic")
    actions, g = case_actions()
    seed, sid = DRAWS[hid]
    if mode == "exact":
        perms = torch.stack([torch.randperm(B, generator=g) for _ in range(H)])
        eps = torch.randn(H, B, om.out_size, generator=g)
        out = engine.rollout(actions.to(DEV), s0, P, mode="exact", perms=perms.to(DEV), eps=eps.to(DEV))
        kw = dict(perms=perms, eps=eps)
    elif mode == "device":
        out = engine.rollout(actions.to(DEV), s0, P, mode="device", seed=seed, stream_id=sid)
        kw = dict(perms=engine.device_perms(H, B, seed, sid).cpu(), eps=engine.fast_normals(H, B, seed, sid).cpu())
    else:
        out = engine.rollout(actions.to(DEV), s0, P, mode="fast", seed=seed, stream_id=sid)
        kw = dict(members=fast_members(engine, POP, P, H, seed, sid), eps=engine.fast_normals(H, B, seed, sid).cpu())
    ref, skip = reference(om, actions, s0, (mode, hid), **kw)
    assert_returns_close_nan_aware(out, ref, skip)


# ---- 2. hipets_step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
def test_single_transitions_with_nan_and_infinite_rows(engine, monkeypatch, mode):
    """rewards finite where the oracle's are, T1 there; non-finite in the same rows"""
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, s0_fix={0: 2.4, 4: -0.18}, seed=1)
    engine.set_model(spec)
    B = 120
    g = torch.Generator().manual_seed(5)
    x = torch.from_numpy(s0).repeat(B, 1) + torch.randn(B, OBS, generator=g) * 0.15
    x[7, OBS - 1] = float("nan")
    x[33, 1] = float("nan")
    x[50, OBS - 2] = float("inf")
    x[61, 3] = float("-inf")
    a = torch.rand(B, ACT, generator=g) * 2 - 1
    seed, sid = 77, 9
    if mode == "exact":
        perm = torch.randperm(B, generator=g)
        eps = torch.randn(B, om.out_size, generator=g)
        got = engine.step(x.to(DEV), a.to(DEV), mode="exact", sample=True, perm=perm.to(DEV), eps=eps.to(DEV))
        ref = po.step(om, x, a, perm=perm, eps=eps, sample=True)
    elif mode == "device":
        got = engine.step(x.to(DEV), a.to(DEV), mode="device", sample=True, seed=seed, stream_id=sid)
        perm = engine.device_perms(1, B, seed, sid).cpu()[0]
        ref = po.step(om, x, a, perm=perm, eps=engine.fast_normals(1, B, seed, sid).cpu()[0], sample=True)
    else:
        got = engine.step(x.to(DEV), a.to(DEV), mode="fast", sample=True, seed=seed, stream_id=sid)
        nwg, r = engine.fast_geometry(B, 1, 1)
        sched = engine.fast_schedule(1, nwg, seed, sid).cpu()[0]
        members = sched[torch.arange(B) // (16 * r)].long()
        ref = po.step(om, x, a, member_of_row=members, eps=engine.fast_normals(1, B, seed, sid).cpu()[0], sample=True)
    nobs, rew, done = (t.cpu() for t in got)
    r_nobs, r_rew, r_done = ref
    bad_rows = ~torch.isfinite(r_nobs).all(-1)
    assert bad_rows[7] and bad_rows[33] and bad_rows[50] and bad_rows[61] and int(bad_rows.sum()) == 4
    assert torch.equal(~torch.isfinite(nobs).all(-1), bad_rows)
    good = ~bad_rows
    assert torch.allclose(nobs[good], r_nobs[good], rtol=1e-5, atol=2e-6)  # T1
    near = box_margin(r_nobs) < 1e-4
    assert int(near.sum()) <= 2
    cmp = ~near
    assert torch.equal(done[cmp], r_done[cmp])
    assert 4 < int(r_done.sum()) < B  # a mix of terminated / alive rows beyond the four non-finite ones
    fin = torch.isfinite(r_rew[:, 0]) & cmp
    assert not torch.isfinite(r_rew[:, 0]).all()  # the table propagates NaN / inf
    assert torch.equal(torch.isfinite(rew[:, 0])[cmp], torch.isfinite(r_rew[:, 0])[cmp])
    print(f"max |reward err| {float((rew[fin] - r_rew[fin]).abs().max()):.3e} over {int(fin.sum())} rows in {float(r_rew[fin].min()):.2f} .. {float(r_rew[fin].max()):.2f}")
    assert torch.allclose(rew[fin], r_rew[fin], rtol=1e-5, atol=2e-6)


# ---- 3. the shipped forms restated in the enum's op order: bit for bit ----------------------------------------------------------
RESTATED = {  # obs, act, the table
    "cartpole_pets": (4, 1, forms.cartpole_pets_terms()),
    "pusher": (20, 7, forms.pusher_terms()),
    "halfcheetah": (17, 6, forms.halfcheetah_terms()),
}


@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("name", list(RESTATED))
def test_restated_shipped_forms_give_the_bits_of_the_enum_path(engine, name, mode):
    """Same model, seed and stream, the same kernel instance: the table machine repeats the fp32 ops of the enum form one for one
    (tests/reward_group_forms.py has the derivation per form), so rollout returns and hipets_step rewards are torch.equal."""
    obs, act, table = RESTATED[name]
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=40, seed=3, reward=name, termination="no_termination")
    s0 = (np.random.default_rng(0).standard_normal(obs) * 0.05).astype(np.float32)
    B = 120
    g = torch.Generator().manual_seed(11)
    actions = (torch.rand(POP, H, act, generator=g) * 2 - 1).to(DEV)
    x = (torch.from_numpy(s0).repeat(B, 1) + torch.randn(B, obs, generator=g) * 0.15).to(DEV)
    a = (torch.rand(B, act, generator=g) * 2 - 1).to(DEV)
    results = []
    for rew in (name, table):
        engine.set_model(dataclasses.replace(to_spec(om, obs, act), reward=rew))
        assert engine.kernel_class(POP, P, H, mode)[0] == "generic"
        results.append((engine.rollout(actions, s0, P, mode=mode, seed=321, stream_id=4).cpu(),
                        [t.cpu() for t in engine.step(x, a, mode=mode, sample=True, seed=77, stream_id=9)]))
    (ret_enum, step_enum), (ret_tab, step_tab) = results
    assert torch.isfinite(ret_enum).all() and float(ret_enum.min()) < float(ret_enum.max())
    print(f"{name} {mode}: max |return gap| {float((ret_tab - ret_enum).abs().max()):.3e}, max |reward gap| {float((step_tab[1] - step_enum[1]).abs().max()):.3e}")
    assert torch.equal(step_tab[0], step_enum[0])  # next_obs: the same model arithmetic
    assert torch.equal(step_tab[1], step_enum[1])  # rewards
    assert torch.equal(ret_tab, ret_enum)


# ---- 4. every row-tile count ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [40, 200])
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_forced_rows_per_group(engine, monkeypatch, r, hid):
    """R = 1 .. 4 of the generic and the hidden-static instance (the register-tight ones among them), DEVICE: T2 against the oracle"""
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, hid=hid, s0_fix=S0_FIX)
    engine.set_model(spec)
    B = POP * P
    assert engine.kernel_class(POP, P, H, "device", rows_per_group=r) == ("hidden_static" if hid == 200 else "generic", r)
    actions, _ = case_actions()
    seed, sid = DRAWS[hid]
    out = engine.rollout(actions.to(DEV), s0, P, mode="device", seed=seed, stream_id=sid, rows_per_group=r)
    kw = dict(perms=engine.device_perms(H, B, seed, sid).cpu(), eps=engine.fast_normals(H, B, seed, sid).cpu())
    ref, skip = reference(om, actions, s0, ("device", hid), **kw)
    assert_returns_close_nan_aware(out, ref, skip)


# ---- 5. / 6. launch forms -------------------------------------------------------------------------------------------------------
def test_persistent_device_rollout_equals_per_step_launches(engine, monkeypatch):
    """The hidden-static instance at ~200 logical workgroups: one persistent launch == H per-step launches, bit for bit."""
    P_, H_, M, pop = 20, 4, 5, 320
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, hid=200, s0_fix=S0_FIX)
    engine.set_model(spec)
    assert engine.kernel_class(pop, P_, H_, "device", rows_per_group=2) == ("hidden_static", 2)
    assert M * -(-(pop * P_ // M) // (16 * 2)) <= 256  # one workgroup per CU: the persistent form applies
    actions = (torch.rand(pop, H_, ACT, generator=torch.Generator().manual_seed(11)) * 2 - 1).to(DEV)
    kw = dict(mode="device", seed=77, stream_id=9, rows_per_group=2)
    a = engine.rollout(actions, s0, P_, **kw).clone()
    again = engine.rollout(actions, s0, P_, **kw).clone()
    engine.set_persistent(False)
    try:
        b = engine.rollout(actions, s0, P_, **kw).clone()
    finally:
        engine.set_persistent(True)
    assert torch.isfinite(a).all() and torch.equal(a, again) and torch.equal(a, b)
    assert float(a.min()) < float(a.max())


def test_fused_plan_equals_per_iteration_path(engine, monkeypatch):
    """CEMOptimizer.optimize over a model with a grouped table: the one-call fused plan and the per-iteration path (what a callback
    forces) return the same plan bit for bit."""
    H_, P_, pop = 10, 5, 120
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, hid=200, s0_fix=S0_FIX)
    fn = hipets.make_eval_fn(spec, P_, engine=engine, seed=13, mode="device")
    assert isinstance(fn, hipets.HipTrajectoryEvalFn)
    obj = _BoundObjective(fn, s0)
    lb, ub = [[-1.0] * ACT] * H_, [[1.0] * ACT] * H_
    a = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    b = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    x0 = torch.zeros(H_, ACT)
    plan = a.optimize(obj, x0=x0)
    assert torch.isfinite(plan).all() and float(plan.abs().max()) > 0
    assert torch.equal(plan, b.optimize(obj, x0=x0, callback=lambda *_: None))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_set_model_checks_well_formedness_itself(engine, monkeypatch):
    """hipets_set_model validates the table itself (a C client has no Python layer in front of it): HIPETS_ERR_INVALID_ARGUMENT with
    the offending entry named.  The Python-side checks are switched off for the purpose."""
    from hipets import _lib

    om = po.make_synthetic_model(OBS, ACT, ensemble_size=5, hid=40, seed=3)
    base = to_spec(om, OBS, ACT)
    monkeypatch.setattr(RewardTerms, "validate", lambda self, *a, **k: None)
    monkeypatch.setattr(hipets.ModelSpec, "validate", lambda self: None)
    monkeypatch.setitem(_lib.TERM_OP, "pow", 7)
    cases = [
        ([T("linear", 0), T("linear", 0, level=3)], "reward term 1: level 3 outside [0, 2]"),
        ([T("linear", 0, level=2), T("linear", 0, source="group", level=2)], "reward term 1: GROUP at level 2 has no deeper group"),
        ([T("linear", 0), T("linear", 0, source="group")], "reward term 1: GROUP consumes an empty group"),
        ([T("linear", 0, level=1), T("linear", 0, source="group"), T("linear", 0, source="group")], "reward term 2: GROUP consumes an empty group"),
        ([T("linear", 0, level=1), T("linear", 1)], "reward term 0: the group at level 1 is left open at the end of the table"),
        ([T("linear", 0, level=2), T("linear", 1, level=2), T("linear", 0, level=1), T("linear", 0, source="group")],
         "reward term 1: the group at level 2 is left open at the end of the table"),
        ([T("linear", 0), T("linear", 1, level=1, op="mul")], "reward term 1: mul / div into an empty group (level 1"),
        ([T("linear", 0, op="pow")], "reward term 0: unknown op 7"),
        ([T("linear", 0, level=1), T("linear", 0, j=1, source="group")], "reward term 1: j = 1 is set on a GROUP / CONST entry"),
    ]
    for terms, msg in cases:
        with pytest.raises(hipets.HipetsError, match=re.escape(msg)) as exc:
            engine.set_model(dataclasses.replace(base, reward=RewardTerms(terms)))
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT, msg
    monkeypatch.undo()
    engine.set_model(dataclasses.replace(base, reward=REWARD, termination=BOX))  # and the engine still takes a good model
    assert engine.rollout(torch.zeros(40, 2, ACT, device=DEV), np.zeros(OBS, np.float32), 5, mode="device").shape == (40,)
