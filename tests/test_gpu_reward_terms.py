"""The parametric closed forms -- a reward term table (hipets.RewardTerms, HIPETS_REW_TERMS) and a healthy box
(hipets.BoxTermination, HIPETS_TERM_BOX) -- ON THE GPU, in the non-lean tail of the generic and hidden-static rollout kernels:
against the oracle evaluating the very same objects as torch callables (registered under fresh names in po.REWARD_FNS /
po.TERMINATION_FNS), against the enum path for the shipped forms restated as tables, across launch forms, and where the library
refuses them.  Shapes and tolerances are those of tests/test_gpu_closed_forms.py: E 5, pop 40, P 5, H 8; hipets_step at B 120;
T1 (rtol 1e-5, atol 2e-6) for one step, T2 (1e-4 max(1, |ref|)) for returns; candidates with a row within 1e-4 of a box bound
are excluded (the comparison is discontinuous there), at most two per case."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import hipets
from conftest import to_spec
from hipets import BoxTermination, RewardTerms
from hipets import Interval as I
from hipets import RewardTerm as T
from hipets.planning import _BoundObjective
from oracle import device_draws
from oracle import pets_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, ACT = 9, 3

# a form no enum covers: 0.25 - 2 (s0 - 1.1)^2 - 0.7 |s2 - s5| + s3 - 0.3 (s6 - s7)^2 - 0.05 sum a^2 + 0.5 (1 - done)
BOX = BoxTermination([I(0, -0.5, 2.5, hi_open=True), I(4, -1.5, math.inf, lo_open=True)], require_finite=True)
REWARD = RewardTerms([T("square", 0, w=-2.0, c=1.1), T("abs", 2, w=-0.7, j=5), T("linear", 3), T("square", 6, w=-0.3, j=7)]
                     + [T("square", i, w=-0.05, source="act") for i in range(ACT)], bias=0.25, alive_bonus=0.5, termination_fn=BOX)
S0_FIX = {0: 0.96, 4: -0.18}
# (seed, stream_id) of the in-kernel draws per hidden width: chosen on the CPU from the exported draws so that the case keeps the
# cap of two excluded candidates and its mix of terminated / alive rows
DRAWS = {40: (321, 4), 200: (321, 4)}


def box_margin(nobs):
    """distance of every row of nobs [.., obs] from the nearest finite bound of BOX"""
    x = torch.nan_to_num(nobs, nan=1e9, posinf=1e9, neginf=-1e9)
    return torch.stack([(x[..., 0] + 0.5).abs(), (x[..., 0] - 2.5).abs(), (x[..., 4] + 1.5).abs()]).min(0).values


def register(monkeypatch, reward, termination, tag="parametric"):
    """the oracle looks functions up by name: the objects themselves, under fresh names -> (reward name, termination name)"""
    names = []
    for table, fn, kind in ((po.REWARD_FNS, reward, "rew"), (po.TERMINATION_FNS, termination, "term")):
        if isinstance(fn, str) or fn is None:
            names.append(fn)
        else:
            monkeypatch.setitem(table, f"{tag}_{kind}", fn)
            names.append(f"{tag}_{kind}")
    return names


def make(monkeypatch, obs, act, reward, termination, hid=40, s0_fix=None, seed=0, **mkw):
    """(oracle model, its ModelSpec with the OBJECTS as reward / termination, start state)"""
    rew_name, term_name = register(monkeypatch, reward, termination)
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=hid, seed=seed + 3, reward=rew_name, termination=term_name, **mkw)
    spec = dataclasses.replace(to_spec(om, obs, act), reward=reward, termination=termination)
    s0 = (np.random.default_rng(seed).standard_normal(obs) * 0.05).astype(np.float32)
    for d, v in (s0_fix or {}).items():
        s0[d] = v
    return om, spec, s0


def fast_members(engine, pop, P, H, seed, sid):
    nwg, r = engine.fast_geometry(pop, P, H, 0)
    sched = engine.fast_schedule(H, nwg, seed, sid).cpu()
    wg = device_draws.fast_row_workgroup(torch.arange(pop * P), P, r)
    return torch.stack([sched[t][wg].long() for t in range(H)])


def assert_returns_close_nan_aware(out, ref, skip=None):
    out, ref = out.detach().cpu(), ref.detach().cpu()
    keep = torch.ones_like(ref, dtype=torch.bool) if skip is None else ~skip
    assert torch.equal(torch.isnan(out)[keep], torch.isnan(ref)[keep]), "NaN returns in different places"
    ok = keep & ~torch.isnan(ref)
    assert torch.isfinite(out[ok]).all()
    tol = 1e-4 * torch.clamp(ref[ok].abs(), min=1.0)  # T2
    err = (out[ok] - ref[ok]).abs()
    print(f"max |err| {float(err.max()):.3e} over {int(ok.sum())} returns in {float(ref[ok].min()):.2f} .. {float(ref[ok].max()):.2f}")
    assert (err <= tol).all(), f"max err {err.max():.3e}"


# ---- 1. a form no enum covers, against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [40, 200])
@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
def test_rollouts_of_a_form_no_enum_covers(engine, monkeypatch, mode, hid):
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, hid=hid, s0_fix=S0_FIX)
    engine.set_model(spec)
    pop, P, H = 40, 5, 8
    B = pop * P
    assert engine.kernel_class(pop, P, H, "fast" if mode == "fast" else "device")[0] == ("hidden_static" if hid == 200 else "generic")
    g = torch.Generator().manual_seed(11)
    actions = torch.rand(pop, H, ACT, generator=g) * 2 - 1
    actions[3, 2:] = float("nan")  # candidate 3 from step 2 on, candidate 17 from step 5 on: their rows go non-finite
    actions[17, 5:] = float("nan")
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
        kw = dict(members=fast_members(engine, pop, P, H, seed, sid), eps=engine.fast_normals(H, B, seed, sid).cpu())
    trace = {}
    ref = po.rollout(om, actions, s0, P, trace=trace, **kw)
    nobs = torch.stack(trace["next_obs"])        # [H, B, obs]
    dones = torch.stack(trace["dones"])[..., 0]  # [H, B]
    print("rows done per step", [int(d.sum()) for d in dones], "NaN returns", int(torch.isnan(ref).sum()))
    assert 0 < int(dones[0].sum()) < B or 0 < int(dones[1].sum()) < B, "degenerate case: no mix of terminated / alive rows"
    nonfinite_rows = ~torch.isfinite(nobs).all(-1)
    assert nonfinite_rows[2, 3 * P:(3 + 1) * P].all() and not nonfinite_rows[1].any()  # the NaN actions did their job
    assert dones[2, 3 * P:(3 + 1) * P].all()  # require_finite
    assert torch.isnan(ref).any()  # a candidate whose rows were all alive when they went non-finite: NaN propagates through the table
    skip = (box_margin(nobs) < 1e-4).any(0).view(pop, P).any(1)
    assert int(skip.sum()) <= 2, "too many candidates on a bound: pick another seed"
    assert_returns_close_nan_aware(out, ref, skip)


# ---- 2. hipets_step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
def test_single_transitions_with_nan_and_infinite_rows(engine, monkeypatch, mode):
    """next_obs / reward T1 where the reference is finite, non-finite in the same rows; done flags equal away from the bounds.
    The start state sits next to the upper bound of dim 0, so the rows straddle it."""
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, s0_fix={0: 2.4, 4: -0.18}, seed=1)
    engine.set_model(spec)
    B = 120
    g = torch.Generator().manual_seed(5)
    x = torch.from_numpy(s0).repeat(B, 1) + torch.randn(B, OBS, generator=g) * 0.15
    x[7, OBS - 1] = float("nan")
    x[33, 1] = float("nan")
    x[50, OBS - 2] = float("inf")
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
    assert bad_rows[7] and bad_rows[33] and bad_rows[50] and int(bad_rows.sum()) == 3
    assert torch.equal(~torch.isfinite(nobs).all(-1), bad_rows)
    good = ~bad_rows
    assert torch.allclose(nobs[good], r_nobs[good], rtol=1e-5, atol=2e-6)  # T1
    near = box_margin(r_nobs) < 1e-4
    assert int(near.sum()) <= 2
    cmp = ~near
    assert torch.equal(done[cmp], r_done[cmp])
    print("rows done", int(r_done.sum()), "of", B)
    assert 3 < int(r_done.sum()) < B  # a mix of terminated / alive rows beyond the three non-finite ones
    assert r_done[7] and r_done[33] and r_done[50]  # require_finite
    fin = torch.isfinite(r_rew[:, 0]) & cmp
    assert not torch.isfinite(r_rew[:, 0]).all()  # the table propagates NaN / inf
    assert torch.equal(torch.isfinite(rew[:, 0])[cmp], torch.isfinite(r_rew[:, 0])[cmp])
    assert torch.allclose(rew[fin], r_rew[fin], rtol=1e-5, atol=2e-6)


# ---- 3. the shipped forms restated, against the enum path ---------------------------------------------------------------------
THR = 12 * 2 * math.pi / 360
CARTPOLE_BOX = BoxTermination([I(0, -2.4, 2.4, lo_open=True, hi_open=True), I(2, -THR, THR, lo_open=True, hi_open=True)])


def halfcheetah_terms(act):
    return RewardTerms([T("linear", 0)] + [T("square", i, w=-0.1, source="act") for i in range(act)])


def hopper_box(obs):
    return BoxTermination([I(0, 0.7, math.inf, lo_open=True), I(1, -0.2, 0.2, lo_open=True, hi_open=True)]
                          + [I(d, -100.0, 100.0, lo_open=True, hi_open=True) for d in range(1, obs)], require_finite=True)


PUSHER_GOAL = (0.45, -0.05, -0.323)
RESTATED = {  # obs, act, enum (reward, termination), restated (reward, termination), start-state overrides
    "halfcheetah": (17, 6, ("halfcheetah", "no_termination"), (halfcheetah_terms(6), "no_termination"), {}),
    "pusher": (20, 7, ("pusher", "no_termination"),
               (RewardTerms([T("abs", 14 + k, w=-0.5, j=17 + k) for k in range(3)] + [T("abs", 17 + k, w=-1.25, c=PUSHER_GOAL[k]) for k in range(3)]
                            + [T("square", i, w=-0.1, source="act") for i in range(7)]), "no_termination"), {}),
    "cartpole": (4, 1, ("cartpole", "cartpole"), (RewardTerms([], alive_bonus=1.0, termination_fn=CARTPOLE_BOX), CARTPOLE_BOX), {0: 2.3}),
    "hopper_halfcheetah": (11, 3, ("halfcheetah", "hopper"), (halfcheetah_terms(3), hopper_box(11)), {0: 0.76, 1: 0.0}),
}


@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("name", list(RESTATED))
def test_restated_shipped_forms_equal_the_enum_path(engine, name, mode):
    """Same model, seed and stream: the table / box run computes what the built-in closed form computes -- returns within T2
    (a table sums its action costs in another order than the enum's loop), hipets_step done flags equal."""
    obs, act, enum, restated, s0_fix = RESTATED[name]
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=40, seed=3, reward=enum[0], termination=enum[1])
    s0 = (np.random.default_rng(0).standard_normal(obs) * 0.05).astype(np.float32)
    for d, v in s0_fix.items():
        s0[d] = v
    pop, P, H, B = 40, 5, 8, 120
    g = torch.Generator().manual_seed(11)
    actions = (torch.rand(pop, H, act, generator=g) * 2 - 1).to(DEV)
    x = (torch.from_numpy(s0).repeat(B, 1) + torch.randn(B, obs, generator=g) * 0.15).to(DEV)
    a = (torch.rand(B, act, generator=g) * 2 - 1).to(DEV)
    results = []
    for rew, term in (enum, restated):
        engine.set_model(dataclasses.replace(to_spec(om, obs, act), reward=rew, termination=term))
        assert engine.kernel_class(pop, P, H, mode)[0] == "generic"
        results.append((engine.rollout(actions, s0, P, mode=mode, seed=321, stream_id=4).cpu(),
                        [t.cpu() for t in engine.step(x, a, mode=mode, sample=True, seed=77, stream_id=9)]))
    (ret_enum, step_enum), (ret_tab, step_tab) = results
    assert torch.isfinite(ret_enum).all()
    assert_returns_close_nan_aware(ret_tab, ret_enum)
    assert torch.equal(step_tab[0], step_enum[0])  # next_obs: the same model arithmetic
    assert torch.equal(step_tab[2], step_enum[2])  # dones
    assert torch.allclose(step_tab[1], step_enum[1], rtol=1e-5, atol=2e-6)
    if enum[1] != "no_termination":
        assert 0 < int(step_enum[2].sum()) < B, "degenerate case: no mix of terminated / alive rows"
        assert float(ret_enum.min()) < float(ret_enum.max())


# ---- 4. determinism and form equality -------------------------------------------------------------------------------------------
def test_persistent_device_rollout_equals_per_step_launches(engine, monkeypatch):
    """The hidden-static instance at ~200 logical workgroups: one persistent launch == H per-step launches, bit for bit."""
    P, H, M, pop = 20, 4, 5, 320
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, hid=200, s0_fix=S0_FIX)
    engine.set_model(spec)
    cls, r = engine.kernel_class(pop, P, H, "device", rows_per_group=2)
    assert (cls, r) == ("hidden_static", 2)
    assert M * -(-(pop * P // M) // (16 * r)) <= 256  # one workgroup per CU: the persistent form applies
    actions = (torch.rand(pop, H, ACT, generator=torch.Generator().manual_seed(11)) * 2 - 1).to(DEV)
    kw = dict(mode="device", seed=77, stream_id=9, rows_per_group=2)
    a = engine.rollout(actions, s0, P, **kw).clone()
    again = engine.rollout(actions, s0, P, **kw).clone()
    engine.set_persistent(False)
    try:
        b = engine.rollout(actions, s0, P, **kw).clone()
    finally:
        engine.set_persistent(True)
    assert torch.isfinite(a).all() and torch.equal(a, again) and torch.equal(a, b)
    assert float(a.min()) < float(a.max())


def test_fused_plan_equals_per_iteration_path(engine, monkeypatch):
    """CEMOptimizer.optimize over a model with the parametric forms: the one-call fused plan and the per-iteration path (what a
    callback forces) return the same plan bit for bit -- the forms are on the fused plans' path, not beside it."""
    H, P, pop = 10, 5, 120
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, hid=200, s0_fix=S0_FIX)
    fn = hipets.make_eval_fn(spec, P, engine=engine, seed=13, mode="device")
    assert isinstance(fn, hipets.HipTrajectoryEvalFn)
    obj = _BoundObjective(fn, s0)
    lb, ub = [[-1.0] * ACT] * H, [[1.0] * ACT] * H
    a = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    b = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    x0 = torch.zeros(H, ACT)
    plan = a.optimize(obj, x0=x0)
    assert torch.isfinite(plan).all() and float(plan.abs().max()) > 0
    assert torch.equal(plan, b.optimize(obj, x0=x0, callback=lambda *_: None))


# ---- 5. batched start states ----------------------------------------------------------------------------------------------------
def test_two_environments_in_one_device_launch(engine, monkeypatch):
    """n_env = 2: ONE balanced permutation per step over the rows of both environments; each environment's returns replayed
    through the oracle from its own start state."""
    om, spec, s0 = make(monkeypatch, OBS, ACT, REWARD, BOX, s0_fix=S0_FIX)
    engine.set_model(spec)
    pop_env, n_env, P, H = 20, 2, 5, 8
    pop, B, M = pop_env * n_env, pop_env * n_env * P, 5
    g = torch.Generator().manual_seed(11)
    actions = torch.rand(pop, H, ACT, generator=g) * 2 - 1
    s0s = np.stack([s0, s0 + (torch.randn(OBS, generator=g) * 0.05).numpy().astype(np.float32)])
    s0s[1, 0] = 2.2  # the second environment starts next to the other bound of dim 0
    seed, sid = 5, 9
    out = engine.rollout(actions.to(DEV), s0s, P, mode="device", seed=seed, stream_id=sid, n_env=n_env).cpu()
    eps = engine.fast_normals(H, B, seed, sid).cpu()
    perms = engine.device_perms(H, B, seed, sid).cpu()
    members = torch.empty(H, B, dtype=torch.long)  # slot j holds row perms[t][j] and runs member j // (B / M)
    for t in range(H):
        members[t][perms[t]] = torch.arange(B) // (B // M)
    done_rows = 0
    for e_ in range(n_env):
        sl = slice(e_ * pop_env * P, (e_ + 1) * pop_env * P)
        trace = {}
        ref = po.rollout(om, actions[e_ * pop_env:(e_ + 1) * pop_env], s0s[e_], P, members=members[:, sl], eps=eps[:, sl], trace=trace)
        nobs = torch.stack(trace["next_obs"])
        done_rows += int(torch.stack(trace["dones"]).sum())
        skip = (box_margin(nobs) < 1e-4).any(0).view(pop_env, P).any(1)
        assert int(skip.sum()) <= 2
        assert_returns_close_nan_aware(out[e_ * pop_env:(e_ + 1) * pop_env], ref, skip)
    assert 0 < done_rows < H * B


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_reduced_precision_has_no_instance_for_a_term_table(engine):
    """The parametric forms run on the generic and hidden-static instances; bf16 arithmetic exists in shape-specialised ones only."""
    obs, act = 17, 6
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=200, seed=3)
    engine.set_model(dataclasses.replace(to_spec(om, obs, act, precision="bf16"), reward=halfcheetah_terms(act)))
    with pytest.raises(hipets.HipetsError, match="precision bf16:"):
        engine.rollout(torch.zeros(480, 3, act, device=DEV), np.zeros(obs, np.float32), 20, mode="device")
    engine.set_model(dataclasses.replace(to_spec(om, obs, act), reward=halfcheetah_terms(act)))  # fp32: the hidden-static instance, not the lean one
    assert engine.kernel_class(480, 20, 30, "device")[0] == "hidden_static"
    engine.set_model(to_spec(om, obs, act))
    assert engine.kernel_class(480, 20, 30, "device")[0] == "fused"


def test_set_model_names_the_entry_it_refuses(engine, monkeypatch):
    """hipets_set_model validates the tables itself (a C client has no Python layer in front of it): HIPETS_ERR_INVALID_ARGUMENT with
    the offending entry named.  The Python-side checks are switched off for the purpose."""
    om = po.make_synthetic_model(OBS, ACT, ensemble_size=5, hid=40, seed=3)
    base = to_spec(om, OBS, ACT)
    monkeypatch.setattr(RewardTerms, "validate", lambda self, *a, **k: None)
    monkeypatch.setattr(BoxTermination, "validate", lambda self, *a, **k: None)
    monkeypatch.setattr(hipets.ModelSpec, "validate", lambda self: None)
    ok_box = BoxTermination([I(0, -1.0, 1.0)])
    cases = [
        (dict(reward=RewardTerms([T("linear", 0)] * 65)), "n_reward_terms 65"),
        (dict(termination=BoxTermination([I(0)] * 65)), "n_term_intervals 65"),
        (dict(reward=RewardTerms([T("linear", 0), T("linear", OBS)])), f"reward term 1: dim i = {OBS}"),
        (dict(reward=RewardTerms([T("linear", 0, j=OBS)])), f"reward term 0: dim j = {OBS}"),
        (dict(reward=RewardTerms([T("square", ACT, source="act")])), f"reward term 0: dim i = {ACT}"),
        (dict(termination=BoxTermination([I(0), I(1), I(OBS, 0.0, 1.0)])), f"term interval 2: dim {OBS}"),
        (dict(termination=BoxTermination([I(0), I(1, 2.0, 1.0)])), "term interval 1: lo 2"),
        (dict(reward=RewardTerms([], alive_bonus=1.0, termination_fn=ok_box)), "alive_bonus 1 needs a termination_fn other than NONE"),
    ]
    for kw, msg in cases:
        with pytest.raises(hipets.HipetsError, match=msg) as exc:
            engine.set_model(dataclasses.replace(base, **kw))
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT, msg
    # unknown fn / source codes and tables without their enum: straight through the binding
    from hipets import _lib
    monkeypatch.setitem(_lib.TERM_FN, "cube", 9)
    monkeypatch.setitem(_lib.TERM_SRC, "state", 5)
    for kw, msg in [(dict(reward=RewardTerms([T("cube", 0)])), "reward term 0: unknown fn 9"),
                    (dict(reward=RewardTerms([T("linear", 0), T("linear", 0, source="state")])), "reward term 1: unknown source 5")]:
        with pytest.raises(hipets.HipetsError, match=msg) as exc:
            engine.set_model(dataclasses.replace(base, **kw))
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT
    monkeypatch.setitem(_lib.REW, "terms", _lib.REW["halfcheetah"])  # a table next to an enum that does not ask for it
    with pytest.raises(hipets.HipetsError, match="reward_fn 4 is not HIPETS_REW_TERMS") as exc:
        engine.set_model(dataclasses.replace(base, reward=RewardTerms([T("linear", 0)])))
    assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT
    monkeypatch.setitem(_lib.TERM, "box", _lib.TERM["hopper"])
    with pytest.raises(hipets.HipetsError, match="termination_fn 3 is not HIPETS_TERM_BOX"):
        engine.set_model(dataclasses.replace(base, termination=ok_box))
    monkeypatch.undo()
    engine.set_model(dataclasses.replace(base, reward=REWARD, termination=BOX))  # and the engine still takes a good model
    assert engine.rollout(torch.zeros(40, 2, ACT, device=DEV), np.zeros(OBS, np.float32), 5, mode="device").shape == (40,)
