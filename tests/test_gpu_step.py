"""hipets_step -- one model transition for B independent rows (ModelEnv.step, mbrl/models/model_env.py:87-140) -- against the
oracle at the shapes the library ships, and the three callers of that path: Engine.step, hipets.ModelEnv.reset / step (MBPO's model
rollouts) and UnfusedTrajectoryEvalFn (the fallback for Python reward / termination callables, row a14).

Every in-kernel draw is replayed through the oracle with what the engine exports for the same (seed, stream): device_perms +
fast_normals (DEVICE), fast_schedule dealt 16 r rows per workgroup + fast_normals (FAST), injected perm / eps (EXACT).  One
transition is held to T1 (rtol 1e-5, atol 2e-6), done flags must be equal away from the termination thresholds
(test_gpu_closed_forms.threshold_margin), returns of the unfused objective to T2."""
import numpy as np
import pytest
import torch

import hipets
from conftest import to_spec
from oracle import feistel_perm as fp
from oracle import pets_oracle as po
from test_gpu_closed_forms import threshold_margin
from test_gpu_device_mode import SHIPPED_DEVICE_INSTANCES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T1 = dict(rtol=1e-5, atol=2e-6)
ELITE = [0, 2, 3, 5, 6]  # 7 members / 5 elites (conf/dynamics_model/gaussian_mlp_ensemble.yaml), not a prefix of the members
M = len(ELITE)
# 385 rows per member domain (24 full row tiles + 1 row), 25 tiles per domain; FAST: one domain of 1925 rows, 121 tiles.  Neither
# tile count is a multiple of 2, 3 or 4: every forced R ends on a ragged workgroup
B_RAGGED = 1925
# start-state offsets that put the rows next to the thresholds of the termination function (a mix of ended / alive rows)
NEAR = {"humanoid": {0: 1.05}, "hopper": {0: 0.76, 1: 0.0}, "cartpole": {0: 2.3}, "inverted_pendulum": {1: 0.16}}


def shipped_model(obs, act, mkw, seed=0, **extra):
    return po.make_synthetic_model(obs, act, ensemble_size=7, elite=ELITE, hid=200, seed=seed, **{**mkw, **extra})


def batch(om, obs, act, B, seed=0):
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(B, obs, generator=g) * 0.1
    for d, v in NEAR.get(om.termination, {}).items():
        x[:, d] += v
    a = torch.rand(B, act, generator=g) * 2 - 1
    return x, a


def fast_map(engine, B, seed, sid, rows_per_group=0):
    """Per-row member slots of a FAST step with (seed, sid): workgroup w owns rows [16 r w, 16 r (w + 1)) (hipets_step)."""
    nwg, r = engine.fast_geometry(B, 1, 1, rows_per_group or -1)
    return engine.fast_schedule(1, nwg, seed, sid).cpu()[0].long()[torch.arange(B) // (16 * r)]


def run_step(engine, om, x, a, mode, seed=7, sid=3, sample=True, R=0, generic=False, perm_sid=0):
    """(GPU step, oracle kwargs for po.step): the step's draws as the engine exports them."""
    B = x.shape[0]
    kw = dict(rows_per_group=R, generic_kernel=generic, sample=sample)
    if mode == "exact":
        g = torch.Generator().manual_seed(sid)
        perm = None if om.propagation == "expectation" else torch.randperm(B, generator=g)
        eps = torch.randn(B, om.out_size, generator=g) if sample else None
        got = engine.step(x.to(DEV), a.to(DEV), mode="exact", perm=None if perm is None else perm.to(DEV),
                          eps=None if eps is None else eps.to(DEV), **kw)
        return got, dict(perm=perm, eps=eps, sample=sample)
    eps = engine.fast_normals(1, B, seed, sid).cpu()[0]
    if mode == "device":
        got = engine.step(x.to(DEV), a.to(DEV), mode="device", seed=seed, stream_id=sid, perm_stream_id=perm_sid, **kw)
        perm = None
        if om.propagation != "expectation":
            perm = engine.device_perms(1, B, seed, perm_sid or sid).cpu()
            perm = perm if perm.ndim == 1 else perm[0]
        return got, dict(perm=perm, eps=eps, sample=sample)
    got = engine.step(x.to(DEV), a.to(DEV), mode="fast", seed=seed, stream_id=sid, **kw)
    members = None if om.propagation == "expectation" else fast_map(engine, B, seed, sid, R)
    return got, dict(member_of_row=members, eps=eps, sample=sample)


def assert_step_close(om, got, ref, rows=None):
    nobs, rew, done = (t.cpu() for t in got)
    if rows is not None:
        nobs, rew, done = nobs[rows], rew[rows], done[rows]
    r_nobs, r_rew, r_done = ref
    assert torch.isfinite(nobs).all() and torch.isfinite(rew).all()
    assert torch.allclose(nobs, r_nobs, **T1), f"next_obs: max err {(nobs - r_nobs).abs().max():.3e}"
    assert torch.allclose(rew, r_rew, **T1), f"rewards: max err {(rew - r_rew).abs().max():.3e}"
    near = threshold_margin(om.termination, r_nobs) < 1e-4  # the comparison is discontinuous there
    assert int(near.sum()) <= max(2, len(near) // 500)
    assert torch.equal(done[~near], r_done[~near])


# ---------------------------------------------------------------------------------------------------------------------------
# A.1  every shipped instance shape in step form, against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _wide(name):
    return name == "humanoid_v4_wide"


def _step_rs(name, Rs):
    """Row-tile counts a step of the shape can run: the default plus every R it ships.  A step never takes the WIDE layout, and in the
    general layout two row tiles of Humanoid-v4's 752-wide output rows do not fit LDS (test_wide_model_step_runs_the_general_layout)."""
    return (0,) + tuple(R for R in Rs if not (_wide(name) and R > 1))


STEP_CASES = [(name, obs, act, mkw, R, mode, "random_model", True)
              for name, obs, act, mkw, Rs in SHIPPED_DEVICE_INSTANCES for R in _step_rs(name, Rs) for mode in ("exact", "device", "fast")]
_CFG2 = SHIPPED_DEVICE_INSTANCES[1]
assert _CFG2[0] == "cfg2_halfcheetah"
STEP_CASES += [(*_CFG2[:4], 0, mode, prop, True) for prop in ("fixed_model", "expectation") for mode in ("exact", "device", "fast")]
STEP_CASES += [(*_CFG2[:4], R, mode, "random_model", False) for R in (0, 3) for mode in ("exact", "device", "fast")]
STEP_IDS = [f"{c[0]}_R{c[4]}_{c[5]}_{c[6][:5]}{'' if c[7] else '_mean'}" for c in STEP_CASES]


def test_ragged_batch_geometry():
    for R in (2, 3, 4):
        assert (-(-(B_RAGGED // M) // 16)) % R and (-(-B_RAGGED // 16)) % R
    assert (B_RAGGED // M) % 16 and B_RAGGED % 16 and B_RAGGED % M == 0


@pytest.mark.parametrize("name,obs,act,mkw,R,mode,prop,sample", STEP_CASES, ids=STEP_IDS)
def test_step_of_every_shipped_instance_matches_oracle(engine, name, obs, act, mkw, R, mode, prop, sample):
    om = shipped_model(obs, act, mkw, seed=1, propagation=prop)
    engine.set_model(to_spec(om, obs, act))
    x, a = batch(om, obs, act, B_RAGGED)
    # TS-infinity in DEVICE mode: the map comes from the reset's stream (perm_stream_id), the eps from the step's own
    got, kw = run_step(engine, om, x, a, mode, R=R, sample=sample, perm_sid=11 if prop == "fixed_model" else 0)
    assert_step_close(om, got, po.step(om, x, a, **kw))


def _expected_instance(engine, name, mode, sample, prop, B, R):
    """(kernel class, row tiles) the step runs by default: shape-specialised where the call draws in-kernel and an instance exists for
    the step's R (hipets_kernel_class answers for the step-synchronous geometry of one step), else the hidden-static instance -- except
    on the wide model, whose step runs the general layout: neither its WIDE instances nor the hidden-static one (an output row wider
    than the hidden ones) apply, it runs the generic instance."""
    if _wide(name):
        return "generic", 1
    if mode == "exact" or not sample or prop == "expectation":
        return "hidden_static", R or None
    return engine.kernel_class(B, 1, 1, mode, rows_per_group=R)


@pytest.mark.parametrize("name,obs,act,mkw,R,mode,prop,sample", STEP_CASES, ids=STEP_IDS)
def test_step_default_instance_equals_generic_kernel_bitwise(engine, name, obs, act, mkw, R, mode, prop, sample):
    """The step-form twin of test_gpu_rollout.test_hidden_static_instances_equal_the_generic_kernel_bitwise: the default instance
    of every case above against the fully generic one (generic_kernel=True) and the hidden-static one (=2).  Same bits, except where
    the default is a one-tile FUSED instance (its k-split sums hidden columns 192..207 in another order: a tenth of T1)."""
    om = shipped_model(obs, act, mkw, seed=1, propagation=prop)
    engine.set_model(to_spec(om, obs, act))
    x, a = batch(om, obs, act, B_RAGGED)
    perm_sid = 11 if prop == "fixed_model" else 0
    default, _ = run_step(engine, om, x, a, mode, R=R, sample=sample, perm_sid=perm_sid)
    generic, _ = run_step(engine, om, x, a, mode, R=R, sample=sample, perm_sid=perm_sid, generic=True)
    hstatic, _ = run_step(engine, om, x, a, mode, R=R, sample=sample, perm_sid=perm_sid, generic=2)
    for g_, h_ in zip(generic, hstatic):
        assert torch.equal(g_, h_)
    cls, r = _expected_instance(engine, name, mode, sample, prop, B_RAGGED, R)
    if R and mode != "exact" and sample and prop == "random_model" and not _wide(name):
        assert (cls, r) == ("fused", R)  # every shipped (shape, R) has its step-form instance
    for d_, g_ in zip(default, generic):
        assert torch.isfinite(d_.float()).all()
        if cls == "fused" and r == 1 and d_.dtype != torch.bool:
            assert torch.allclose(d_, g_, rtol=1e-6, atol=2e-7)
        else:
            assert torch.equal(d_, g_)


def test_wide_model_step_runs_the_general_layout(engine):
    """Humanoid-v4 (obs 376, 752 outputs): a step runs the general layout with one row tile per workgroup (its WIDE instances are a
    rollout layout); two row tiles of that layout need more than the 160 KB of LDS and are refused with a message."""
    name, obs, act, mkw, Rs = SHIPPED_DEVICE_INSTANCES[-1]
    assert _wide(name) and 2 in Rs
    om = shipped_model(obs, act, mkw)
    engine.set_model(to_spec(om, obs, act))
    x, a = batch(om, obs, act, 160)
    with pytest.raises(hipets.HipetsError, match="does not fit LDS"):
        engine.step(x.to(DEV), a.to(DEV), mode="device", seed=1, stream_id=1, rows_per_group=2)
    got, kw = run_step(engine, om, x, a, "device", R=1)
    assert_step_close(om, got, po.step(om, x, a, **kw))


# ---------------------------------------------------------------------------------------------------------------------------
# A.3  batch edges
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_B = [(B, 0) for B in (5, 75, 80, 85, 165)] + [(16 * M * R + d, R) for R in (1, 2, 3, 4) for d in (-5, 5)]


@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
@pytest.mark.parametrize("B,R", EDGE_B, ids=[f"B{b}_R{r}" for b, r in EDGE_B])
def test_step_batch_edges_gaussian_mlp(engine, B, R, mode):
    """One row per member (B = 5), a member domain of 15 / 16 / 17 rows, 33 rows per domain, and 16 M R +- 5 rows: the last workgroup of
    every domain one tile short of / five rows into the next of R tiles."""
    obs, act, mkw = _CFG2[1:4]
    om = shipped_model(obs, act, mkw, seed=2)
    engine.set_model(to_spec(om, obs, act))
    x, a = batch(om, obs, act, B, seed=B)
    got, kw = run_step(engine, om, x, a, mode, R=R, sid=B)
    assert_step_close(om, got, po.step(om, x, a, **kw))


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("B", [1, 15, 16, 17])
def test_step_batch_edges_basic_ensemble(engine, B, mode):
    """BasicEnsemble (iid members, no batch rule, basic_ensemble.py:142-196): a single row, one tile minus / exactly / plus one row."""
    obs, act = 17, 6
    om = po.make_synthetic_model(obs, act, ensemble_size=M, hid=200, seed=3, ensemble_kind="basic_ensemble")
    engine.set_model(to_spec(om, obs, act))
    x, a = batch(om, obs, act, B, seed=B)
    if mode == "exact":
        g = torch.Generator().manual_seed(B)
        members, eps = torch.randint(M, (B,), generator=g), torch.randn(B, obs, generator=g)
        got = engine.step(x.to(DEV), a.to(DEV), mode="exact", members=members, eps=eps.to(DEV))
        kw = dict(member_of_row=members, eps=eps)
    else:
        got, kw = run_step(engine, om, x, a, "fast", sid=B)
    assert_step_close(om, got, po.step(om, x, a, **kw))


@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
def test_step_batch_not_a_multiple_of_the_members_is_refused(engine, mode):
    """gaussian_mlp.py:195-200, raised for every propagation method: in every mode of Engine.step, and by ModelEnv.reset."""
    obs, act, mkw = _CFG2[1:4]
    om = shipped_model(obs, act, mkw)
    spec = to_spec(om, obs, act)
    engine.set_model(spec)
    x, a = batch(om, obs, act, 84)
    text = "GaussianMLP ensemble requires batch size to be a multiple of the number of models. Current batch size is 84 for 5 models."
    kw = dict(perm=torch.randperm(84).to(DEV), eps=torch.zeros(84, obs, device=DEV)) if mode == "exact" else {}
    with pytest.raises(hipets.HipetsError) as err:
        engine.step(x.to(DEV), a.to(DEV), mode=mode, **kw)
    assert str(err.value) == text
    env = hipets.ModelEnv(spec, engine=engine, mode=mode)
    with pytest.raises(ValueError) as err:
        env.reset(x.numpy())
    assert str(err.value) == text


# ---------------------------------------------------------------------------------------------------------------------------
# A.4  the benched shape: bench.py's model_env_step workload
# ---------------------------------------------------------------------------------------------------------------------------
B_BENCH = 100_000


def _workgroup_rows(first, per_wg, n_wg, span):
    """every row of the first, a middle and the last workgroup of a run of `span` rows starting at `first`"""
    out = []
    for w in (0, n_wg // 2, n_wg - 1):
        lo = first + w * per_wg
        out.append(torch.arange(lo, min(lo + per_wg, first + span)))
    return torch.cat(out)


@pytest.mark.parametrize("mode", ["device", "fast"])
def test_step_at_the_benched_shape(engine, mode):
    """100 000 rows, obs 17 / act 6, hid 200, 7 members / 5 elites, sample=True.  All outputs finite; a row depends only on itself, so
    the oracle replays a subset of >= 4 096 rows -- every row of the first, a middle and the last workgroup of each member domain
    (DEVICE) or of the grid (FAST), plus random rows -- with the member of each row taken from the full permutation / schedule."""
    obs, act = 17, 6
    om = po.make_synthetic_model(obs, act, ensemble_size=7, elite=[0, 1, 2, 3, 4], hid=200, seed=4)
    engine.set_model(to_spec(om, obs, act))
    x, a = batch(om, obs, act, B_BENCH, seed=4)
    seed, sid = 1, 6
    got = engine.step(x.to(DEV), a.to(DEV), mode=mode, sample=True, seed=seed, stream_id=sid)
    for t in got:
        assert torch.isfinite(t.float()).all()
    if mode == "device":
        perm = engine.device_perms(1, B_BENCH, seed, sid).cpu()[0]
        rpd = B_BENCH // M
        _, R = engine.kernel_class(B_BENCH, 1, 1, "device")
        n_wg = -(-rpd // (16 * R))
        slots = torch.cat([_workgroup_rows(d * rpd, 16 * R, n_wg, rpd) for d in range(M)])
        picked = perm[slots]
        member = torch.empty(B_BENCH, dtype=torch.long)
        member[perm] = torch.arange(B_BENCH) // rpd  # slot j -> member j // (B / M) (gaussian_mlp.py:164-166)
    else:
        nwg, R = engine.fast_geometry(B_BENCH, 1, 1, -1)
        picked = _workgroup_rows(0, 16 * R, nwg, B_BENCH)
        member = fast_map(engine, B_BENCH, seed, sid)
    g = torch.Generator().manual_seed(0)
    extra = torch.randperm(B_BENCH, generator=g)[:max(0, 4096 - len(picked)) + 512]
    rows = torch.unique(torch.cat([picked, extra]))
    assert len(rows) >= 4096
    eps = engine.fast_normals(1, B_BENCH, seed, sid).cpu()[0]
    ref = po.step(om, x[rows], a[rows], member_of_row=member[rows], eps=eps[rows], sample=True)
    assert_step_close(om, got, ref, rows=rows)


@pytest.mark.parametrize("prop,step", [("random_model", 0), ("fixed_model", 0xFFFFFFFF)])
def test_exported_permutation_at_the_benched_batch_is_the_cpu_restatement(engine, prop, step):
    """hipets_device_perms at B = 100 000 == oracle/feistel_perm.py, for the per-step key (random_model, step 0) and the TS-infinity
    key (fixed_model, step 0xFFFFFFFF)."""
    om = po.make_synthetic_model(17, 6, ensemble_size=7, elite=[0, 1, 2, 3, 4], hid=200, seed=4, propagation=prop)
    engine.set_model(to_spec(om, 17, 6))
    got = engine.device_perms(1, B_BENCH, 1, 6).cpu()
    got = got if got.ndim == 1 else got[0]
    assert np.array_equal(got.numpy(), fp.permutation(B_BENCH, 1, 6, step))


# ---------------------------------------------------------------------------------------------------------------------------
# B  hipets.ModelEnv: the member map travels in the model state
# ---------------------------------------------------------------------------------------------------------------------------
ENV_B = 165  # 33 rows per member domain; FAST: 11 row tiles


def env_model(kind, prop, seed=5):
    return po.make_synthetic_model(17, 6, ensemble_size=M, hid=200, seed=seed, propagation=prop, ensemble_kind=kind)


def env_obs(B=ENV_B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 17, generator=g) * 0.2).numpy(), [torch.rand(B, 6, generator=g) * 2 - 1 for _ in range(5)]


def oracle_map(om, idx):
    """po.step kwargs for a map as ModelEnv exports it: a permutation (GaussianMLP) or member slots (BasicEnsemble / FAST)"""
    idx = idx.cpu()
    return dict(perm=idx) if om.ensemble_kind == "gaussian_mlp" and len(torch.unique(idx)) == len(idx) else dict(member_of_row=idx)


ENV_CASES = [("gaussian_mlp", "device"), ("gaussian_mlp", "exact"), ("basic_ensemble", "fast"), ("basic_ensemble", "exact")]


@pytest.mark.parametrize("prop", ["fixed_model", "random_model"])
@pytest.mark.parametrize("kind,mode", ENV_CASES, ids=[f"{k[:5]}_{m}" for k, m in ENV_CASES])
def test_model_env_reset_and_five_steps_replayed(engine, kind, mode, prop):
    """reset + five steps, each replayed through the oracle from the GPU's previous state: the reset's map (TS-infinity: the member of
    every row is the same at every step while the eps change) or the step's own draw (TS1)."""
    om = env_model(kind, prop)
    env = hipets.ModelEnv(to_spec(om, 17, 6), engine=engine, mode=mode, seed=13)
    replay = torch.Generator().manual_seed(13)  # what EXACT mode draws from its own generator, in the same order
    obs0, acts = env_obs()
    torch.manual_seed(21)
    state = env.reset(obs0, return_as_np=False)
    B, fixed, basic = ENV_B, prop == "fixed_model", kind == "basic_ensemble"
    idx = state["propagation_indices"]
    if fixed:
        assert idx is not None and tuple(idx.shape) == (B,) and idx.dtype == torch.int64
        if mode == "device":
            assert torch.equal(idx.cpu(), engine.device_perms(1, B, 13, 1).cpu())  # the first reset keys stream 1
        if mode == "fast":
            assert torch.equal(idx.cpu(), fast_map(engine, B, 13, 1))
        if mode == "exact" and basic:
            assert torch.equal(idx.cpu(), torch.randint(M, (B,), generator=replay))
    else:
        assert idx is None
    x = torch.from_numpy(obs0.astype(np.float32))
    prev_eps = None
    for t, a in enumerate(acts, start=1):
        rng = torch.get_rng_state()
        nobs, rew, done, state = env.step(a.to(DEV), state, sample=True)
        assert state["propagation_indices"] is idx
        if mode == "exact":
            if fixed:
                kw = oracle_map(om, idx)
            elif basic:
                kw = dict(member_of_row=torch.randint(M, (B,), generator=replay))
            else:  # gaussian_mlp.py:205: the global generator
                after = torch.get_rng_state()
                torch.set_rng_state(rng)
                kw = dict(perm=torch.randperm(B))
                assert torch.equal(torch.get_rng_state(), after)
            eps = torch.empty(B, 17).normal_(0.0, 1.0, generator=replay)
        else:
            eps = engine.fast_normals(1, B, 13, t).cpu()[0]
            if fixed:
                kw = oracle_map(om, idx)
            elif mode == "device":
                kw = dict(perm=engine.device_perms(1, B, 13, t).cpu()[0])
            else:
                kw = dict(member_of_row=fast_map(engine, B, 13, t))
        assert prev_eps is None or not torch.equal(eps, prev_eps)
        assert_step_close(om, (nobs, rew, done), po.step(om, x, a, eps=eps, sample=True, **kw))
        x, prev_eps = nobs.cpu(), eps


@pytest.mark.parametrize("kind,mode", [("gaussian_mlp", "device"), ("basic_ensemble", "fast")])
def test_model_env_interleaved_states_keep_their_own_maps(engine, kind, mode):
    """reset A, reset B, step A, step B, step A: every state steps with the map its own reset drew; two resets of the same batch size
    draw different maps (the reference draws a fresh randperm / randint at every reset)."""
    om = env_model(kind, "fixed_model")
    env = hipets.ModelEnv(to_spec(om, 17, 6), engine=engine, mode=mode, seed=17)
    obs_a, acts = env_obs(seed=1)
    obs_b, _ = env_obs(seed=2)
    sa = env.reset(obs_a, return_as_np=False)
    sb = env.reset(obs_b, return_as_np=False)
    ia, ib = sa["propagation_indices"], sb["propagation_indices"]
    assert ia is not None and ib is not None
    ia, ib = ia.cpu(), ib.cpu()
    assert not torch.equal(ia, ib)
    xs = {"a": torch.from_numpy(obs_a.astype(np.float32)), "b": torch.from_numpy(obs_b.astype(np.float32))}
    states, maps = {"a": sa, "b": sb}, {"a": ia, "b": ib}
    for t, who in enumerate("aba", start=1):
        nobs, rew, done, states[who] = env.step(acts[t].to(DEV), states[who], sample=True)
        ref = po.step(om, xs[who], acts[t], eps=engine.fast_normals(1, ENV_B, 17, t).cpu()[0], sample=True, **oracle_map(om, maps[who]))
        assert_step_close(om, (nobs, rew, done), ref)
        xs[who] = nobs.cpu()


@pytest.mark.parametrize("kind,mode", ENV_CASES, ids=[f"{k[:5]}_{m}" for k, m in ENV_CASES])
def test_model_env_fixed_model_step_without_indices_raises(engine, kind, mode):
    """gaussian_mlp.py:207-211, basic_ensemble.py:182-186: a TS-infinity step needs the map of a reset."""
    om = env_model(kind, "fixed_model")
    env = hipets.ModelEnv(to_spec(om, 17, 6), engine=engine, mode=mode, seed=3)
    obs0, acts = env_obs()
    obs = torch.from_numpy(obs0.astype(np.float32)).to(DEV)
    for state in ({"obs": obs}, {"obs": obs, "propagation_indices": None}):
        with pytest.raises(Exception) as err:
            env.step(acts[0].to(DEV), state, sample=True)
        assert err.type is ValueError and str(err.value) == "When using propagation='fixed_model', `propagation_indices` must be provided."


@pytest.mark.parametrize("kind,mode", ENV_CASES, ids=[f"{k[:5]}_{m}" for k, m in ENV_CASES])
def test_model_env_honours_caller_supplied_indices(engine, kind, mode):
    """A ``propagation_indices`` tensor the caller put into the state (torch.randperm(B) for a GaussianMLP, torch.randint(M, (B,)) for
    a BasicEnsemble) is the map the step uses; the eps still come from the step's own stream.  A copy of the reset's own map steps like
    the map itself (the in-kernel path and the explicit one agree to T1)."""
    om = env_model(kind, "fixed_model")
    env = hipets.ModelEnv(to_spec(om, 17, 6), engine=engine, mode=mode, seed=19)
    obs0, acts = env_obs(seed=3)
    state = env.reset(obs0, return_as_np=False)
    assert state["propagation_indices"] is not None
    g = torch.Generator().manual_seed(4)
    mine = torch.randint(M, (ENV_B,), generator=g) if kind == "basic_ensemble" else torch.randperm(ENV_B, generator=g)
    x = torch.from_numpy(obs0.astype(np.float32))
    replay = torch.Generator().manual_seed(19)
    if mode == "exact" and kind == "basic_ensemble":
        torch.randint(M, (ENV_B,), generator=replay)  # the reset's draw
    for t, idx in enumerate((mine.to(DEV), state["propagation_indices"].clone()), start=1):
        nobs, rew, done, nxt = env.step(acts[t].to(DEV), {**state, "propagation_indices": idx}, sample=True)
        assert nxt["propagation_indices"] is idx
        if mode == "exact":
            eps = torch.empty(ENV_B, 17).normal_(0.0, 1.0, generator=replay)
        else:
            eps = engine.fast_normals(1, ENV_B, 19, t).cpu()[0]
        assert_step_close(om, (nobs, rew, done), po.step(om, x, acts[t], eps=eps, sample=True, **oracle_map(om, idx)))
    if mode != "exact":  # the reset's own map through the in-kernel path: the same transition as its copy above (step stream 3)
        keyed = env.step(acts[2].to(DEV), state, sample=True)[:3]
        eps = engine.fast_normals(1, ENV_B, 19, 3).cpu()[0]
        assert_step_close(om, keyed, po.step(om, x, acts[2], eps=eps, sample=True, **oracle_map(om, state["propagation_indices"])))


@pytest.mark.parametrize("kind,mode", [("gaussian_mlp", "device"), ("basic_ensemble", "fast")])
def test_model_env_reset_exports_its_own_models_map_on_a_shared_engine(engine, kind, mode):
    """Engines are shared per GPU.  Env X (random_model) steps, then env Y (fixed_model, same member count and hidden width) resets
    and steps: Y's ``propagation_indices`` is a [B] map of Y's own model and the map Y's step uses."""
    ox, oy = env_model(kind, "random_model", seed=6), env_model(kind, "fixed_model", seed=7)
    ex = hipets.ModelEnv(to_spec(ox, 17, 6), engine=engine, mode=mode, seed=23)
    ey = hipets.ModelEnv(to_spec(oy, 17, 6), engine=engine, mode=mode, seed=29)
    obs0, acts = env_obs(seed=5)
    ex.step(acts[0].to(DEV), ex.reset(obs0, return_as_np=False), sample=True)
    state = ey.reset(obs0, return_as_np=False)
    idx = state["propagation_indices"]
    assert idx is not None and tuple(idx.shape) == (ENV_B,)
    nobs, rew, done, _ = ey.step(acts[1].to(DEV), state, sample=True)
    eps = engine.fast_normals(1, ENV_B, 29, 1).cpu()[0]
    x = torch.from_numpy(obs0.astype(np.float32))
    assert_step_close(oy, (nobs, rew, done), po.step(oy, x, acts[1], eps=eps, sample=True, **oracle_map(oy, idx)))
    want = engine.device_perms(1, ENV_B, 29, 1).cpu() if mode == "device" else fast_map(engine, ENV_B, 29, 1)
    assert torch.equal(idx.cpu(), want)


def test_model_env_return_as_np_round_trips(engine):
    """return_as_np=True (the reference's default) hands out numpy copies of what return_as_np=False returns, and the state it hands
    back steps on unchanged."""
    om = env_model("gaussian_mlp", "fixed_model")
    spec = to_spec(om, 17, 6)
    envs = [hipets.ModelEnv(spec, engine=engine, seed=31) for _ in range(2)]
    obs0, acts = env_obs(seed=6)
    s_np, s_t = envs[0].reset(obs0), envs[1].reset(obs0, return_as_np=False)
    assert torch.equal(s_np["propagation_indices"], s_t["propagation_indices"])
    for a in acts[:3]:
        out_np = envs[0].step(a.numpy(), s_np, sample=True)
        out_t = envs[1].step(a.to(DEV), s_t, sample=True)
        assert isinstance(out_np[0], np.ndarray) and out_np[2].dtype == bool and out_np[1].shape == (ENV_B, 1)
        for n_, t_ in zip(out_np[:3], out_t[:3]):
            assert np.array_equal(n_, t_.cpu().numpy())
        assert out_np[3]["propagation_indices"] is s_np["propagation_indices"]
        s_np, s_t = out_np[3], out_t[3]


# ---------------------------------------------------------------------------------------------------------------------------
# C  UnfusedTrajectoryEvalFn replayed through the oracle
# ---------------------------------------------------------------------------------------------------------------------------
UNFUSED = [  # name, obs, act, model kwargs, pop, P, H, step_mode
    ("hid200_device_random", 17, 6, dict(ensemble_size=7, elite=ELITE, hid=200), 100, 20, 5, "device"),
    ("hid200_device_fixed", 17, 6, dict(ensemble_size=7, elite=ELITE, hid=200, propagation="fixed_model"), 100, 20, 5, "device"),
    ("hid200_basic_fast_fixed", 17, 6, dict(ensemble_size=M, hid=200, propagation="fixed_model", ensemble_kind="basic_ensemble"), 100, 20, 5, "fast"),
    ("small_hopper_device", 11, 3, dict(ensemble_size=M, hid=40, termination="hopper"), 24, 5, 6, "device"),
    ("small_hopper_basic_fast_fixed", 11, 3, dict(ensemble_size=M, hid=40, termination="hopper", propagation="fixed_model",
                                                  ensemble_kind="basic_ensemble"), 24, 5, 6, "fast"),
]


@pytest.mark.parametrize("name,obs,act,mkw,pop,P,H,step_mode", UNFUSED, ids=[c[0] for c in UNFUSED])
def test_unfused_eval_fn_replayed_through_oracle(engine, name, obs, act, mkw, pop, P, H, step_mode):
    """The horizon loop of ModelEnv.evaluate_action_sequences on the host, one hipets_step per step, the reward / termination of the
    oracle's own closed forms as Python callables on the device tensors: returns == po.rollout (T2) fed the per-step exports of the
    eval fn's streams -- calls * 4096 + 1 + t (DEVICE; TS-infinity map: calls * 4096 + 1), calls * 4096 + t (FAST) -- on two
    consecutive calls."""
    om = po.make_synthetic_model(obs, act, seed=8, **mkw)
    s0 = (np.random.default_rng(2).standard_normal(obs) * 0.05).astype(np.float32)
    if om.termination == "hopper":  # smaller, less noisy steps from just above the height threshold: rows end at every step
        om.weights[-1] = om.weights[-1] * 0.2
        om.max_logvar = torch.full_like(om.max_logvar, -5.0)
        s0[0], s0[1] = 0.8, 0.0
    seed = 37
    rew_fn = po.REWARD_FNS[om.reward] if om.reward is not None else None
    fn = hipets.UnfusedTrajectoryEvalFn(to_spec(om, obs, act), P, reward_fn=rew_fn, termination_fn=po.TERMINATION_FNS[om.termination],
                                        engine=engine, seed=seed, step_mode=step_mode)
    B = pop * P
    fixed = om.propagation == "fixed_model"
    g = torch.Generator().manual_seed(9)
    for call in (1, 2):
        actions = torch.rand(pop, H, act, generator=g) * 2 - 1
        out = fn(s0, actions.to(DEV))
        assert fn.calls == call
        if step_mode == "device":
            sids = [call * 4096 + 1 + t for t in range(H)]
            perms = engine.device_perms(1, B, seed, sids[0]).cpu() if fixed else torch.stack([engine.device_perms(1, B, seed, s).cpu()[0] for s in sids])
            kw = dict(perms=perms)
        else:
            sids = [call * 4096 + t for t in range(H)]
            kw = dict(members=torch.stack([fast_map(engine, B, seed, sids[0] if fixed else s) for s in sids]))
        eps = torch.stack([engine.fast_normals(1, B, seed, s).cpu()[0] for s in sids])
        trace = {}
        ref = po.rollout(om, actions, s0, P, eps=eps, trace=trace, **kw)
        ended = torch.stack(trace["dones"])[..., 0].cummax(0).values  # [H, B]: the row has terminated by step t
        if om.termination != "no_termination":  # the termination function fires mid-horizon, not all at once
            assert 0 < int(ended[0].sum()) < int(ended[H // 2].sum()) < int(ended[-1].sum()) < B
        near = threshold_margin(om.termination, torch.stack(trace["next_obs"])) < 1e-4  # (a discontinuity of the return)
        keep = ~near.any(0).view(pop, P).any(1)
        assert int((~keep).sum()) <= 2
        out = out.cpu()
        assert torch.isfinite(out).all()
        err = (out - ref).abs()[keep]
        assert (err <= 1e-4 * torch.clamp(ref[keep].abs(), min=1.0)).all(), f"max err {err.max():.3e}"  # T2
