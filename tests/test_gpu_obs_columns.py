"""The parametric observation preprocessing -- a column table (hipets.ObsColumns, HIPETS_OBS_COLUMNS: model-input column k is
id / sin / cos of one observation dim) -- ON THE GPU, in the input build of the generic and hidden-static rollout kernels: against
the oracle evaluating the very same object (registered under a fresh name in po.OBS_PROCESS_FNS), against the enum path for the two
shipped preprocessors restated as tables (bit for bit), across input widths, launch forms and entry points, and where the library
refuses it.  Tolerances are those of tests/test_gpu_reward_terms.py / test_gpu_closed_forms.py: T1 (rtol 1e-5, atol 2e-6) for one
step, T2 (1e-4 max(1, |ref|)) for returns.  No termination function anywhere, so no candidate is excluded.  The oracle's
make_synthetic_model fixes the input width per preprocessor name, hence the small factory below (same initialisation)."""
import dataclasses

import numpy as np
import pytest
import torch

import hipets
from conftest import to_spec
from hipets import ObsColumns
from hipets.planning import _BoundObjective
from oracle import device_draws
from oracle import pets_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, ACT = 5, 2
# a table no enum covers: dim 4 unused, dim 1 three times, order permuted; 8 columns from 5 dims
TABLE = ObsColumns([(3, "cos"), (0, "id"), (1, "sin"), (1, "cos"), (2, "id"), (3, "sin"), (1, "id"), (0, "cos")])
T1 = dict(rtol=1e-5, atol=2e-6)


def cycled_table(n_cols, obs):
    """n_cols columns over `obs` dims: dims in a stride-3 walk (every dim turns up where n_cols >= obs), fns cycling cos / id / sin"""
    return ObsColumns([((3 * k + 1) % obs, ("cos", "id", "sin")[k % 3]) for k in range(n_cols)])


def make(monkeypatch, obs, act, table, hid=40, seed=0, name="columns_under_test", **kw):
    """(oracle model whose obs_process is `table` under a fresh name, its ModelSpec with the OBJECT, start state).  models/util.py:15-28
    initialisation (truncated normal, std 1 / (2 sqrt(in)), zero bias), logvar bounds -10 / 0.5, non-trivial f64 normaliser stats."""
    monkeypatch.setitem(po.OBS_PROCESS_FNS, name, table)
    E, n_in = 5, len(table.columns) + act
    g = torch.Generator().manual_seed(seed + 3)
    dims = [n_in] + [hid] * 4 + [2 * obs]
    ws, bs = [], []
    for li in range(len(dims) - 1):
        w = torch.empty(E, dims[li], dims[li + 1])
        for e in range(E):
            po.truncated_normal_(w[e], std=float(1 / (2 * np.sqrt(dims[li]))), generator=g)
        ws.append(w)
        bs.append(torch.zeros(E, 1, dims[li + 1]))
    rng = np.random.default_rng(seed + 4)
    om = po.OracleModel(weights=ws, biases=bs, min_logvar=-10 * torch.ones(1, obs), max_logvar=0.5 * torch.ones(1, obs),
                        norm_mean=torch.from_numpy(rng.normal(0, 0.1, size=(1, n_in))), norm_std=torch.from_numpy(rng.uniform(0.5, 2.0, size=(1, n_in))),
                        obs_process=name, reward="halfcheetah", termination="no_termination", **kw)
    spec = dataclasses.replace(to_spec(om, obs, act), obs_process=table)
    s0 = (np.random.default_rng(seed).standard_normal(obs) * 0.5).astype(np.float32)
    return om, spec, s0


def fast_members(engine, pop, P, H, seed, sid):
    nwg, r = engine.fast_geometry(pop, P, H, 0)
    sched = engine.fast_schedule(H, nwg, seed, sid).cpu()
    wg = device_draws.fast_row_workgroup(torch.arange(pop * P), P, r)
    return torch.stack([sched[t][wg].long() for t in range(H)])


def assert_returns_close(out, ref):
    out, ref = out.detach().cpu(), ref.detach().cpu()
    assert torch.isfinite(ref).all() and torch.isfinite(out).all()
    err, tol = (out - ref).abs(), 1e-4 * torch.clamp(ref.abs(), min=1.0)  # T2
    print(f"max |err| {float(err.max()):.3e} over {ref.numel()} returns in {float(ref.min()):.2f} .. {float(ref.max()):.2f}")
    assert (err <= tol).all(), f"max err {err.max():.3e}"
    assert float(ref.min()) < float(ref.max())


def rollout_against_oracle(engine, om, s0, act, pop, P, H, mode, seed=321, sid=4):
    B = pop * P
    g = torch.Generator().manual_seed(11)
    actions = torch.rand(pop, H, act, generator=g) * 2 - 1
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
    nobs = torch.stack(trace["next_obs"])
    print("max |next_obs|", float(nobs.abs().max()))
    assert_returns_close(out, ref)


# ---- 1. a table no enum covers, against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [40, 200])
@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
def test_rollouts_of_a_table_no_enum_covers(engine, monkeypatch, mode, hid):
    om, spec, s0 = make(monkeypatch, OBS, ACT, TABLE, hid=hid)
    engine.set_model(spec)
    pop, P, H = 20, 5, 4
    assert engine.kernel_class(pop, P, H, "fast" if mode == "fast" else "device")[0] == ("hidden_static" if hid == 200 else "generic")
    rollout_against_oracle(engine, om, s0, ACT, pop, P, H, mode)


# ---- 2. input-width edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs, act, n_cols", [(5, 2, 7), (5, 2, 14), (5, 2, 15), (5, 2, 3), (40, 6, 70)])
def test_input_width_edges(engine, monkeypatch, obs, act, n_cols):
    """in 9 (one k chunk, padding columns 9..15), 16 (exactly one chunk), 17 (a second chunk that is nearly empty; the quad of columns
    12..15 straddles the obs / action boundary at 14 and 15 columns), 5 (fewer columns than dims) and 76 (obs 40: 30 dims as sin and cos,
    10 as id); 35 rows: not a multiple of the 16-row tile"""
    if n_cols == 70:
        table = ObsColumns([(d, "sin") for d in range(30)] + [(d, "id") for d in range(30, 40)] + [(d, "cos") for d in range(30)])
    else:
        table = cycled_table(n_cols, obs)
    om, spec, s0 = make(monkeypatch, obs, act, table, seed=n_cols)
    assert spec.in_dim == n_cols + act
    engine.set_model(spec)
    rollout_against_oracle(engine, om, s0, act, 7, 5, 4, "exact")


# ---- 3. hipets_step --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, elite", [(37, [3]), (40, None)])
@pytest.mark.parametrize("mode", ["exact", "device", "fast"])
def test_single_transitions_with_nan_and_infinite_rows(engine, monkeypatch, mode, B, elite):
    """next_obs / reward T1 where the reference is finite; the three rows with a NaN, +inf or -inf in a dim that enters as sin / cos are
    non-finite in the same rows as the oracle (sin(inf) is NaN).  A GaussianMLP ensemble takes batches that are a multiple of its
    active members only (gaussian_mlp.py:195-200, which the library keeps): B = 37 runs on ONE elite member of the five, B = 40 on all."""
    om, spec, s0 = make(monkeypatch, OBS, ACT, TABLE, seed=1, elite_models=elite)
    engine.set_model(spec)
    g = torch.Generator().manual_seed(5)
    x = torch.from_numpy(s0).repeat(B, 1) + torch.randn(B, OBS, generator=g) * 0.5
    x[7, 1] = float("nan")   # dim 1: sin, cos and id columns
    x[20, 3] = float("inf")  # dim 3: cos and sin columns only
    x[33, 0] = float("-inf")  # dim 0: id and cos columns
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
    nobs, rew, _ = (t.cpu() for t in got)
    r_nobs, r_rew, _ = ref
    bad_rows = ~torch.isfinite(r_nobs).all(-1)
    assert bad_rows[7] and bad_rows[20] and bad_rows[33] and int(bad_rows.sum()) == 3
    assert torch.equal(~torch.isfinite(nobs).all(-1), bad_rows)
    assert torch.isnan(r_nobs[20]).all() and torch.isnan(nobs[20]).all()  # sin(inf) = NaN reaches every output through the hidden layers
    good = ~bad_rows
    print("max |next_obs err|", float((nobs[good] - r_nobs[good]).abs().max()))
    assert torch.allclose(nobs[good], r_nobs[good], **T1)
    assert torch.equal(torch.isfinite(rew[:, 0]), torch.isfinite(r_rew[:, 0]))
    assert torch.allclose(rew[good], r_rew[good], **T1)


# ---- 4. the shipped forms restated, against the enum path ---------------------------------------------------------------------
RESTATED = {  # obs, act, reward, the preprocessor as a table
    "halfcheetah": (18, 6, "halfcheetah", ObsColumns([(1, "id"), (2, "sin"), (2, "cos")] + [(d, "id") for d in range(3, 18)])),
    "cartpole_pets": (4, 1, "cartpole_pets", ObsColumns([(1, "sin"), (1, "cos"), (0, "id"), (2, "id"), (3, "id")])),
}


@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("name", list(RESTATED))
def test_restated_shipped_forms_equal_the_enum_path_bit_for_bit(engine, name, mode):
    """Same model, kernel instance, seed and stream: the table evaluates the sinf / cosf the enum evaluates, on the same values."""
    obs, act, reward, table = RESTATED[name]
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=40, seed=3, obs_process=name, reward=reward)
    s0 = (np.random.default_rng(0).standard_normal(obs) * 0.5).astype(np.float32)
    pop, P, H, B = 40, 5, 8, 120
    g = torch.Generator().manual_seed(11)
    actions = (torch.rand(pop, H, act, generator=g) * 2 - 1).to(DEV)
    x = (torch.from_numpy(s0).repeat(B, 1) + torch.randn(B, obs, generator=g) * 0.5).to(DEV)
    a = (torch.rand(B, act, generator=g) * 2 - 1).to(DEV)
    results = []
    for obs_process in (name, table):
        engine.set_model(dataclasses.replace(to_spec(om, obs, act), obs_process=obs_process))
        assert engine.kernel_class(pop, P, H, mode)[0] == "generic"
        results.append((engine.rollout(actions, s0, P, mode=mode, seed=321, stream_id=4).cpu(),
                        [t.cpu() for t in engine.step(x, a, mode=mode, sample=True, seed=77, stream_id=9)]))
    (ret_enum, step_enum), (ret_tab, step_tab) = results
    assert torch.isfinite(ret_enum).all() and float(ret_enum.min()) < float(ret_enum.max())
    assert torch.equal(ret_tab, ret_enum)
    assert torch.equal(step_tab[0], step_enum[0]) and torch.equal(step_tab[1], step_enum[1])


# ---- 5. launch forms ---------------------------------------------------------------------------------------------------------------
def test_persistent_device_rollout_equals_per_step_launches(engine, monkeypatch):
    """The hidden-static instance at 200 logical workgroups: one persistent launch == H per-step launches, bit for bit."""
    P, H, M, pop = 20, 4, 5, 320
    om, spec, s0 = make(monkeypatch, OBS, ACT, TABLE, hid=200)
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
    """CEMOptimizer.optimize over a model with a column table: the one-call fused plan and the per-iteration path (what a callback
    forces) return the same plan bit for bit -- the table is on the fused plans' path, not beside it."""
    H, P, pop = 10, 5, 120
    om, spec, s0 = make(monkeypatch, OBS, ACT, TABLE, hid=200)
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


# ---- 6. batched start states -------------------------------------------------------------------------------------------------------
def test_two_environments_in_one_device_launch(engine, monkeypatch):
    """n_env = 2: ONE balanced permutation per step over the rows of both environments; each environment's returns replayed
    through the oracle from its own start state."""
    om, spec, s0 = make(monkeypatch, OBS, ACT, TABLE)
    engine.set_model(spec)
    pop_env, n_env, P, H = 20, 2, 5, 4
    pop, B, M = pop_env * n_env, pop_env * n_env * P, 5
    g = torch.Generator().manual_seed(11)
    actions = torch.rand(pop, H, ACT, generator=g) * 2 - 1
    s0s = np.stack([s0, s0 + (torch.randn(OBS, generator=g) * 0.7).numpy().astype(np.float32)])
    seed, sid = 5, 9
    out = engine.rollout(actions.to(DEV), s0s, P, mode="device", seed=seed, stream_id=sid, n_env=n_env).cpu()
    eps = engine.fast_normals(H, B, seed, sid).cpu()
    perms = engine.device_perms(H, B, seed, sid).cpu()
    members = torch.empty(H, B, dtype=torch.long)  # slot j holds row perms[t][j] and runs member j // (B / M)
    for t in range(H):
        members[t][perms[t]] = torch.arange(B) // (B // M)
    for e_ in range(n_env):
        sl = slice(e_ * pop_env * P, (e_ + 1) * pop_env * P)
        ref = po.rollout(om, actions[e_ * pop_env:(e_ + 1) * pop_env], s0s[e_], P, members=members[:, sl], eps=eps[:, sl])
        assert_returns_close(out[e_ * pop_env:(e_ + 1) * pop_env], ref)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_reduced_precision_has_no_instance_for_a_column_table(engine, precision):
    """A table runs on the generic and hidden-static instances; bf16 / bf16x3 arithmetic exists in shape-specialised ones only.  The
    identity table over a shape that HAS such an instance without it."""
    obs, act = 17, 6
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=200, seed=3)
    identity = ObsColumns([(d, "id") for d in range(obs)])
    engine.set_model(dataclasses.replace(to_spec(om, obs, act, precision=precision), obs_process=identity))
    with pytest.raises(hipets.HipetsError, match=f"precision {precision}: no shape-specialised kernel instance"):
        engine.rollout(torch.zeros(480, 3, act, device=DEV), np.zeros(obs, np.float32), 20, mode="device")
    engine.set_model(dataclasses.replace(to_spec(om, obs, act), obs_process=identity))  # fp32: the hidden-static instance, not the lean one
    assert engine.kernel_class(480, 20, 30, "device")[0] == "hidden_static"
    engine.set_model(to_spec(om, obs, act))
    assert engine.kernel_class(480, 20, 30, "device")[0] == "fused"


def test_set_model_columns_names_the_entry_it_refuses(engine, monkeypatch):
    """hipets_set_model_columns validates its table itself (a C client has no Python layer in front of it): HIPETS_ERR_INVALID_ARGUMENT
    with the offending entry named.  The Python-side checks are switched off for the purpose."""
    from hipets import _lib

    om, base, _ = make(monkeypatch, OBS, ACT, TABLE)
    monkeypatch.setattr(ObsColumns, "validate", lambda self, *a, **k: None)
    monkeypatch.setattr(hipets.ModelSpec, "validate", lambda self: None)
    cols = list(TABLE.columns)

    def refused(table, msg):
        with pytest.raises(hipets.HipetsError, match=msg) as exc:
            engine.set_model(dataclasses.replace(base, obs_process=table))
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT, msg

    refused(ObsColumns([(0, "id")] * 513), r"n_cols 513 outside \[1, 512\]")
    refused(ObsColumns([]), r"n_cols 0 outside \[1, 512\]")
    refused(ObsColumns(cols[:7]), "in_dim 10 != n_cols 7 \\+ act_dim 2")
    refused(ObsColumns(cols + [(0, "id")]), "in_dim 10 != n_cols 9 \\+ act_dim 2")
    refused(ObsColumns(cols[:5] + [(OBS, "sin")] + cols[6:]), rf"obs column 5: dim {OBS} outside \[0, {OBS}\)")
    refused(ObsColumns([(-1, "id")] + cols[1:]), rf"obs column 0: dim -1 outside \[0, {OBS}\)")
    monkeypatch.setitem(_lib.COL_FN, "tan", 3)
    refused(ObsColumns(cols[:7] + [(0, "tan")]), "obs column 7: unknown fn 3")
    lib, real = engine._lib, engine._lib.hipets_set_model_columns
    monkeypatch.setattr(lib, "hipets_set_model_columns", lambda h, d, c, n, st: real(h, d, None, n, st))  # a null table
    refused(TABLE, "cols is null")
    monkeypatch.setattr(lib, "hipets_set_model_columns", lambda h, d, c, n, st: lib.hipets_set_model(h, d, st))  # the plain entry point
    refused(TABLE, "call hipets_set_model_columns")
    monkeypatch.setattr(lib, "hipets_set_model_columns", real)
    monkeypatch.setitem(_lib.OBS, "columns", _lib.OBS["halfcheetah"])  # a table next to an enum that does not ask for it
    refused(TABLE, "obs_process 1 is not HIPETS_OBS_COLUMNS")
    monkeypatch.undo()
    engine.set_model(base)  # and the engine still takes a good model
    assert engine.rollout(torch.zeros(40, 2, ACT, device=DEV), np.zeros(OBS, np.float32), 5, mode="device").shape == (40,)


# ---- 8. the drop-in path -----------------------------------------------------------------------------------------------------------
class _Lin:
    def __init__(self, w, b):
        self.weight, self.bias, self.use_bias = torch.nn.Parameter(w), torch.nn.Parameter(b), True


class _FakeMLP:
    def __init__(self, om):
        self.hidden_layers = [[_Lin(w, b), torch.nn.SiLU()] for w, b in zip(om.weights[:-1], om.biases[:-1])]
        self.mean_and_logvar = _Lin(om.weights[-1], om.biases[-1])
        self.min_logvar, self.max_logvar = om.min_logvar, om.max_logvar
        self.elite_models, self.propagation_method, self.deterministic = None, "random_model", False

    def parameters(self):
        for layer in self.hidden_layers:
            yield layer[0].weight
            yield layer[0].bias
        yield self.mean_and_logvar.weight


def _halfcheetah(act, next_obs):
    return po.rew_halfcheetah(act, next_obs)


def _no_termination(act, next_obs):
    return torch.zeros(len(next_obs), 1, dtype=torch.bool)


_halfcheetah.hipets_closed_form = "halfcheetah"  # (functions defined outside mbrl.env opt in explicitly)
_no_termination.hipets_closed_form = "no_termination"


class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n), np.ones(n)


class _FakeModelEnv:
    """what hipets reads from a live mbrl.models.ModelEnv whose OneDTransitionRewardModel was built with obs_process_fn=table"""

    def __init__(self, om, table, obs, act):
        class Obj:
            pass

        dm = Obj()
        dm.model = _FakeMLP(om)
        dm.input_normalizer = Obj()
        dm.input_normalizer.mean, dm.input_normalizer.std = om.norm_mean, om.norm_std
        dm.obs_process_fn = table
        dm.target_is_delta, dm.no_delta_list, dm.learned_rewards = True, [], False
        self.dynamics_model = dm
        self.reward_fn, self.termination_fn = _halfcheetah, _no_termination
        self.observation_space, self.action_space = _Space(obs), _Space(act)
        self.device = DEV


def test_drop_in_path_on_a_model_env_whose_model_preprocesses_with_a_table(engine, monkeypatch):
    om, _, s0 = make(monkeypatch, OBS, ACT, TABLE)
    me = _FakeModelEnv(om, TABLE, OBS, ACT)
    pop, P, H, seed = 20, 5, 4, 13
    fn = hipets.make_eval_fn(me, P, engine=engine, seed=seed)
    assert isinstance(fn, hipets.HipTrajectoryEvalFn) and fn.spec.obs_process is TABLE and fn.spec.in_dim == len(TABLE.columns) + ACT
    actions = torch.rand(pop, H, ACT, generator=torch.Generator().manual_seed(11)) * 2 - 1
    out = fn(s0, actions.to(DEV))  # the default mode: in-kernel draws of (seed, call counter)
    B = pop * P
    ref = po.rollout(om, actions, s0, P, perms=engine.device_perms(H, B, seed, fn.calls).cpu(), eps=engine.fast_normals(H, B, seed, fn.calls).cpu())
    assert_returns_close(out, ref)
    env = hipets.ModelEnv(me, engine=engine, seed=seed)
    x = np.tile(s0, (10, 1)) + np.random.default_rng(2).standard_normal((10, OBS)).astype(np.float32) * 0.3
    state = env.reset(x, return_as_np=False)
    a = torch.rand(10, ACT, generator=torch.Generator().manual_seed(3)) * 2 - 1
    nobs, rew, done, state = env.step(a, state, sample=False)
    assert nobs.shape == (10, OBS) and rew.shape == (10, 1) and not bool(done.any())
    assert torch.isfinite(nobs).all() and torch.isfinite(rew).all()
    assert torch.equal(state["obs"], nobs)
