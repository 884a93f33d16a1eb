"""hipets_ensemble_predict / hipets_uncertainty_penalty on the GPU against tests/ensemble_restatement.py.

Parity: per element within T1 x max(1, 4 u) of the float64 restatement, u the largest share of T1 that the float32 torch restatement
itself uses against float64 on the same case (computed here on the CPU) -- for the means, the log-variances and each statistic
separately.  The cases and what each is for: ensemble_restatement.GPU_CASES; building one asserts that exchanging members 0 and 1 in any
single layer moves member 0's mean by more than T1 on every row, so parity refuses a kernel that reads the wrong member or layer.
The other checks compare bits: a row's outputs across batch sizes (hence row tiles) and requested outputs, a NaN row's neighbours, the
penalty against its numpy restatement, the model_in route against the raw route, hipets_step before and after a snapshot."""
import functools

import numpy as np
import pytest
import torch

import ensemble_restatement as er
import hipets
from hipets._pack import pack_model_desc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, {only_elite: (float64 outputs, bound factors)}) -- computed once per case and shared"""
    case = er.make_case(name)
    x64 = er.model_input(case, case["obs"], case["act"], f64=True)
    x32 = er.model_input(case, case["obs"], case["act"])
    refs = {}
    for elite in ((False, True) if case["elites"] is not None else (False,)):
        m64, l64, s64 = er.ensemble_f64(case, x64, elite)
        m32, l32, s32 = er.ensemble_f32_torch(case, x32, elite)
        factors = dict(mean=er.bound_factor(m32, m64), logvar=1.0 if l64 is None else er.bound_factor(l32, l64),
                       stats=[er.bound_factor(s32[:, k], s64[:, k]) for k in range(4)])
        refs[elite] = ((m64, l64, s64), factors)
    return case, refs


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(got, want, factor, what):
    share = er.t1_share(got.cpu().numpy(), want)
    print(f"{what}: largest share of T1 {share.max():.3f}, bound factor {factor:.2f}")
    assert share.max() <= factor, (what, float(share.max()), factor)


def batches_of(name, predictor, rows):
    if name != "small_silu":
        return [rows]
    r = predictor.geometry(rows)[0]  # row tiles of a full launch: the ragged last workgroup on both sides of its edge
    return [1, 16 * r - 1, 16 * r + 1]


@pytest.mark.parametrize("name", [n for n in er.GPU_CASES])
def test_parity_with_the_float64_restatement(engine, name):
    case, refs = reference(name)
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    obs, act = dev(case["obs"]), dev(case["act"])
    for elite, ((m64, l64, s64), f) in refs.items():
        for B in batches_of(name, predictor, len(case["obs"])):
            mean, logvar = predictor.predict(obs[:B], act[:B], only_elite=elite)
            stats = predictor.uncertainty(obs[:B], act[:B], only_elite=elite)
            tag = f"{name} elite={elite} B={B}"
            assert mean.shape == m64[:, :B].shape and stats.shape == (B, 4)
            check(mean, m64[:, :B], f["mean"], tag + " mean")
            if case["deterministic"]:
                assert logvar is None
                s = stats.cpu().numpy()
                assert (s[:, 0] == 0).all() and np.array_equal(s[:, 2], s[:, 1])
            else:
                check(logvar, l64[:, :B], f["logvar"], tag + " logvar")
            for k, stat in enumerate(er.STATS):
                check(stats[:, k], s64[:B, k], f["stats"][k], f"{tag} {stat}")


def test_deterministic_model_has_no_logvar_head(engine):
    case, _ = reference("det_relu")
    hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    with pytest.raises(ValueError, match="log-variance"):
        engine.ensemble_predict(dev(case["obs"]), dev(case["act"]), logvar=True)
    lv = torch.empty(4, len(case["obs"]), case["out_dim"], device=DEV)
    with pytest.raises(hipets.HipetsError, match="log-variance"):  # the library's own refusal
        engine._call("hipets_ensemble_predict", obs=dev(case["obs"]), actions=dev(case["act"]), model_in=None, batch=len(case["obs"]), only_elite=0,
                     mean=None, logvar=lv, stats=None)


def test_argument_refusals(engine):
    case, _ = reference("exact16")
    hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    obs, act = dev(case["obs"]), dev(case["act"])
    x = dev(er.model_input(case, case["obs"], case["act"]))
    out = torch.empty(len(obs), 4, device=DEV)
    call = lambda **kw: engine._call("hipets_ensemble_predict", **{**dict(obs=obs, actions=act, model_in=None, batch=len(obs), only_elite=0, mean=None,  # noqa: E731
                                                                          logvar=None, stats=out), **kw})
    call()
    for kw, word in ((dict(model_in=x), "either"), (dict(actions=None), "either"), (dict(batch=0), "batch"), (dict(stats=None), "no output")):
        with pytest.raises(hipets.HipetsError, match=word) as exc:
            call(**kw)
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT


def test_model_in_route(engine):
    """a ready model input gives the raw route's bits when it holds the kernel's own input (identity columns, float32 normaliser: one
    correctly rounded subtraction and division per element, the same in numpy), and stays inside the bound otherwise (sin / cos)"""
    case, _ = reference("columns_id")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    raw = predictor.predict(case["obs"], case["act"]) + (predictor.uncertainty(case["obs"], case["act"], only_elite=False),)
    x = er.model_input(case, case["obs"], case["act"])
    ready = engine.ensemble_predict(model_in=dev(x), stats=True)
    for a, b in zip(raw, ready):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    case, refs = reference("columns_f32")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    (m64, l64, _), f = refs[False]
    mean, logvar = predictor.forward(er.model_input(case, case["obs"], case["act"]))
    check(mean, m64, f["mean"], "columns_f32 model_in mean")
    check(logvar, l64, f["logvar"], "columns_f32 model_in logvar")


def test_geometry(engine):
    case, _ = reference("humanoid_fit")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    r, lds = predictor.geometry(40)
    assert r == 1 and lds == hipets._pack.ensemble_lds_bytes(393, 200, 377, False, 5) <= 160 * 1024
    case, _ = reference("stock")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    assert [predictor.geometry(b)[0] for b in (1, 16, 17, 32, 33, 100000)] == [1, 1, 2, 2, 4, 4]  # the largest R the rule allows
    assert predictor.geometry(1000)[1] == hipets._pack.ensemble_lds_bytes(23, 200, 18, False, 5, 4)


def test_rows_do_not_depend_on_batch_row_tiles_or_requested_outputs(engine):
    case, _ = reference("stock")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    obs, act = dev(case["obs"]), dev(case["act"])
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    full = engine.ensemble_predict(obs, act, only_elite=True, stats=True)
    for B in (1, 17, 100):  # one, two and four row tiles per workgroup
        assert predictor.geometry(B)[0] == {1: 1, 17: 2, 100: 4}[B]
        part = engine.ensemble_predict(obs[:B], act[:B], only_elite=True, stats=True)
        assert torch.equal(bits(part[0]), bits(full[0][:, :B])) and torch.equal(bits(part[1]), bits(full[1][:, :B]))
        assert torch.equal(bits(part[2]), bits(full[2][:B]))
    tail = engine.ensemble_predict(obs[990:].contiguous(), act[990:].contiguous(), only_elite=True, stats=True)  # another place in the batch
    assert torch.equal(bits(tail[0]), bits(full[0][:, 990:])) and torch.equal(bits(tail[2]), bits(full[2][990:]))
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        some = engine.ensemble_predict(obs, act, only_elite=True, mean=want[0], logvar=want[1], stats=want[2])
        for got, ref, asked in zip(some, full, want):
            assert (got is None) == (not asked) and (got is None or torch.equal(bits(got), bits(ref)))


def test_a_nan_row_stays_in_its_row(engine):
    case, _ = reference("small_silu")
    hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    obs, act = dev(case["obs"]), dev(case["act"])
    clean = engine.ensemble_predict(obs, act, stats=True)
    bad = obs.clone()
    bad[5, 1] = float("nan")
    bad[37] = float("inf")
    dirty = engine.ensemble_predict(bad, act, stats=True)
    keep = torch.ones(len(obs), dtype=torch.bool, device=DEV)
    keep[[5, 37]] = False
    for c, d in zip(clean, dirty):
        rows = (lambda t: t[:, keep]) if c.ndim == 3 else (lambda t: t[keep])
        assert torch.equal(rows(c).view(torch.int32), rows(d).view(torch.int32))
    assert torch.isnan(dirty[0][:, 5]).all() and torch.isnan(dirty[2][5, 1:]).all()


def test_penalty_equals_its_restatement_bit_for_bit(engine):
    rng = np.random.default_rng(7)
    B = 1000
    stats = rng.gamma(2.0, 1.0, (B, 4)).astype(np.float32)
    stats[3, :] = np.nan
    stats[4, 1] = np.inf
    rewards = rng.standard_normal(B).astype(np.float32)
    dones = (rng.uniform(size=B) < 0.1).astype(np.uint8)
    for stat, coef, thr, hr in ((0, 1.0, None, None), (1, 0.37, 2.0, None), (2, 2.5, 1.5, -100.0), (3, 0.0, 2.0, None), (1, -0.5, 0.0, 0.25)):
        r, d = dev(rewards), dev(dones)
        engine.uncertainty_penalty(dev(stats), stat, coef, r, d, halt_threshold=thr, halt_reward=hr)
        want_r, want_d = er.penalty_np(stats, stat, coef, rewards, dones, thr, hr)
        got_r = r.cpu().numpy()
        nan = np.isnan(want_r)  # (IEEE leaves a NaN's sign and payload open: NaN where the restatement has one, the bits elsewhere)
        assert nan.any() and np.array_equal(np.isnan(got_r), nan), (stat, coef, thr, hr)
        assert np.array_equal(got_r[~nan].view(np.uint32), want_r[~nan].view(np.uint32)), (stat, coef, thr, hr)
        assert np.array_equal(d.cpu().numpy(), want_d)
    r, flags = dev(rewards), dev(dones).bool()  # bool dones, as ModelEnv.step holds them
    engine.uncertainty_penalty(dev(stats), 0, 1.0, r, flags, halt_threshold=2.0)
    assert np.array_equal(flags.cpu().numpy(), er.penalty_np(stats, 0, 1.0, rewards, dones, 2.0)[1].astype(bool))


def test_a_refused_set_leaves_no_ensemble(engine):
    case, _ = reference("exact16")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    assert predictor.geometry(16)[0] == 1
    spec = er.case_spec(case, precision="bf16")
    ws = [w.to(DEV).contiguous() for w in spec.weights]
    bs = [b.to(DEV).contiguous() for b in spec.biases]
    d, cols, keep = pack_model_desc(spec, ws, bs)
    try:
        with pytest.raises(hipets.HipetsError, match="fp32 only") as exc:
            engine._call("hipets_ensemble_set", desc=d, cols=cols, n_cols=0)
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT
        with pytest.raises(hipets.HipetsError, match="engine has no ensemble"):
            engine._geometry("hipets_ensemble_geometry", 16)
        with pytest.raises(hipets.HipetsError, match="engine has no ensemble"):
            engine._call("hipets_ensemble_predict", obs=dev(case["obs"]), actions=dev(case["act"]), model_in=None, batch=4, only_elite=0, mean=None,
                         logvar=None, stats=torch.empty(4, 4, device=DEV))
    finally:
        engine.ensemble_spec = engine.ensemble_owner = None  # (the binding's mirror of the slot, which the raw call went around)
    assert predictor.geometry(16)[0] == 1  # the predictor finds the slot empty and takes its snapshot again


def test_a_snapshot_does_not_move_the_model_step(engine):
    case, _ = reference("small_silu")
    spec = er.case_spec(case)
    obs, act = dev(case["obs"][:48]), dev(case["act"][:48])
    engine.set_model(spec)
    before = engine.step(obs, act, mode="device", seed=3, stream_id=5)
    other, _ = reference("basic_tanh")
    hipets.EnsemblePredictor(er.case_spec(other), engine=engine).uncertainty(other["obs"], other["act"])
    after = engine.step(obs, act, mode="device", seed=3, stream_id=5)
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32), b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))


def test_predictor_follows_a_model_that_was_trained(engine, monkeypatch):
    """the snapshot rule: when the live model's version token moved, the model is read and packed again before the next launch"""
    import types

    import hipets.ensemble as he

    case, _ = reference("small_silu")
    live, state = types.SimpleNamespace(dynamics_model=None, device=DEV), {"version": 0, "spec": er.case_spec(case)}
    monkeypatch.setattr(he, "model_version", lambda model: state["version"])
    monkeypatch.setattr(he, "spec_from_model_env", lambda model, **kw: state["spec"])
    predictor = hipets.EnsemblePredictor(live, engine=engine)
    base = predictor.uncertainty(case["obs"], case["act"]).clone()
    assert torch.equal(predictor.uncertainty(case["obs"], case["act"]), base) and predictor.spec is state["spec"]
    moved = er.case_spec(case)
    moved.weights[-1] = moved.weights[-1] * 1.5
    state.update(version=1, spec=moved)
    assert not torch.equal(predictor.uncertainty(case["obs"], case["act"]), base) and predictor.spec is moved


@pytest.mark.parametrize("key", ["gmlp", "det", "basic"])
def test_forward_matches_the_reference_goldens(engine, key):
    """EnsemblePredictor.forward / predict against the reference's own float32 outputs (tests/golden/ensemble_predict_cases.npz): within
    the parity rule of the float64 restatement, and of the recorded outputs by that bound plus their own distance to float64"""
    from test_ensemble_host import GMLP, GOLDEN, golden_case

    extra = {"gmlp": dict(GMLP, obs_dim=3, act_dim=3, learned_rewards=True, basic=False, norm_mean=GOLDEN["gmlp_norm_mean"], norm_std=GOLDEN["gmlp_norm_std"]),
             "det": dict(activation="relu", obs_dim=4, act_dim=2, learned_rewards=False, basic=False),
             "basic": dict(activation="tanh", obs_dim=4, act_dim=2, learned_rewards=False, basic=True)}[key]
    case = golden_case(key, **extra)
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    x = GOLDEN[f"{key}_model_in"]
    for elite in ((False, True) if key == "gmlp" else (False,)):
        pre = f"{key}_elite_" if elite else f"{key}_"
        m64, l64, _ = er.ensemble_f64(case, x, elite)
        m32, l32, _ = er.ensemble_f32_torch(case, x, elite)
        routes = [predictor.forward(x, only_elite=elite)]
        if key == "gmlp":  # the raw route: the kernel's own obs_process and float64 normaliser
            routes.append(predictor.predict(GOLDEN["gmlp_obs"], GOLDEN["gmlp_act"], only_elite=elite))
        for mean, logvar in routes:
            for got, f64, f32, name in ((mean, m64, m32, "mean"), (logvar, l64, l32, "logvar")):
                if f64 is None:
                    assert got is None
                    continue
                factor, recorded = er.bound_factor(f32, f64), GOLDEN[pre + name]
                check(got, f64, factor, f"{key} elite={elite} {name} against float64")
                check(got, recorded, factor + float(er.t1_share(recorded, f64).max()), f"{key} elite={elite} {name} against the recorded reference")
