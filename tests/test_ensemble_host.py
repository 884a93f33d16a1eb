"""Host checks of hipets.ensemble (no GPU): the restatements of tests/ensemble_restatement.py against the reference's own classes
(tests/golden/ensemble_predict_cases.npz, recorded by tests/make_ensemble_golden.py), the penalty's restatement on hand-computed rows,
UncertaintyPenalty's validation, the new symbols, the shape rule, and the near-agreement case's claim about the variance rule."""
import os
import re

import numpy as np
import pytest
import torch

import ensemble_restatement as er
import hipets
from conftest import ROOT
from hipets import _lib
from hipets._pack import check_ensemble_shape, ensemble_lds_bytes

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ensemble_predict_cases.npz"))


def golden_case(key, **kw):
    n = sum(1 for k in GOLDEN.files if re.fullmatch(key + r"_w\d+", k))
    ws, bs = [GOLDEN[f"{key}_w{i}"] for i in range(n)], [GOLDEN[f"{key}_b{i}"] for i in range(n)]
    det = f"{key}_min_logvar" not in GOLDEN.files
    case = dict(E=ws[0].shape[0], weights=ws, biases=bs, deterministic=det, out_dim=ws[-1].shape[2] // (1 if det else 2), slope=0.01,
                normalizer="none", columns=None, elites=None)
    if not det:
        case.update(min_logvar=GOLDEN[f"{key}_min_logvar"], max_logvar=GOLDEN[f"{key}_max_logvar"])
    case.update(kw)
    return case


GMLP = dict(activation="silu", normalizer="f64", columns=[(int(d), ("id", "sin", "cos")[int(f)]) for d, f in GOLDEN["gmlp_columns"]],
            elites=[int(i) for i in GOLDEN["gmlp_elites"]])


def _close(got, want, what):
    share = er.t1_share(got, want).max()
    print(f"{what}: max share of T1 {share:.3g}, bit-equal {np.array_equal(np.asarray(got, np.float32), np.asarray(want, np.float32))}")
    assert share <= 1.0, (what, share)


@pytest.mark.parametrize("key,kw,elite", [("gmlp", GMLP, False), ("gmlp", GMLP, True), ("det", dict(activation="relu"), False),
                                          ("basic", dict(activation="tanh"), False)], ids=["gmlp", "gmlp_elite", "det", "basic"])
def test_restatements_equal_the_reference_forward(key, kw, elite):
    case = golden_case(key, **kw)
    x = GOLDEN[f"{key}_model_in"]
    pre = f"{key}_elite_" if elite else f"{key}_"
    for fn, name in ((er.ensemble_f32_torch, "f32"), (er.ensemble_f64, "f64")):
        mean, logvar, stats = fn(case, x, only_elite=elite)
        _close(mean, GOLDEN[pre + "mean"], f"{key} {name} mean")
        if case["deterministic"]:
            assert logvar is None and (stats[:, 0] == 0).all() and np.array_equal(stats[:, 2], stats[:, 1])
        else:
            _close(logvar, GOLDEN[pre + "logvar"], f"{key} {name} logvar")
        assert stats.shape == (len(x), 4) and np.isfinite(stats).all() and (stats[:, 3] > 0).all()
    # the two restatements' statistics agree with each other (float32 against float64)
    _close(er.ensemble_f32_torch(case, x, elite)[2], er.ensemble_f64(case, x, elite)[2], f"{key} stats")


def test_model_input_equals_the_reference():
    case = golden_case("gmlp", **GMLP)
    case.update(norm_mean=GOLDEN["gmlp_norm_mean"], norm_std=GOLDEN["gmlp_norm_std"])
    x = er.model_input(case, GOLDEN["gmlp_obs"], GOLDEN["gmlp_act"])
    assert x.dtype == np.float32
    _close(x, GOLDEN["gmlp_model_in"], "model input")
    _close(er.model_input(case, GOLDEN["gmlp_obs"], GOLDEN["gmlp_act"], f64=True), GOLDEN["gmlp_model_in"], "model input f64")


def test_penalty_restatement_on_hand_computed_rows():
    f = np.float32
    stats = np.zeros((4, 4), f)
    stats[:, 2] = [0.5, 2.0, np.nan, 1.0]
    rewards, dones = np.array([1.0, 1.0, 1.0, -3.0], f), np.array([0, 0, 0, 1], np.uint8)
    r, d = er.penalty_np(stats, 2, 2.0, rewards, dones)  # no halt
    assert np.array_equal(r[[0, 1, 3]], np.array([0.0, -3.0, -5.0], f)) and np.isnan(r[2]) and np.array_equal(d, dones)
    r, d = er.penalty_np(stats, 2, 2.0, rewards, dones, halt_threshold=0.75)  # halt: rows above the threshold are done; NaN never halts
    assert np.array_equal(d, [0, 1, 0, 1]) and np.array_equal(r[[0, 1, 3]], np.array([0.0, -3.0, -5.0], f)) and np.isnan(r[2])
    r, d = er.penalty_np(stats, 2, 2.0, rewards, dones, halt_threshold=0.75, halt_reward=-100.0)
    assert np.array_equal(d, [0, 1, 0, 1]) and np.array_equal(r[[0, 1, 3]], np.array([0.0, -100.0, -100.0], f)) and np.isnan(r[2])
    r, d = er.penalty_np(stats[[0, 1, 3]], 2, 0.0, rewards[[0, 1, 3]], dones[[0, 1, 3]], halt_threshold=1.0)  # coef 0: rewards keep their bits
    assert np.array_equal(r.view(np.uint32), rewards[[0, 1, 3]].view(np.uint32)) and np.array_equal(d, [0, 1, 1])
    r, _ = er.penalty_np(stats, 0, 3.0, rewards, dones)  # another column: all zeros there
    assert np.array_equal(r, rewards)
    assert r.dtype == np.float32 and d.dtype == np.uint8


def test_uncertainty_penalty_validation():
    p = hipets.UncertaintyPenalty("max_std", coef=1)
    assert (p.kind, p.coef, p.halt_threshold, p.halt_reward, p.only_elite, p.stat) == ("max_std", 1.0, None, None, True, 0)
    assert [hipets.UncertaintyPenalty(k).stat for k in er.STATS] == [0, 1, 2, 3] and _lib.ENSEMBLE_STATS == er.STATS
    assert hipets.UncertaintyPenalty("disagreement", 0.5, halt_threshold=2, halt_reward=-10).halt_reward == -10.0
    assert hash(hipets.UncertaintyPenalty("total_std", 2.0)) == hash(hipets.UncertaintyPenalty("total_std", 2.0))
    for bad in (dict(kind="std"), dict(coef=float("nan")), dict(coef=float("inf")), dict(coef="1"), dict(coef=None), dict(coef=True),
                dict(halt_threshold=float("nan")), dict(halt_reward=-1.0), dict(halt_threshold=1.0, halt_reward=float("nan"))):
        with pytest.raises(ValueError):
            hipets.UncertaintyPenalty(**bad)


def test_new_symbols_are_declared_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    for name in ("hipets_ensemble_set", "hipets_ensemble_predict", "hipets_ensemble_geometry", "hipets_uncertainty_penalty"):
        assert re.search(r"^int " + name + r"\(", header, flags=re.M), name
        assert name in _lib.SYMBOLS
    assert "#define HIPETS_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9
    assert [n for n, _ in _lib.SYMBOLS["hipets_ensemble_predict"][1]] == ["e", "obs", "actions", "model_in", "batch", "only_elite", "mean", "logvar",
                                                                          "stats", "stream"]


def _spec(E=3, obs=4, act=2, hid=16, layers=3, **kw):
    out = obs
    dims = [obs + act] + [hid] * (layers - 1) + [2 * out]
    return hipets.ModelSpec(weights=[torch.zeros(E, dims[i], dims[i + 1]) for i in range(layers)],
                            biases=[torch.zeros(E, 1, dims[i + 1]) for i in range(layers)], obs_dim=obs, act_dim=act,
                            min_logvar=torch.zeros(1, out), max_logvar=torch.ones(1, out), reward="none", **kw)


def test_shape_rule_as_a_function():
    check_ensemble_shape(_spec())
    # the stock 23-200x4-36 shape fits four row tiles, Humanoid's one (LDS opt-in limit 160 KiB)
    assert ensemble_lds_bytes(23, 200, 18, False, 5, row_tiles=4) == 4 * 64 * (36 + 212 + 212 + 36) <= 160 * 1024
    assert ensemble_lds_bytes(393, 200, 377, False, 5) == 64 * (404 + 212 + 772 + 754) <= 160 * 1024 < ensemble_lds_bytes(393, 200, 377, False, 5, 2)
    check_ensemble_shape(_spec(obs=376, act=17, hid=200, layers=5))
    for kw, word in ((dict(precision="bf16"), "bf16"), (dict(precision="bf16x3"), "bf16x3"), (dict(E=17), "ensemble_size"),
                     (dict(obs=510, act=3), "in_dim"), (dict(hid=1025), "hidden"), (dict(obs=500, act=2, hid=1024), "LDS")):
        with pytest.raises(hipets.UnsupportedModelError, match=word):
            check_ensemble_shape(_spec(**kw))
    with pytest.raises(hipets.UnsupportedModelError, match="out_dim"):  # (a wide output alone: obs 513 would trip in_dim first)
        s = _spec(obs=400, act=2)
        s.weights[-1] = torch.zeros(3, 16, 2 * 513)
        check_ensemble_shape(s)


@pytest.mark.parametrize("kw", [dict(precision="bf16"), dict(precision="bf16x3"), dict(E=17), dict(obs=500, act=2, hid=1024)],
                         ids=["bf16", "bf16x3", "seventeen_members", "lds"])
def test_predictor_refuses_at_construction_without_a_device(kw):
    class NoEngine:  # (nothing of it may be touched)
        def __getattr__(self, name):
            raise AssertionError(f"the engine's {name} was used")

    with pytest.raises(hipets.UnsupportedModelError):
        hipets.EnsemblePredictor(_spec(**kw), engine=NoEngine())
    with pytest.raises(hipets.UnsupportedModelError):
        hipets.EnsemblePredictor(_spec(**kw))  # (no engine given: none is made either)


def test_variance_about_the_first_member_survives_near_agreement():
    """members that agree to 1e-2 around a mean shifted by 5: the shifted-sum float32 statistic stays inside T1, the one-pass
    E[x^2] - E[x]^2 of the raw means misses by hundreds of T1 (thousands at shift 30)"""
    for shift, least in ((5.0, 100.0), (30.0, 1000.0)):
        case = er.make_case("near_agree", near=(1e-2, shift))
        x = er.model_input(case, case["obs"], case["act"], f64=True)
        mean64, _, stats64 = er.ensemble_f64(case, x)
        mean32 = er.ensemble_f32_torch(case, x.astype(np.float32))[0]
        shifted = er.t1_share(er.shifted_disagreement_f32(mean32), stats64[:, 1]).max()
        naive = er.t1_share(er.naive_disagreement_f32(mean32), stats64[:, 1]).max()
        print(f"shift {shift}: shifted sums use {shifted:.3g} of T1, the naive form {naive:.4g}")
        assert shifted < 1.0 and naive > least
