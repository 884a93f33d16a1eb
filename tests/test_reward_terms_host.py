"""The parametric closed forms (hipets.RewardTerms, hipets.BoxTermination; include/hipets.h HIPETS_REW_TERMS / HIPETS_TERM_BOX)
on the host, no GPU: the torch callables restate the closed forms mbrl.env ships (against the oracle, which is bitwise the
reference), ModelSpec.validate and the classes refuse what the kernels cannot take, spec_from_model_env recognises the
instances, and the ctypes binding has the header's version and struct sizes.  (What hipets_set_model itself refuses needs an
engine: tests/test_gpu_reward_terms.py.)"""
import ctypes
import dataclasses
import math
import os
import re

import pytest
import torch

import hipets
from conftest import ROOT
from hipets import BoxTermination, RewardTerms, UnsupportedModelError
from hipets import Interval as I
from hipets import RewardTerm as T
from hipets import _lib
from oracle import pets_oracle as po

B = 4000
T1 = dict(rtol=1e-5, atol=2e-6)
THR = 12 * 2 * math.pi / 360


def halfcheetah_terms(act_dim=6):
    """reward_fns.halfcheetah (:33-38): s0 - 0.1 sum a^2 (the 0.0 * s2^2 term adds an exact zero on finite rows)"""
    return RewardTerms([T("linear", 0)] + [T("square", i, w=-0.1, source="act") for i in range(act_dim)])


def pusher_terms():
    """reward_fns.pusher (:41-53): -(0.5 |tip - obj|_1 + 1.25 |goal - obj|_1 + 0.1 sum a^2)"""
    goal = (0.45, -0.05, -0.323)
    return RewardTerms([T("abs", 14 + k, w=-0.5, j=17 + k) for k in range(3)] + [T("abs", 17 + k, w=-1.25, c=goal[k]) for k in range(3)]
                       + [T("square", i, w=-0.1, source="act") for i in range(7)])


def cartpole_box():
    return BoxTermination([I(0, -2.4, 2.4, lo_open=True, hi_open=True), I(2, -THR, THR, lo_open=True, hi_open=True)])


def hopper_box(obs_dim=11):
    return BoxTermination([I(0, 0.7, math.inf, lo_open=True), I(1, -0.2, 0.2, lo_open=True, hi_open=True)]
                          + [I(d, -100.0, 100.0, lo_open=True, hi_open=True) for d in range(1, obs_dim)], require_finite=True)


BOXES = {
    "cartpole": (4, cartpole_box(), {}),
    "walker2d": (8, BoxTermination([I(0, 0.8, 2.0, True, True), I(1, -1.0, 1.0, True, True)]), {0: (1.0, 1.4)}),
    "ant": (6, BoxTermination([I(0, 0.2, 1.0)], require_finite=True), {0: (0.3, 0.6)}),
    "inverted_pendulum": (5, BoxTermination([I(1, -0.2, 0.2)], require_finite=True), {1: (0.15, 0.0)}),
    "hopper": (11, hopper_box(), {0: (1.0, 1.0), 1: (0.15, 0.0)}),
}


def rows(obs, act, scale=None, seed=0):
    """B random rows; dims listed in ``scale`` {dim: (std, mean)} sit around the thresholds; row 5 holds a NaN, row 9 an inf,
    row 20 a value beyond hopper's 100"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, obs, generator=g) * 1.5
    for d, (std, mean) in (scale or {}).items():
        s[:, d] = s[:, d] / 1.5 * std + mean
    a = torch.rand(B, act, generator=g) * 2 - 1
    s[5, 0] = float("nan")
    s[9, 1] = float("inf")
    s[20, obs - 1] = 150.0
    return a, s


def assert_t1_nan_aware(got, ref):
    assert got.shape == ref.shape == (B, 1) and got.dtype == torch.float32
    assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), "non-finite values in different rows"
    fin = torch.isfinite(ref)
    print(f"max |diff| {float((got[fin] - ref[fin]).abs().max()):.3e}")
    assert torch.allclose(got[fin], ref[fin], **T1)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))


def test_halfcheetah_as_a_term_table():
    a, s = rows(17, 6)
    s[9, 0] = float("inf")
    ref = po.rew_halfcheetah(a, s)
    assert torch.isnan(ref[5, 0]) and torch.isinf(ref[9, 0])
    # (the table has no 0.0 * s2^2 term: it restates the reference on rows whose s2 is finite, as all of these are)
    assert torch.isfinite(s[:, 2]).all()
    assert_t1_nan_aware(halfcheetah_terms()(a, s), ref)


def test_pusher_as_a_term_table():
    a, s = rows(20, 7)
    s[9, 18] = float("inf")
    ref = po.rew_pusher(a, s)
    assert torch.isnan(ref[9, 0]) or torch.isinf(ref[9, 0])
    assert_t1_nan_aware(pusher_terms()(a, s), ref)


def test_cartpole_reward_is_an_alive_bonus_over_the_cartpole_box():
    a, s = rows(4, 1)
    s[9, 2] = float("inf")
    box = cartpole_box()
    rew = RewardTerms([], alive_bonus=1.0, termination_fn=box)
    ref = po.rew_cartpole(a, s)
    assert 0 < float(ref.mean()) < 1
    assert torch.equal(rew(a, s), ref)  # 0 / 1 exactly
    assert float(rew(a, s)[5]) == 0.0  # a NaN row is done: no bonus


@pytest.mark.parametrize("name", sorted(BOXES))
def test_boxes_restate_the_shipped_termination_functions(name):
    obs, box, scale = BOXES[name]
    a, s = rows(obs, 2, scale)
    ref = po.TERMINATION_FNS[name](a, s)
    got = box(a, s)
    assert got.dtype == torch.bool and got.shape == (B, 1)
    assert 0.02 < float(ref.float().mean()) < 0.98, "degenerate case"
    assert torch.equal(got, ref)
    assert bool(got[5])  # the NaN row fails every test on its dim / the finite test
    # on a threshold: an open bound is done, a closed one alive
    for iv in box.intervals:
        for bound, is_open in ((iv.lo, iv.lo_open), (iv.hi, iv.hi_open)):
            if math.isfinite(bound):
                x = s[100:101].clone()
                x[0, :] = 0.0
                for other in box.intervals:  # a healthy row ...
                    x[0, other.dim] = 0.5 * (max(other.lo, -1e3) + min(other.hi, 1e3))
                x[0, iv.dim] = bound  # ... put on this bound (float32(bound), as the kernel's table holds it)
                assert bool(box(a[:1], x)[0, 0]) == is_open
                assert torch.equal(box(a[:1], x), po.TERMINATION_FNS[name](a[:1], x))


def test_humanoid_box_differs_from_the_reference_on_nan_rows_only():
    a, s = rows(9, 3, {0: (0.6, 1.5)})
    box = BoxTermination([I(0, 1.0, 2.0)])
    ref = po.term_humanoid(a, s)
    got = box(a, s)
    fin = torch.isfinite(s[:, 0])
    assert torch.equal(got[fin], ref[fin]) and 0 < float(ref.float().mean()) < 1
    assert not bool(ref[5]) and bool(got[5])  # the reference's humanoid leaves a NaN row alive; a box ends it


def test_terms_accumulate_in_table_order_in_fp32():
    """bias first, then term by term: the order is part of the definition (fp32 addition does not associate)"""
    a = torch.zeros(1, 1)
    s = torch.tensor([[1.0, 2.0 ** -24, 2.0 ** -24]])
    up = RewardTerms([T("linear", 0), T("linear", 1), T("linear", 2)])
    down = RewardTerms([T("linear", 1), T("linear", 2), T("linear", 0)])
    assert float(up(a, s)) == 1.0 and float(down(a, s)) == 1.0 + 2.0 ** -23
    assert float(RewardTerms([T("square", 0, w=2.0, c=3.0)], bias=0.5)(a, s)) == 0.5 + 2.0 * 4.0
    assert float(RewardTerms([T("abs", 0, j=1, w=-1.0, source="obs")])(a, torch.tensor([[1.0, 4.0]]))) == -3.0
    assert float(RewardTerms([T("linear", 0, source="act")])(torch.tensor([[7.0]]), s)) == 7.0
    out = RewardTerms([T("linear", 0)])(a.double(), s.double())
    assert out.dtype == torch.float32 and out.shape == (1, 1)


# ---- validation ----------------------------------------------------------------------------------------------------------
def small_spec(**kw):
    E, obs, act, hid = 3, 5, 2, 8
    d = dict(weights=[torch.zeros(E, obs + act, hid), torch.zeros(E, hid, hid), torch.zeros(E, hid, 2 * obs)],
             biases=[torch.zeros(E, 1, hid), torch.zeros(E, 1, hid), torch.zeros(E, 1, 2 * obs)],
             obs_dim=obs, act_dim=act, min_logvar=-10 * torch.ones(1, obs), max_logvar=0.5 * torch.ones(1, obs))
    d.update(kw)
    return hipets.ModelSpec(**d)


def test_a_spec_with_the_parametric_forms_validates():
    box = BoxTermination([I(0, -1.0, 1.0), I(4, 0.0, math.inf, lo_open=True)], require_finite=True)
    rew = RewardTerms([T("linear", 4), T("square", 1, source="act", w=-0.1), T("abs", 0, j=3)], bias=0.25, alive_bonus=0.5, termination_fn=box)
    small_spec(reward=rew, termination=box).validate()
    small_spec(reward=rew, termination=BoxTermination([I(0, -1.0, 1.0), I(4, 0.0, math.inf, lo_open=True)], require_finite=True)).validate()  # an EQUAL box
    small_spec(reward=dataclasses.replace(rew, alive_bonus=0.0, termination_fn=None), termination="hopper").validate()  # a table over an enum termination
    small_spec(reward="halfcheetah", termination=box).validate()  # a box under an enum reward
    small_spec(reward=RewardTerms([T("linear", 0)] * 64), termination=BoxTermination([I(0)] * 64)).validate()  # the limits themselves
    assert rew == dataclasses.replace(rew) and hash(rew) == hash(dataclasses.replace(rew))


@pytest.mark.parametrize("make,match", [
    (lambda: RewardTerms([T("linear", 0)] * 65), "at most 64"),
    (lambda: BoxTermination([I(0)] * 65), "at most 64"),
    (lambda: RewardTerms([T("cube", 0)]), "term 0: fn 'cube'"),
    (lambda: RewardTerms([T("linear", 0), T("linear", 0, source="state")]), "term 1: source 'state'"),
    (lambda: RewardTerms([T("linear", -1)]), "term 0: dim i = -1"),
    (lambda: BoxTermination([I(0), I(1, 2.0, 1.0)]), "interval 1: lo 2.0 is not <= hi 1.0"),
    (lambda: BoxTermination([I(0, float("nan"), 1.0)]), "interval 0: lo nan"),
    (lambda: BoxTermination([I(-2)]), "interval 0: dim -2"),
    (lambda: RewardTerms([], alive_bonus=1.0), "alive_bonus != 0 needs termination_fn"),
    (lambda: RewardTerms([], alive_bonus=1.0, termination_fn=po.term_cartpole), "alive_bonus != 0 needs termination_fn"),
])
def test_the_classes_refuse_what_no_kernel_can_take(make, match):
    with pytest.raises(UnsupportedModelError, match=re.escape(match)):
        make()


@pytest.mark.parametrize("kw,match", [
    (dict(reward=RewardTerms([T("linear", 4), T("linear", 5)])), "term 1: dim i = 5 outside [0, 5)"),  # obs_dim 5
    (dict(reward=RewardTerms([T("abs", 0, j=7)])), "term 0: dim j = 7 outside [0, 5)"),
    (dict(reward=RewardTerms([T("square", 2, source="act")])), "term 0: dim i = 2 outside [0, 2)"),  # act_dim 2
    (dict(termination=BoxTermination([I(0), I(5, 0.0, 1.0)])), "interval 1: dim 5 outside [0, 5)"),
    # the kernel's alive bonus uses the step's own `done`: the table's box must be the model's termination
    (dict(reward=RewardTerms([], alive_bonus=1.0, termination_fn=BoxTermination([I(0, -1.0, 1.0)])), termination=BoxTermination([I(0, -1.0, 2.0)])),
     "alive_bonus != 0 needs RewardTerms.termination_fn to equal the model's termination"),
    (dict(reward=RewardTerms([], alive_bonus=1.0, termination_fn=BoxTermination([I(0, -1.0, 1.0)])), termination="cartpole"),
     "alive_bonus != 0 needs RewardTerms.termination_fn to equal the model's termination"),
    (dict(reward=RewardTerms([], alive_bonus=1.0, termination_fn=BoxTermination([I(0, -1.0, 1.0)]))),  # no_termination
     "alive_bonus != 0 needs RewardTerms.termination_fn to equal the model's termination"),
    (dict(reward=RewardTerms([], alive_bonus=1.0, termination_fn=BoxTermination([I(7, -1.0, 1.0)])), termination=BoxTermination([I(7, -1.0, 1.0)])),
     "interval 0: dim 7 outside [0, 5)"),
])
def test_validate_checks_dims_against_the_model_and_the_alive_bonus_rule(kw, match):
    with pytest.raises(UnsupportedModelError, match=re.escape(match)):
        small_spec(**kw).validate()


# ---- spec_from_model_env ----------------------------------------------------------------------------------------------------
class _Lin:
    def __init__(self, w, b):
        self.weight, self.bias, self.use_bias = torch.nn.Parameter(w), torch.nn.Parameter(b), True


class _FakeModelEnv:
    """the attributes spec_from_model_env reads from a live mbrl.models.ModelEnv"""

    def __init__(self, reward_fn, termination_fn):
        s = small_spec()

        class Obj:
            pass

        mlp = Obj()
        mlp.hidden_layers = [[_Lin(w, b), torch.nn.SiLU()] for w, b in zip(s.weights[:-1], s.biases[:-1])]
        mlp.mean_and_logvar = _Lin(s.weights[-1], s.biases[-1])
        mlp.min_logvar, mlp.max_logvar = s.min_logvar, s.max_logvar
        mlp.elite_models, mlp.propagation_method, mlp.deterministic = None, "random_model", False
        dm = Obj()
        dm.model, dm.input_normalizer, dm.obs_process_fn = mlp, None, None
        dm.target_is_delta, dm.no_delta_list, dm.learned_rewards = True, [], False
        self.dynamics_model = dm
        self.reward_fn, self.termination_fn = reward_fn, termination_fn
        self.observation_space, self.action_space = Obj(), Obj()
        self.observation_space.shape, self.action_space.shape = (5,), (2,)


def test_spec_from_model_env_recognises_the_instances():
    box = BoxTermination([I(0, -1.0, 1.0)], require_finite=True)
    rew = RewardTerms([T("linear", 4), T("square", 1, source="act", w=-0.1)], alive_bonus=1.0, termination_fn=box)
    spec = hipets.spec_from_model_env(_FakeModelEnv(rew, box))
    assert spec.reward is rew and spec.termination is box
    assert spec.custom_reward_fn is None and spec.custom_termination_fn is None
    no_term = lambda a, o: torch.zeros(len(o), 1, dtype=torch.bool)  # noqa: E731
    no_term.hipets_closed_form = "no_termination"
    spec = hipets.spec_from_model_env(_FakeModelEnv(dataclasses.replace(rew, alive_bonus=0.0), no_term))  # a table over an enum termination
    assert isinstance(spec.reward, RewardTerms) and spec.termination == "no_termination"
    # ... and still validates what it recognised
    with pytest.raises(UnsupportedModelError, match=re.escape("dim i = 9 outside [0, 5)")):
        hipets.spec_from_model_env(_FakeModelEnv(RewardTerms([T("linear", 9)]), box))


def test_a_plain_callable_keeps_its_error_and_learns_about_the_classes():
    def my_reward(act, next_obs):
        return next_obs[:, :1]

    box = BoxTermination([I(0, -1.0, 1.0)])
    with pytest.raises(UnsupportedModelError, match="reward_fn") as exc:
        hipets.spec_from_model_env(_FakeModelEnv(my_reward, box))
    assert "my_reward" in str(exc.value) and "closed forms" in str(exc.value) and "hipets.RewardTerms" in str(exc.value)
    with pytest.raises(UnsupportedModelError, match="termination_fn") as exc:
        hipets.spec_from_model_env(_FakeModelEnv(RewardTerms([T("linear", 0)]), lambda a, o: o[:, :1] > 0))
    assert "hipets.BoxTermination" in str(exc.value)
    spec = hipets.spec_from_model_env(_FakeModelEnv(my_reward, box), allow_custom_fns=True)  # the unfused path, as before
    assert spec.reward == "none" and spec.custom_reward_fn is my_reward and spec.termination is box


# ---- binding ---------------------------------------------------------------------------------------------------------------
def test_abi_version_and_the_two_new_structs():
    assert _lib.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    assert re.search(r"#define HIPETS_ABI_VERSION 9\b", header)
    assert ctypes.sizeof(_lib.RewardTermC) == 24 and ctypes.sizeof(_lib.TermIntervalC) == 16

    def fields(struct_name):
        body = re.search(r"typedef struct \{([^{}]*)\} " + struct_name + ";", header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.findall(r"([a-z_0-9]+)\s*$", decl.strip())[0] for decl in body.split(";") if decl.strip()]

    assert fields("hipets_reward_term") == [f[0] for f in _lib.RewardTermC._fields_]
    assert fields("hipets_term_interval") == [f[0] for f in _lib.TermIntervalC._fields_]
    tail = ["reward_terms", "term_intervals", "n_reward_terms", "n_term_intervals", "reward_bias", "alive_bonus", "term_require_finite"]
    assert [f[0] for f in _lib.ModelDesc._fields_][-7:] == tail and fields("hipets_model_desc")[-7:] == tail
    for name, table in (("HIPETS_REW_TERMS", _lib.REW["terms"]), ("HIPETS_TERM_BOX", _lib.TERM["box"]),
                        ("HIPETS_MAX_REWARD_TERMS", _lib.MAX_REWARD_TERMS), ("HIPETS_MAX_TERM_INTERVALS", _lib.MAX_TERM_INTERVALS),
                        ("HIPETS_BOX_LO_OPEN", _lib.BOX_LO_OPEN), ("HIPETS_BOX_HI_OPEN", _lib.BOX_HI_OPEN),
                        ("HIPETS_TERM_FN_ABS", _lib.TERM_FN["abs"]), ("HIPETS_TERM_SRC_ACT", _lib.TERM_SRC["act"])):
        assert int(re.search(name + r"\s*=?\s*(\d+)", header).group(1)) == table, name
    # a zeroed descriptor tail means "no tables": what a client compiled against the fields but not using them passes
    d = _lib.ModelDesc()
    assert not d.reward_terms and not d.term_intervals and d.n_reward_terms == 0 and d.alive_bonus == 0.0 and d.term_require_finite == 0
