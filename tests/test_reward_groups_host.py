"""Reward tables with grouped terms (hipets.RewardTerms: level / op / the 'group' and 'const' sources / sin, cos, exp, sqrt;
include/hipets.h HIPETS_TERM_WORD) on the host, no GPU: the torch callable restates the three shipped closed-form rewards in the
enum's op order (against the oracle, which is bitwise the reference), evaluates a custom form with every construct like a
hand-written float64 formula, propagates NaN / inf as IEEE arithmetic does, refuses ill-formed tables with the entry named, and
packs a plain (ABI v9) entry to the v9 integer codes.  (What hipets_set_model itself refuses needs an engine:
tests/test_gpu_reward_groups.py.)"""
import math
import re

import pytest
import torch

import reward_group_forms as forms
from hipets import RewardTerms, UnsupportedModelError
from hipets import RewardTerm as T
from hipets import _lib
from hipets import model as hm
from hipets.engine import pack_reward_terms
from oracle import pets_oracle as po

B = 200_000


def rows(obs, act, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, act, generator=g) * 2 - 1, torch.randn(B, obs, generator=g) * 1.5


# ---- oracle agreement -------------------------------------------------------------------------------------------------------
def test_cartpole_pets_restated_equals_the_oracle_bit_for_bit():
    a, s = rows(4, 1)
    got, ref = forms.cartpole_pets_terms()(a, s), po.rew_cartpole_pets(a, s)
    assert got.shape == ref.shape == (B, 1) and got.dtype == torch.float32
    assert 0.0 < float(ref.max()) and float(ref.min()) < 0.0  # both the exp term and the action cost show
    assert torch.equal(got, ref)


@pytest.mark.parametrize("name,obs,act", [("pusher", 20, 7), ("halfcheetah", 17, 6)])
def test_pusher_and_halfcheetah_restated_agree_with_the_oracle(name, obs, act):
    """rtol 1e-6, no absolute slack: torch sums three, six and seven addends in another order than the table, which changes the
    sum of the squared actions by up to 3.1e-7 of itself.  Pusher's addends all have one sign, so the bound is relative to the result.
    Halfcheetah's two addends, s0 and -0.1 sum a^2, cancel on some rows (the largest gap of 4.8e-7 is 4e-4 of a result of 3.8e-5
    where both addends are 0.178): there the bound is relative to the magnitudes that were added, |s0| + 0.1 sum a^2 -- the
    forward error of the one addition that follows the reordered sum."""
    a, s = rows(obs, act)
    table = forms.pusher_terms() if name == "pusher" else forms.halfcheetah_terms()
    assert len(table.terms) == (17 if name == "pusher" else 9)
    assert {t.level for t in table.terms} == ({0, 1, 2} if name == "pusher" else {0, 1})
    got, ref = table(a, s), po.REWARD_FNS[name](a, s)
    scale = ref.abs() if name == "pusher" else (s[:, :1].abs() + 0.1 * a.double().square().sum(dim=1, keepdim=True)).float()
    err = (got - ref).abs()
    print(f"{name}: max gap {float(err.max()):.2e}, max gap / scale {float((err / scale).max()):.2e}")
    assert (err <= 1e-6 * scale).all()
    if name == "pusher":
        assert torch.allclose(got, ref, rtol=1e-6, atol=0.0)


def test_halfcheetah_restated_keeps_the_zero_weight_term():
    """0.0 * s2^2 is NaN for a non-finite s2: the restated table says so too (the flat v9 table had to leave the term out)"""
    a, s = rows(17, 6)
    s[3, 2] = float("inf")
    s[4, 2] = float("nan")
    got, ref = forms.halfcheetah_terms()(a, s), po.rew_halfcheetah(a, s)
    assert torch.isnan(ref[3, 0]) and torch.isnan(ref[4, 0])
    assert torch.equal(torch.isnan(got), torch.isnan(ref))


# ---- the custom form ------------------------------------------------------------------------------------------------------------
def test_custom_form_with_every_construct_matches_a_float64_formula():
    """rtol 1e-5 of the value, plus the forward error of adding the parts up in fp32: (number of entries) * 2^-24 * (sum of the
    parts' magnitudes) -- the parts cancel, so a bound relative to the result alone has no meaning on the rows where they do."""
    table = forms.custom_terms()
    used = {(t.source, t.fn, t.op, t.level, t.j is not None) for t in table.terms}
    assert {t.level for t in table.terms} == {0, 1, 2}
    assert ("const", "linear", "div", 1, False) in used and ("obs", "cos", "mul", 1, False) in used
    assert ("group", "sqrt", "add", 0, False) in used and ("group", "exp", "add", 0, False) in used
    assert ("obs", "sin", "add", 2, True) in used and any(t.fn == "cos" and t.c != 0.0 and t.j is None for t in table.terms)
    a, s = rows(9, forms.CUSTOM_ACT)
    got = table(a, s)
    ref, mag = forms.custom_formula_f64(a, s)
    assert got.dtype == torch.float32 and got.shape == (B, 1)
    err = (got[:, 0].double() - ref).abs()
    tol = 1e-5 * ref.abs() + len(table.terms) * 2.0 ** -24 * mag
    print(f"max |err| {float(err.max()):.3e}, max err / tol {float((err / tol).max()):.3f}, values {float(ref.min()):.2f} .. {float(ref.max()):.2f}")
    assert (err <= tol).all()
    # the alive bonus still comes last, over the model's own box
    box = hm.BoxTermination([hm.Interval(0, -0.5, 2.5, hi_open=True)], require_finite=True)
    with_bonus = forms.custom_terms(alive_bonus=0.5, termination_fn=box)(a, s)
    assert torch.equal(with_bonus, got + 0.5 * (~box(a, s)).float())


def test_entries_run_in_table_order_and_a_consumed_group_starts_over():
    a = torch.zeros(1, 1)
    s = torch.tensor([[3.0, 4.0, 2.0]])
    norm = RewardTerms([T("square", 0, level=1), T("square", 1, level=1), T("sqrt", 0, source="group")])
    assert float(norm(a, s)) == 5.0
    # the second group does not see the first one's sum; c is subtracted from the group before f
    two = RewardTerms([T("linear", 0, level=1), T("linear", 0, w=10.0, source="group"), T("linear", 1, level=1), T("linear", 0, c=1.0, source="group")])
    assert float(two(a, s)) == 30.0 + 3.0
    # mul and div combine the weighted term, at every level; bias starts level 0
    prod = RewardTerms([T("linear", 0, level=2), T("linear", 1, w=0.5, level=2, op="mul"), T("linear", 0, source="group", level=1),
                        T("linear", 2, level=1, op="div"), T("linear", 0, source="group", op="mul")], bias=2.0)
    assert float(prod(a, s)) == 2.0 * ((3.0 * (0.5 * 4.0)) / 2.0)
    assert float(RewardTerms([T("linear", 0, c=0.25, source="const"), T("exp", 0, c=0.0, source="const")])(a, s)) == 0.25 + 1.0


# ---- IEEE behaviour -------------------------------------------------------------------------------------------------------------
def test_nan_inf_and_domain_errors_propagate_as_ieee():
    a = torch.zeros(5, 1)
    s = torch.tensor([[4.0, 0.0], [-4.0, 0.0], [float("nan"), 1.0], [float("inf"), 1.0], [1.0, 0.0]])
    root = RewardTerms([T("linear", 0, level=1), T("sqrt", 0, source="group")])(a, s)[:, 0]
    assert float(root[0]) == 2.0 and math.isnan(float(root[1])) and math.isnan(float(root[2])) and float(root[3]) == math.inf
    quot = RewardTerms([T("linear", 0, c=1.0, source="const"), T("linear", 1, op="div")])(a, s)[:, 0]  # 1 / s1
    assert float(quot[0]) == math.inf and float(quot[2]) == 1.0
    neg = RewardTerms([T("linear", 0, c=-1.0, source="const"), T("linear", 1, op="div")])(a, s)[:, 0]
    assert float(neg[0]) == -math.inf
    zero_over_zero = RewardTerms([T("linear", 1, op="div")])(a, s)[:, 0]  # A0 = bias = 0
    assert math.isnan(float(zero_over_zero[0])) and float(zero_over_zero[2]) == 0.0
    trig = RewardTerms([T("sin", 0), T("cos", 0)])(a, s)[:, 0]
    assert math.isnan(float(trig[2])) and math.isnan(float(trig[3])) and math.isfinite(float(trig[0]))  # sin(inf) is NaN
    grow = RewardTerms([T("exp", 0, w=1.0, c=-100.0)])(a, s)[:, 0]  # exp(s0 + 100)
    assert float(grow[0]) == math.inf and float(grow[3]) == math.inf and math.isnan(float(grow[2]))
    # a NaN inside a group reaches the result through the consumption
    through = RewardTerms([T("linear", 0, level=2), T("square", 0, source="group", level=1), T("linear", 0, w=0.0, source="group")])(a, s)[:, 0]
    assert math.isnan(float(through[2])) and math.isnan(float(through[3])) and float(through[0]) == 0.0


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,match", [
    (lambda: [T("linear", 0, level=3)], "term 0: level 3 outside [0, 2]"),
    (lambda: [T("linear", 0), T("linear", 0, level=-1)], "term 1: level -1 outside [0, 2]"),
    (lambda: [T("linear", 0, op="pow")], "term 0: op 'pow' is not one of ('add', 'mul', 'div')"),
    (lambda: [T("tanh", 0)], "term 0: fn 'tanh' is not one of"),
    (lambda: [T("cube", 0)], "term 0: fn 'cube'"),
    (lambda: [T("linear", 0), T("linear", 0, source="state")], "term 1: source 'state'"),
    (lambda: [T("linear", 0, level=2), T("linear", 0, source="group", level=2)], "term 1: 'group' at level 2 has no deeper group to consume"),
    (lambda: [T("linear", 0, source="group")], "term 0: 'group' consumes an empty group (level 1"),
    (lambda: [T("linear", 0, level=1), T("linear", 0, source="group"), T("linear", 0, source="group")], "term 2: 'group' consumes an empty group (level 1"),
    (lambda: [T("linear", 0, level=2), T("linear", 0, source="group")], "term 1: 'group' consumes an empty group (level 1"),
    (lambda: [T("linear", 0), T("linear", 1, level=1, op="mul")], "term 1: 'mul' into an empty group (level 1"),
    (lambda: [T("linear", 0, level=2, op="div")], "term 0: 'div' into an empty group (level 2"),
    (lambda: [T("linear", 0, level=1), T("linear", 1)], "term 0: the group at level 1 is left open at the end of the table"),
    (lambda: [T("linear", 0, level=2), T("linear", 1, level=2), T("linear", 1)], "term 1: the group at level 2 is left open"),
    (lambda: [T("linear", 0, level=1), T("linear", 0, j=1, source="group")], "term 1: j = 1 is set on a 'group' entry"),
    (lambda: [T("linear", 0, j=0, source="const")], "term 0: j = 0 is set on a 'const' entry"),
    (lambda: [T("sin", 5, level=1)] * 65, "at most 64"),
])
def test_ill_formed_tables_are_refused_with_the_entry_named(make, match):
    with pytest.raises(UnsupportedModelError, match=re.escape(match)):
        RewardTerms(make())


def test_what_is_well_formed():
    RewardTerms([T("linear", 0, op="mul"), T("linear", 0, op="div")])  # mul / div into level 0: it starts at the bias
    RewardTerms([T("linear", 0, level=1), T("linear", 1, level=1, op="mul"), T("linear", 0, source="group")])
    RewardTerms([T("linear", 0, level=2), T("linear", 1, level=1), T("linear", 0, source="group", level=1), T("linear", 0, source="group")])  # interleaved levels
    RewardTerms([T("linear", 99, source="const"), T("linear", 0, level=1), T("linear", 99, source="group")]).validate(obs_dim=3, act_dim=1)  # i of const / group is not read
    with pytest.raises(UnsupportedModelError, match=re.escape("term 0: dim i = 3 outside [0, 3)")):
        RewardTerms([T("sqrt", 3)]).validate(obs_dim=3, act_dim=1)
    assert hm.TERM_FNS == ("linear", "square", "abs", "sin", "cos", "exp", "sqrt") and hm.TERM_SOURCES == ("obs", "act", "group", "const")
    assert hm.TERM_OPS == ("add", "mul", "div")
    t = T("square", 1, -0.1, None, 0.0, "act")  # the six v9 fields, positionally: the new ones trail with defaults
    assert (t.level, t.op) == (0, "add")


# ---- packing ----------------------------------------------------------------------------------------------------------------------
def test_a_v9_entry_packs_to_the_v9_codes_and_words_round_trip():
    packed = pack_reward_terms(RewardTerms([T("square", 1, w=-0.1, source="act")]))[0]
    assert (packed.fn, packed.source, packed.i, packed.j) == (1, 1, 1, -1) and packed.c == 0.0 and abs(packed.w + 0.1) < 1e-8
    for name, code in (("linear", 0), ("square", 1), ("abs", 2)):
        assert pack_reward_terms(RewardTerms([T(name, 0)]))[0].fn == code  # level 0, add: the bare fn code
    assert _lib.TERM_FN == {"linear": 0, "square": 1, "abs": 2, "sin": 3, "cos": 4, "exp": 5, "sqrt": 6}
    assert _lib.TERM_SRC == {"obs": 0, "act": 1, "group": 2, "const": 3} and _lib.TERM_OP == {"add": 0, "mul": 1, "div": 2}
    assert [k for k, _ in sorted(_lib.TERM_FN.items(), key=lambda kv: kv[1])] == list(hm.TERM_FNS)
    assert [k for k, _ in sorted(_lib.TERM_SRC.items(), key=lambda kv: kv[1])] == list(hm.TERM_SOURCES)
    assert [k for k, _ in sorted(_lib.TERM_OP.items(), key=lambda kv: kv[1])] == list(hm.TERM_OPS)
    for fn in range(7):
        for op in range(3):
            for level in range(3):
                word = _lib.term_word(fn, op, level)
                assert word == fn | op << 8 | level << 16 and _lib.term_word_fields(word) == (fn, op, level)
    table = forms.custom_terms()
    for t, p in zip(table.terms, pack_reward_terms(table)):
        assert _lib.term_word_fields(p.fn) == (_lib.TERM_FN[t.fn], _lib.TERM_OP[t.op], t.level) and p.source == _lib.TERM_SRC[t.source]
        assert p.j == (-1 if t.j is None else t.j)


def test_the_header_defines_the_word_and_the_new_codes():
    import os

    from conftest import ROOT

    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    assert re.search(r"#define HIPETS_ABI_VERSION 9\b", header)  # additive: no version bump
    for name, value in (("HIPETS_TERM_FN_SIN", 3), ("HIPETS_TERM_FN_COS", 4), ("HIPETS_TERM_FN_EXP", 5), ("HIPETS_TERM_FN_SQRT", 6),
                        ("HIPETS_TERM_SRC_GROUP", 2), ("HIPETS_TERM_SRC_CONST", 3), ("HIPETS_TERM_OP_ADD", 0), ("HIPETS_TERM_OP_MUL", 1),
                        ("HIPETS_TERM_OP_DIV", 2), ("HIPETS_TERM_MAX_LEVEL", _lib.TERM_MAX_LEVEL)):
        assert int(re.search(name + r"\s*=?\s*(\d+)", header).group(1)) == value, name
    assert re.search(r"#define HIPETS_TERM_WORD\(fn, op, level\) \(\(int32_t\)\(\(fn\) \| \(\(op\) << 8\) \| \(\(level\) << 16\)\)\)", header)
    for macro in ("HIPETS_TERM_WORD_FN", "HIPETS_TERM_WORD_OP", "HIPETS_TERM_WORD_LEVEL"):
        assert re.search(r"#define " + macro + r"\(word\)", header)
