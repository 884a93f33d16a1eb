"""Risk-aware particle reductions on the host, no GPU: the float32 restatement's own invariants, ``hipets.ParticleReduce`` (constructors,
validation, the cvar resolution), the two new entry points in header and binding, and -- on the recording stand-in library of
test_engine_binding_host -- which library calls an objective issues: a default objective exactly today's, the setter only on a change."""
import math
import re

import numpy as np
import pytest
import torch

import hipets
from hipets import ParticleReduce, _lib
from particle_reduce_restatement import KINDS, edge_totals, particle_reduce, particle_value, same_bits
from test_abi import HEADER, header_prototypes
from test_engine_binding_host import ACT, OBS, check, make_engine, make_spec, patch_cuda

SHAPES = [(1, 1), (3, 2), (5, 7), (4, 8), (4, 9), (13, 20)]


# ---- the restatement's own invariants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop,P", SHAPES)
def test_worst_k_of_all_particles_is_the_mean(pop, P):
    for first in range(6):
        tot = edge_totals(pop, P, first)
        assert same_bits(particle_reduce(tot, pop, P, "worst_k", k=P), particle_reduce(tot, pop, P, "mean"))


@pytest.mark.parametrize("pop,P", SHAPES)
def test_worst_one_is_the_min_up_to_the_sign_of_a_zero(pop, P):
    for first in range(6):
        tot = edge_totals(pop, P, first)
        worst, low = particle_reduce(tot, pop, P, "worst_k", k=1), particle_reduce(tot, pop, P, "min")
        assert same_bits(worst + np.float32(0.0), low + np.float32(0.0))  # (-0.0 + 0.0 = +0.0; every other value is itself)
    # the one difference: MIN hands the total itself on, WORST_K adds it to s = +0.0 first, and (+0.0) + (-0.0) = +0.0
    assert np.signbit(particle_value([-0.0, 1.0], "min")) and not np.signbit(particle_value([-0.0, 1.0], "worst_k", k=1))
    assert particle_value([-0.0, 1.0], "min") == particle_value([-0.0, 1.0], "worst_k", k=1) == 0.0


def test_one_particle_returns_the_total():
    for x in (3.25, -100.5, 0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        for kind in KINDS:
            if kind == "mean_std" and math.isinf(x):
                continue  # (inf - inf: the spread of one infinite total is NaN by the stated arithmetic)
            got = particle_value([x], kind, kappa=1.5, k=1)
            if x == 0.0:
                assert got == 0.0  # (the sums start from +0.0: the value of a zero total is kept, its sign by MIN / MAX only)
            else:
                assert same_bits(got, np.float32(x)), (kind, x)


@pytest.mark.parametrize("pop,P", SHAPES)
def test_mean_std_of_kappa_zero_is_the_mean_on_finite_totals(pop, P):
    for first in range(3):  # (cases 0..2 of edge_totals with pop <= 3 candidates: finite totals)
        tot = edge_totals(min(pop, 3 - first), P, first)
        n = tot.size // P
        assert np.isfinite(tot).all()
        assert same_bits(particle_reduce(tot, n, P, "mean_std", kappa=0.0), particle_reduce(tot, n, P, "mean"))


def test_hand_made_values():
    t = [4.0, 1.0, 1.0, 3.0]
    assert particle_value(t, "mean") == np.float32(2.25) and particle_value(t, "min") == 1.0 and particle_value(t, "max") == 4.0
    assert particle_value(t, "worst_k", k=1) == 1.0 and particle_value(t, "worst_k", k=2) == 1.0 and particle_value(t, "worst_k", k=3) == np.float32(5.0 / 3.0)
    # q = 3.0625 + 1.5625 + 1.5625 + 0.5625 = 6.75; sqrt(6.75 / 4) = 1.2990381...
    assert particle_value(t, "mean_std", kappa=2.0) == np.float32(np.float32(2.25) - np.float32(2.0) * np.sqrt(np.float32(1.6875)))
    assert particle_value(t, "mean_std", kappa=-1.0) > particle_value(t, "mean")  # optimistic
    # the sum of the k worst runs in PARTICLE order, not in rank order: (1e8 + 1) - 1e8 = 0 in float32, 1e8 + -1e8 + 1 = 1
    assert particle_value([1e8, 1.0, -1e8, 2e8], "worst_k", k=3) == np.float32(0.0)
    assert np.isnan(particle_value([1.0, float("nan"), 2.0], "min")) and np.isnan(particle_value([1.0, float("nan"), 2.0], "worst_k", k=1))
    assert particle_value([1.0, float("inf")], "max") == np.inf and particle_value([1.0, float("-inf")], "worst_k", k=1) == -np.inf


# ---- hipets.ParticleReduce ----------------------------------------------------------------------------------------------------------
def test_constructors():
    R = ParticleReduce
    assert R.mean() == R() == R("mean") and (R.mean().kind, R.mean().kappa, R.mean().worst_k) == ("mean", 0.0, 0)
    assert (R.mean_std(1.5).kind, R.mean_std(1.5).kappa) == ("mean_std", 1.5) and R.mean_std(-2).kappa == -2
    assert R.worst_case().kind == "min" and R.best_case().kind == "max"
    assert (R.worst_k(3).kind, R.worst_k(3).worst_k) == ("worst_k", 3)
    assert R.cvar(0.25).kind == "cvar"
    with pytest.raises(Exception):  # frozen
        R.mean().kappa = 1.0
    assert R.coerce(None) == R.coerce("mean") == R.mean() and R.coerce("min") == R.worst_case() and R.coerce("max") == R.best_case()
    assert R.coerce(R.worst_k(2)) == R.worst_k(2)
    assert R.worst_k(2).abi_args() == {"kind": 4, "kappa": 0.0, "worst_k": 2} and R.mean_std(0.5).abi_args() == {"kind": 1, "kappa": 0.5, "worst_k": 0}


@pytest.mark.parametrize("alpha,P,k", [(0.2, 20, 4), (1.0, 20, 20), (1.0, 1, 1), (0.05, 20, 1), (0.01, 20, 1), (0.3, 10, 3), (0.1, 30, 3), (0.7, 10, 7),
                                       (0.15, 20, 3), (0.21, 20, 5), (0.5, 7, 4), (1e-9, 256, 1)])
def test_cvar_resolution(alpha, P, k):
    r = ParticleReduce.cvar(alpha).resolve(P)
    assert r == ParticleReduce.worst_k(k)
    assert k == max(1, math.ceil(round(alpha * P, 9)))
    assert ParticleReduce.worst_k(2).resolve(P) == ParticleReduce.worst_k(2) and ParticleReduce.mean().resolve(P) == ParticleReduce.mean()


@pytest.mark.parametrize("bad", [lambda: ParticleReduce("median"), lambda: ParticleReduce.mean_std(float("nan")), lambda: ParticleReduce.mean_std(float("inf")),
                                 lambda: ParticleReduce.mean_std("1"), lambda: ParticleReduce.worst_k(0), lambda: ParticleReduce.worst_k(-3),
                                 lambda: ParticleReduce.worst_k(1.5), lambda: ParticleReduce.cvar(0.0), lambda: ParticleReduce.cvar(1.0001),
                                 lambda: ParticleReduce.cvar(-0.1), lambda: ParticleReduce.cvar(float("nan")), lambda: ParticleReduce.coerce("worst"),
                                 lambda: ParticleReduce.coerce(3)])
def test_validation_raises_value_error(bad):
    with pytest.raises(ValueError):
        bad()


# ---- header, binding, version -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound_and_the_version_stays():
    protos = header_prototypes()
    assert protos["hipets_set_particle_reduce"] == ("int", [("hipets_engine*", "e"), ("int32_t", "kind"), ("float", "kappa"), ("int32_t", "worst_k")])
    assert protos["hipets_particle_reduce"] == ("int", [("hipets_engine*", "e"), ("float*", "totals"), ("int32_t", "pop"), ("int32_t", "num_particles"),
                                                        ("float*", "returns"), ("void*", "stream")])
    assert "hipets_set_particle_reduce" in _lib.SYMBOLS and "hipets_particle_reduce" in _lib.SYMBOLS
    src = open(HEADER).read()
    assert re.search(r"#define HIPETS_ABI_VERSION 9\b", src) and _lib.ABI_VERSION == 9
    codes = dict(re.findall(r"HIPETS_REDUCE_([A-Z_]+) = (\d)", src))
    assert {k.lower(): int(v) for k, v in codes.items()} == _lib.REDUCE
    assert hipets.ParticleReduce is ParticleReduce and hasattr(hipets.Engine, "set_particle_reduce") and hasattr(hipets.Engine, "particle_reduce")


# ---- the library calls of an objective, on the recording stand-in -----------------------------------------------------------------------
POP, P, H = 6, 2, 3
S0 = np.zeros(OBS, np.float32)


@pytest.fixture
def eng(monkeypatch):
    patch_cuda(monkeypatch)
    e = make_engine()
    e.reduce = ParticleReduce()  # (what Engine.__init__ sets: the library's initial value)
    yield e
    e._h = None


def calls(eng):
    """The symbols called since the last look (and their records), oldest first."""
    out = list(eng._lib.calls)
    eng._lib.calls.clear()
    return out


def actions():
    return torch.zeros(POP, H, ACT)


def test_engine_methods_bind_the_entry_points(eng):
    eng.set_particle_reduce(ParticleReduce.mean_std(0.75))
    (sym, rec), = calls(eng)
    assert sym == "hipets_set_particle_reduce" and eng.reduce == ParticleReduce.mean_std(0.75)
    check(rec, sym, kind=1, kappa=0.75, worst_k=0)
    eng.set_particle_reduce(ParticleReduce.worst_k(3))
    (sym, rec), = calls(eng)
    check(rec, sym, kind=4, kappa=0.0, worst_k=3)
    tot = torch.zeros(POP * P)
    out = eng.particle_reduce(tot, POP, P)
    (sym, rec), = calls(eng)
    assert sym == "hipets_particle_reduce" and out.shape == (POP,) and out.dtype == torch.float32
    check(rec, sym, totals=tot, pop=POP, num_particles=P, returns=out)
    with pytest.raises(ValueError, match="totals must have 12 elements, got 6"):
        eng.particle_reduce(torch.zeros(POP), POP, P)
    assert calls(eng) == []


def test_a_default_objective_issues_todays_calls_and_the_setter_appears_only_on_a_change(eng):
    spec = make_spec()
    default = hipets.HipTrajectoryEvalFn(spec, P, engine=eng, mode="device")
    assert [s for s, _ in calls(eng)] == ["hipets_set_model"]
    default(S0, actions())
    default(S0, actions())
    assert [s for s, _ in calls(eng)] == ["hipets_rollout", "hipets_rollout"]  # no setter: a fresh engine is at the mean
    named = hipets.HipTrajectoryEvalFn(spec, P, engine=eng, mode="device", particle_reduce="mean")
    calls(eng)
    named(S0, actions())
    assert [s for s, _ in calls(eng)] == ["hipets_rollout"]
    low = hipets.HipTrajectoryEvalFn(spec, P, engine=eng, mode="device", particle_reduce="min")
    assert [s for s, _ in calls(eng)] == ["hipets_set_model"]  # construction binds the model, nothing else
    low(S0, actions())
    (s1, r1), (s2, _) = calls(eng)
    assert (s1, s2) == ("hipets_set_particle_reduce", "hipets_rollout")
    check(r1, s1, kind=2, kappa=0.0, worst_k=0)
    low(S0, actions())
    assert [s for s, _ in calls(eng)] == ["hipets_rollout"]  # unchanged: no setter
    default(S0, actions())  # the shared engine goes back to the mean
    (s1, r1), (s2, _) = calls(eng)
    assert (s1, s2) == ("hipets_set_particle_reduce", "hipets_rollout")
    check(r1, s1, kind=0, kappa=0.0, worst_k=0)
    default(S0, actions())
    assert [s for s, _ in calls(eng)] == ["hipets_rollout"]


def test_cvar_is_resolved_with_the_objectives_own_particles(eng):
    fn = hipets.HipTrajectoryEvalFn(make_spec(), 20, engine=eng, mode="fast", particle_reduce=ParticleReduce.cvar(0.2))
    calls(eng)
    fn(S0, torch.zeros(3, H, ACT))
    (s1, r1), (s2, _) = calls(eng)
    assert (s1, s2) == ("hipets_set_particle_reduce", "hipets_rollout")
    check(r1, s1, kind=4, kappa=0.0, worst_k=4)
    assert eng.reduce == ParticleReduce.worst_k(4)
    with pytest.raises(ValueError):
        hipets.HipTrajectoryEvalFn(make_spec(), 20, engine=eng, particle_reduce="median")
    assert calls(eng) == []  # refused before the model was bound


def test_model_env_takes_the_reduction_per_call(eng):
    env = hipets.ModelEnv(make_spec(), engine=eng, mode="device")
    calls(eng)
    env.evaluate_action_sequences(actions(), S0, P)
    assert [s for s, _ in calls(eng)] == ["hipets_rollout"]
    env.evaluate_action_sequences(actions(), S0, P, particle_reduce=ParticleReduce.mean_std(1.0))
    assert [s for s, _ in calls(eng)] == ["hipets_set_particle_reduce", "hipets_rollout"]
    env.evaluate_action_sequences(actions(), S0, P)
    (s1, r1), (s2, _) = calls(eng)
    assert (s1, s2) == ("hipets_set_particle_reduce", "hipets_rollout")
    check(r1, s1, kind=0, kappa=0.0, worst_k=0)


def test_the_unfused_objective_reduces_through_the_engine_unless_it_is_the_mean(eng):
    rew = lambda act, nobs: nobs[:, :1]  # noqa: E731
    plain = hipets.UnfusedTrajectoryEvalFn(make_spec(), P, reward_fn=rew, engine=eng)
    calls(eng)
    out = plain(S0, actions())
    assert [s for s, _ in calls(eng)] == ["hipets_step"] * H and out.shape == (POP,)  # the mean stays the torch line it is
    risk = hipets.make_eval_fn(make_spec(), P, engine=eng, particle_reduce=ParticleReduce.worst_k(2))
    assert type(risk) is hipets.HipTrajectoryEvalFn and risk.particle_reduce == ParticleReduce.worst_k(2)
    risk = hipets.UnfusedTrajectoryEvalFn(make_spec(), P, reward_fn=rew, engine=eng, particle_reduce=ParticleReduce.worst_k(2))
    calls(eng)
    out = risk(S0, actions())
    got = calls(eng)
    assert [s for s, _ in got] == ["hipets_set_particle_reduce"] + ["hipets_step"] * H + ["hipets_particle_reduce"]
    check(got[0][1], got[0][0], kind=4, kappa=0.0, worst_k=2)
    assert (got[-1][1]["pop"], got[-1][1]["num_particles"], got[-1][1]["returns"]) == (POP, P, out.data_ptr()) and out.shape == (POP,)
