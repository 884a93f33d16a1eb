"""hipets.SACUpdater's host side, without a GPU: the restatement of one SAC update (tests/sac_restatement.py) against the recording of
the reference's own SAC.update_parameters (tests/golden/sac_update_cases.npz, tests/make_sac_update_golden.py), the batch packing and
the reverse_mask rule, the refusals and make_sac_updater's fallback, and the ABI additions."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import hipets
import sac_restatement as sr
from conftest import GOLDEN, ROOT
from hipets import _lib
from hipets import mbpo

REC = np.load(os.path.join(GOLDEN, "sac_update_cases.npz"))


@pytest.mark.parametrize("name", sr.RECORDED)
def test_float32_restatement_equals_the_reference_recording(name):
    """Bit for bit: parameters, target network, log_alpha, both Adam moments and the 5-tuple after one update, with the recorded
    normal tables."""
    case = sr.build_case(name)
    eps = [(REC[f"{name}/eps_next"], REC[f"{name}/eps_cur"])]
    st, outs = sr.restate(case, torch.float32, eps=eps)
    names = sr.POLICY + sr.CRITIC + sr.TARGET + (("log_alpha",) if case["tuning"] else ())
    for n in names:
        assert np.array_equal(st["p"][n].numpy(), REC[f"{name}/p/{n}"]), f"{name}: parameter {n}"
        if n[0] != "t":
            assert np.array_equal(st["m"][n].numpy(), REC[f"{name}/m/{n}"]), f"{name}: exp_avg of {n}"
            assert np.array_equal(st["v"][n].numpy(), REC[f"{name}/v/{n}"]), f"{name}: exp_avg_sq of {n}"
    got = [float(v) for v in outs[0]["losses"]]
    assert got == [float(v) for v in REC[f"{name}/result"]], f"{name}: the 5-tuple"


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_every_case_meets_the_condition_on_its_inputs(name):
    sr.build_case(name)  # (asserts check_kinks)


def test_tiny_sac_takes_the_restatement_s_step():
    """The stand-in agent's stock-torch update (torch.optim.Adam) and the float32 restatement agree bit for bit on the CPU."""
    case = sr.build_case("s5_2_15_15")
    sac, memory = sr.agent_for(case, "cpu")
    B, act = case["shape"][3], case["shape"][1]
    torch.manual_seed(7)
    res = sac.update_parameters(memory, B, 0, None, reverse_mask=True)
    torch.manual_seed(7)
    eps = [(torch.empty(B, act).normal_(), torch.empty(B, act).normal_())]
    st, outs = sr.restate(case, torch.float32, eps=eps)
    for n, t in sac.params().items():
        assert torch.equal(t.detach(), st["p"][n]), n
    assert [float(v) for v in outs[0]["losses"]] == list(res)


def test_tiny_sac_resumes_as_the_restatement_does():
    """Three optimizers that share no setting, resumed from non-zero moments at three step counts: torch.optim.Adam in the stand-in
    agent and the float32 restatement agree bit for bit -- parameters, both moments, the step counts and the 5-tuple."""
    case = sr.build_case("resumed")
    sac, memory = sr.agent_for(case, "cpu")
    for which, own in sr.RESUMED_ADAM.items():
        group = getattr(sac, which + "_optim").param_groups[0]
        assert (group["lr"], tuple(group["betas"]), group["eps"]) == (own["lr"], own["betas"], own["eps"])
    assert sac.target_entropy == case["target_entropy"] != -float(case["shape"][1])
    B, act = case["shape"][3], case["shape"][1]
    torch.manual_seed(7)
    res = sac.update_parameters(memory, B, 0, None, reverse_mask=True)
    torch.manual_seed(7)
    eps = [(torch.empty(B, act).normal_(), torch.empty(B, act).normal_())]
    st, outs = sr.restate(case, torch.float32, eps=eps)
    live = sac.params()
    for n, t in live.items():
        assert torch.equal(t.detach(), st["p"][n]), n
    for n in sr.MOMENTS:
        state = sac.optimizer_of(n).state[live[n]]
        which = "alpha" if n == "log_alpha" else ("policy" if n[0] == "p" else "critic")
        assert torch.equal(state["exp_avg"], st["m"][n]) and torch.equal(state["exp_avg_sq"], st["v"][n]), n
        assert float(state["step"]) == st["steps"][which] == sr.RESUMED_STEPS[which] + 1, n
        assert not torch.equal(st["m"][n], case["start"]["m"][n].float()) and (case["start"]["v"][n] > 0).all()
    assert [float(v) for v in outs[0]["losses"]] == list(res)


@pytest.mark.parametrize("swap", sr.SWAPS, ids=lambda s: "-".join(s))
def test_resumed_case_tells_the_optimizers_apart(swap):
    """The condition that makes parity with "resumed" a check of the per-optimizer indexing: exchanging one quantity (a learning
    rate, a beta, an eps, a step count) between two optimizers moves some parameter or moment of the float64 restatement by more than
    twice what train_restatement.check allows there."""
    for name in ("resumed", "resumed_three"):
        what, ratio = sr.build_case(name)["swaps"][swap]
        print(f"{name}: {swap}: {what} moves {ratio:.1f}x the allowance")
        assert ratio > 2.0


def test_allowance_is_the_rule_of_check():
    g = torch.Generator().manual_seed(0)
    f64 = torch.randn(50, generator=g, dtype=torch.float64)
    near, far = f64 + 1e-6 * torch.randn(50, generator=g, dtype=torch.float64), f64 + 1e-4 * torch.randn(50, generator=g, dtype=torch.float64)
    for f32, others in ((near, ()), (near, [far]), (far, [near]), (near, [near * (1 + 1e-7)])):
        allow = sr.allowance(f32, f64, others)
        at = f64.clone()
        at[3] += allow * 0.999
        sr.tr.check(at, f32, f64, "inside the allowance", others)
        at[3] = f64[3] + allow * 1.001
        with pytest.raises(AssertionError):
            sr.tr.check(at, f32, f64, "past the allowance", others)


def test_pack_sac_batch_and_the_reverse_mask_rule():
    g = np.random.default_rng(0)
    B, obs, act = 7, 3, 2
    tr = (g.normal(size=(B, obs)), g.normal(size=(B, act)).astype(np.float32), g.normal(size=(B, obs)), g.normal(size=B),
          np.array([0, 1, 0, 0, 1, 1, 0], dtype=bool), np.ones(B, dtype=bool))
    for reverse in (False, True):
        out = mbpo.pack_sac_batch(tr, reverse)
        assert out.dtype == np.float32 and out.shape == (B, 2 * obs + act + 2)
        assert np.array_equal(out[:, :obs], tr[0].astype(np.float32)) and np.array_equal(out[:, obs:obs + act], tr[1])
        assert np.array_equal(out[:, obs + act:2 * obs + act], tr[2].astype(np.float32))
        assert np.array_equal(out[:, 2 * obs + act], tr[3].astype(np.float32))
        # sac.py:93-95: the flag as a float, or its logical_not
        mask = torch.FloatTensor(tr[4].astype(np.float32))
        want = mask.logical_not().float() if reverse else mask
        assert np.array_equal(out[:, -1], want.numpy())
    into = np.zeros((B, 2 * obs + act + 2), dtype=np.float32)
    assert mbpo.pack_sac_batch(tr, True, out=into) is into and np.array_equal(into, mbpo.pack_sac_batch(tr, True))


class _FakeEngine:
    device = torch.device("cuda:0")


def _refused(sac, match, **kw):
    with pytest.raises(hipets.UnsupportedModelError, match=match):
        hipets.SACUpdater(sac, **kw)


def test_refusals_at_construction():
    _refused(sr.TinySAC(5, 2, 8, deterministic=True, tuning=False), "GaussianPolicy")
    _refused(sr.TinySAC(5, 2, 8), "on cpu")                                     # modules off the GPU, no engine given
    _refused(sr.TinySAC(5, 2, 8), "engine's device", engine=_FakeEngine())      # modules on another device than the engine's
    for key, value in (("amsgrad", True), ("weight_decay", 1e-4), ("maximize", True)):
        sac = sr.TinySAC(5, 2, 8)
        sac.critic_optim.param_groups[0][key] = value
        _refused(sac, key)
    sac = sr.TinySAC(5, 2, 8)
    sac.policy_optim = torch.optim.SGD(sac.policy.parameters(), lr=1e-3)
    _refused(sac, "policy_optim")
    _refused(sr.TinySAC(513, 2, 8), "obs 513")
    _refused(sr.TinySAC(5, 33, 8), "act 33")
    _refused(sr.TinySAC(5, 2, 1025), "hidden 1025")
    for batch in (0, 1025):
        _refused(sr.TinySAC(5, 2, 8), "batch", batch_size=batch)
    _refused(object(), "not shaped like a SAC agent")


def test_make_sac_updater_falls_back_with_one_warning():
    sac = sr.TinySAC(5, 2, 8, deterministic=True, tuning=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        up = hipets.make_sac_updater(sac)
    assert len(w) == 1 and "GaussianPolicy" in str(w[0].message) and "update_parameters" in str(w[0].message)
    assert up.update_parameters == sac.update_parameters  # the agent's own bound method
    wrapped = type("Agent", (), {})()
    wrapped.sac_agent = sac
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert hipets.make_sac_updater(wrapped).update_parameters == sac.update_parameters
    assert len(w) == 1


def test_abi_additions_keep_the_version():
    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    assert re.search(r"#define HIPETS_ABI_VERSION 9\b", header) and _lib.ABI_VERSION == 9
    for name in ("hipets_sac_bind", "hipets_sac_update", "hipets_sac_forward_taps"):
        assert name in _lib.SYMBOLS and re.search(r"\bint " + name + r"\(", header)
    assert re.search(r"#define HIPETS_SAC_N_PTRS 78\b", header) and _lib.SAC_N_PTRS == 78
    assert re.search(r"#define HIPETS_SAC_MAX_BATCH 1024\b", header) and _lib.SAC_MAX_BATCH == 1024
    assert "sac.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "Out of scope: SAC's updates" not in open(os.path.join(ROOT, "mbrl-lib_amd", "hipets", "mbpo.py")).read()
