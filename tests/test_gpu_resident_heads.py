"""The resident-heads instances of the fused fp32 R = 3 shapes (kspec.hpp KSpec::RES): in the straight persistent form of a DEVICE
rollout -- as many launched as logical workgroups, each bound to one member for the launch -- a wave keeps the biases and the chunk-0
weight fragments of its five ops in AccVGPRs.  Same operands in the same order, so ONE persistent launch must equal the H per-step
launches of the plain instance (`set_persistent(False)`) bit for bit; what can go wrong is WHICH heads a wave holds (another member's,
another model's, another wave's) and whether the launch is the straight persistent one at all.  Which calls get the instance is a
host rule: tests/test_resident_heads_rule.py."""
import numpy as np
import pytest
import torch

import hipets
from conftest import to_spec
from test_gpu_rollout import _random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, ACT, P, M, R = 17, 6, 20, 5, 3  # the cfg2 shape, three row tiles (48 rows) per workgroup


def _both_forms(engine, actions, s0, **kw):
    """(one persistent launch, H per-step launches) of the same call"""
    kw = dict(mode="device", seed=77, stream_id=9, rows_per_group=R, **kw)
    a = engine.rollout(actions.to(DEV), s0, P, **kw)
    engine.set_persistent(False)
    try:
        b = engine.rollout(actions.to(DEV), s0, P, **kw)
    finally:
        engine.set_persistent(True)
    return a, b


# pop 12: 240 rows = exactly one full 48-row workgroup per member, 5 workgroups -- the smallest launch of the resident instance;
# pop 13: 52 rows per member, a second workgroup per member with 4 live rows and 44 padding rows; H 1: the heads are loaded, used once
# (a single step has no hand-over: the call runs as one per-step launch of the plain instance and must agree all the same)
@pytest.mark.parametrize("pop,H", [(12, 4), (13, 4), (12, 1)], ids=["pop12_H4", "pop13_H4_padding_rows", "pop12_H1"])
def test_persistent_launch_equals_per_step_launches(engine, pop, H):
    om, actions, s0, _, _ = _random_case(OBS, ACT, pop, P, H, ensemble_size=M, hid=200)
    engine.set_model(to_spec(om, OBS, ACT))
    assert engine.kernel_class(pop, P, H, "device", rows_per_group=R) == ("fused", R)
    a, b = _both_forms(engine, actions, s0)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_heads_follow_the_model(engine):
    """set_model(A), rollout, set_model(B), rollout: the second launch holds B's heads, not stale ones."""
    pop, H = 12, 4
    om_a, actions, s0, _, _ = _random_case(OBS, ACT, pop, P, H, seed=0, ensemble_size=M, hid=200)
    om_b = _random_case(OBS, ACT, pop, P, H, seed=5, ensemble_size=M, hid=200)[0]
    engine.set_model(to_spec(om_a, OBS, ACT))
    ra, ra_ref = _both_forms(engine, actions, s0)
    engine.set_model(to_spec(om_b, OBS, ACT))
    rb, rb_ref = _both_forms(engine, actions, s0)
    assert torch.equal(ra, ra_ref) and torch.equal(rb, rb_ref)
    assert not torch.equal(ra, rb)


def test_heads_are_the_elite_members(engine):
    """7 members, elites [0, 2, 3, 5, 6], on the stock pets_halfcheetah model (obs 18 through preprocess_fn, no_delta_list [0]): member
    domain d runs elite[d]'s weights, so must its resident heads."""
    obs, act, pop, H = 18, 6, 12, 4
    om, actions, s0, _, _ = _random_case(obs, act, pop, P, H, ensemble_size=7, hid=200, elite=[0, 2, 3, 5, 6], obs_process="halfcheetah",
                                         no_delta_list=[0])
    engine.set_model(to_spec(om, obs, act))
    assert engine.kernel_class(pop, P, H, "device", rows_per_group=R) == ("fused", R)
    a, b = _both_forms(engine, actions, s0)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_the_pop12_rollout_is_one_launch(engine):
    """Without this a silent fall-back to per-step launches would pass every comparison above."""
    pop, H = 12, 4
    om, actions, s0, _, _ = _random_case(OBS, ACT, pop, P, H, ensemble_size=M, hid=200)
    engine.set_model(to_spec(om, OBS, ACT))
    kw = dict(mode="device", seed=77, stream_id=9, rows_per_group=R)
    engine.rollout(actions.to(DEV), s0, P, **kw)  # warm-up: the co-residency self-test of this instance and grid
    try:
        engine.timing_enable(1)
        engine.timing_read(reset=True)
        engine.rollout(actions.to(DEV), s0, P, **kw)
        torch.cuda.synchronize()
        n, _ = engine.timing_read(reset=True)
    finally:
        engine.timing_enable(0)
    assert n == 1
