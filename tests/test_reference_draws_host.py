"""hipets.reference_draws against the oracle on the host, bitwise: what is drawn, from which generator, in which order."""
import itertools
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import to_spec
from hipets import reference_draws as rd
from oracle import pets_oracle as po

OBS, ACT, E, POP, P, H = 5, 2, 4, 6, 2, 3
B = POP * P


def _model(kind, propagation, deterministic):
    return po.make_synthetic_model(OBS, ACT, ensemble_size=E, hid=8, ensemble_kind=kind, propagation=propagation, deterministic=deterministic)


def _seeded():
    torch.manual_seed(11)
    return torch.Generator().manual_seed(22)


def test_rollout_draws_replay_the_oracle_rollout_and_leave_both_generators_where_it_does():
    """Both ensemble kinds x the three propagations x deterministic on / off: the oracle drawing for itself (global_rng + generator)
    and the oracle fed ``rollout_draws`` give equal returns, an equal global RNG state and an equal generator state."""
    g0 = torch.Generator().manual_seed(3)
    actions = torch.rand(POP, H, ACT, generator=g0) * 2 - 1
    s0 = (np.random.default_rng(0).standard_normal(OBS) * 0.1).astype(np.float32)
    for kind, propagation, deterministic in itertools.product(("gaussian_mlp", "basic_ensemble"), ("random_model", "fixed_model", "expectation"),
                                                              (False, True)):
        om = _model(kind, propagation, deterministic)
        g = _seeded()
        ref = po.rollout(om, actions, s0, P, global_rng=True, generator=g)
        ref_state = (torch.get_rng_state(), g.get_state())
        g = _seeded()
        perms, members, eps = rd.rollout_draws(to_spec(om, OBS, ACT), B, H, g)
        out = po.rollout(om, actions, s0, P, perms=perms, members=members, eps=eps)
        case = (kind, propagation, deterministic)
        assert torch.equal(out, ref), case
        assert torch.equal(torch.get_rng_state(), ref_state[0]), case
        assert torch.equal(g.get_state(), ref_state[1]), case
        drawn = [t is not None for t in (perms, members, eps)]
        stochastic_map = propagation != "expectation"
        assert drawn == [stochastic_map and kind == "gaussian_mlp", stochastic_map and kind == "basic_ensemble", not deterministic], case


def test_rollout_draws_are_one_reset_and_h_steps():
    for kind, propagation, deterministic in itertools.product(("gaussian_mlp", "basic_ensemble"), ("random_model", "fixed_model", "expectation"),
                                                              (False, True)):
        spec = to_spec(_model(kind, propagation, deterministic), OBS, ACT)
        g = _seeded()
        perms, members, eps = rd.rollout_draws(spec, B, H, g)
        state = (torch.get_rng_state(), g.get_state())
        g = _seeded()
        fixed = rd.reset_draws(spec, B, g)
        steps = [rd.step_draws(spec, B, g, True) for _ in range(H)]
        assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(g.get_state(), state[1])
        maps = perms if kind == "gaussian_mlp" else members
        if propagation == "fixed_model":
            assert torch.equal(maps, fixed) and all(m is None for m, _ in steps)
        elif propagation == "random_model":
            assert fixed is None and torch.equal(maps, torch.stack([m for m, _ in steps]))
        else:
            assert fixed is None and maps is None and all(m is None for m, _ in steps)
        if deterministic:
            assert eps is None and all(e is None for _, e in steps)
        else:
            assert torch.equal(eps, torch.stack([e for _, e in steps]))
    # sample=False (ModelEnv.step's default) draws no normal and leaves the generator alone
    spec = to_spec(_model("gaussian_mlp", "expectation", False), OBS, ACT)
    g = _seeded()
    before = g.get_state()
    assert rd.step_draws(spec, B, g, False) == (None, None) and torch.equal(g.get_state(), before)


def test_icem_iteration_draws_follow_the_reference_order():
    """Two spectrum normals (the oracle's powerlaw_psd_gaussian records them), then randperm(K) with elites, then the end noise
    at i == 0: values and the generator state afterwards."""
    n, Hh, A, K, keep = 9, 5, 2, 4, 3
    for has_elite, first in itertools.product((False, True), (False, True)):
        torch.manual_seed(7)
        rec = []
        po.powerlaw_psd_gaussian(2.0, size=(n, A, Hh), record_normals=rec)
        want = {"normals": torch.stack(rec[0])}
        if has_elite:
            want["keep_perm"] = torch.randperm(K)
            if first:
                want["end_noise"] = torch.empty(keep, A).normal_(0.0, 1.0)
        state = torch.get_rng_state()
        torch.manual_seed(7)
        got = rd.icem_iteration_draws(n, Hh, A, K, keep, has_elite, first)
        assert sorted(got) == sorted(want)
        assert all(torch.equal(got[k], want[k]) for k in want)
        assert torch.equal(torch.get_rng_state(), state)
        assert got["normals"].shape == (2, n, A, Hh // 2 + 1)


def test_reference_noise_consumes_the_global_generator_like_the_reference():
    """sampler='torch': the product's draw routine == mbrl.util.math.truncated_normal_ (util/math.py:69-92, restated in the
    oracle and pinned bitwise against the reference) on the same torch.manual_seed; the clipped-normal branch is randn."""
    torch.manual_seed(123)
    a = rd.population_noise((40, 6, 3), clipped_normal=False)
    after_a = torch.rand(1)
    torch.manual_seed(123)
    b = po.truncated_normal_(torch.zeros(40, 6, 3))
    after_b = torch.rand(1)
    assert torch.equal(a, b) and torch.equal(after_a, after_b)  # same values AND same generator state afterwards
    assert a.abs().max() <= 2.0
    torch.manual_seed(5)
    c = rd.population_noise((7, 2), clipped_normal=True)
    torch.manual_seed(5)
    assert torch.equal(c, torch.randn(7, 2))


def test_elite_indices_are_torch_topk_after_the_nan_filter():
    """Ties keep the order torch.topk gives them on the host; a NaN counts as -1e-10 (trajectory_opt.py:178-179)."""
    v = torch.tensor([1.0, -1.0, 1.0, float("nan"), 1.0, -1.0, 0.5, 1.0, -2.0, 1.0])
    filtered = v.clone()
    filtered[3] = -1e-10
    for k in (1, 3, 5, 6, 7, 9):
        got = rd.elite_indices(v, k)
        assert got.dtype == torch.int32 and got.device.type == "cpu"
        assert torch.equal(got.long(), torch.topk(filtered, k).indices)
    assert torch.equal(rd.elite_indices(v, 7).long().sort().values, torch.tensor([0, 2, 3, 4, 6, 7, 9]))  # the NaN ranks above the -1s
    assert v[3].isnan()  # the input is left alone


def test_importing_reference_draws_does_not_load_the_library():
    code = "import sys, hipets.reference_draws, hipets._lib as l; sys.exit(0 if l._lib is None else 1)"
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(rd.__file__)))
    assert subprocess.run([sys.executable, "-c", code], env=env).returncode == 0
