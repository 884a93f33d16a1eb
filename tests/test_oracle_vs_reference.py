"""Pins the oracle against the UNMODIFIED reference: what the reference's own classes returned for these cases is recorded in
tests/golden/reference_outputs.npz (and a checkpoint its OneDTransitionRewardModel.save wrote in tests/golden/reference_checkpoint/)
by oracle/ref_cases.py, which also holds the cases' inputs.  Every comparison is bitwise.

Not covered here: hipets.spec_from_model_env / spec_from_planet_model on the reference's LIVE objects (a ModelEnv, a BasicEnsemble,
a PlaNetModel) and the model_version / planet_version freshness tokens following their in-place updates.  Live objects cannot be
stored as data, so those checks run in oracle/ref_cases.check_live_objects each time the fixtures are recorded, not in this suite."""
import numpy as np
import pytest
import torch

from oracle import pets_oracle as po
from oracle import ref_cases as rc


@pytest.fixture(scope="module")
def ref():
    return rc.load_outputs()


@pytest.mark.parametrize("case", rc.ROLLOUT_CASES, ids=rc.rollout_case_id)
def test_rollout_bitwise_vs_reference(ref, case):
    om, actions, s0 = rc.rollout_inputs(case)
    torch.manual_seed(42)
    mine = po.rollout(om, actions, s0, case["P"], global_rng=True, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ref[f"rollout/{rc.rollout_case_id(case)}"], mine)


@pytest.mark.parametrize("propagation", rc.PROPAGATIONS)
def test_basic_ensemble_per_member_logvar_bounds_bitwise(ref, propagation):
    """Every BasicEnsemble member is its own GaussianMLP with its own (learned) logvar bounds."""
    om, actions, s0, P = rc.basic_ensemble_bounds_inputs(propagation)
    mine = po.rollout(om, actions, s0, P, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ref[f"basic_bounds/{propagation}"], mine)


def test_member_map_equals_perm():
    """The oracle's explicit row->member map (used to check FAST mode) == the reference's perm form."""
    om = po.make_synthetic_model(17, 6, ensemble_size=5, hid=24, seed=0)
    B, H, P = 50, 3, 5
    g = torch.Generator().manual_seed(0)
    actions = torch.rand(B // P, H, 6, generator=g)
    s0 = np.zeros(17, np.float32)
    perms = torch.stack([torch.randperm(B, generator=g) for _ in range(H)])
    eps = torch.randn(H, B, 17, generator=g)
    members = torch.empty(H, B, dtype=torch.long)
    for t in range(H):
        members[t][perms[t]] = torch.arange(B) // (B // 5)
    a = po.rollout(om, actions, s0, P, perms=perms, eps=eps)
    b = po.rollout(om, actions, s0, P, members=members, eps=eps)
    assert torch.allclose(a, b, rtol=0, atol=1e-6)


@pytest.mark.parametrize("clipped,return_mean", rc.CEM_CASES)
def test_cem_bitwise_vs_reference(ref, clipped, return_mean):
    H, A, pop, lb, ub, obj = rc.cem_inputs()
    torch.manual_seed(0)
    mine = po.cem_optimize(obj, torch.zeros(H, A), torch.tensor(lb), torch.tensor(ub), 3, 0.2, pop, 0.1,
                           return_mean_elites=return_mean, clipped_normal=clipped)
    assert torch.equal(ref[f"cem/{clipped}-{return_mean}"], mine)


def test_mppi_bitwise_vs_reference_two_calls(ref):
    """Two consecutive plans: pins the persistent mean and the past_action aliasing quirk (Appendix B4/B6)."""
    H, A, pop, lb, ub, obj = rc.mppi_inputs()
    st = po.MPPIState(H, A)
    torch.manual_seed(1)
    m1 = po.mppi_optimize(obj, st, torch.tensor(lb), torch.tensor(ub), 3, pop, 0.9, 1.0, 0.9)
    m2 = po.mppi_optimize(obj, st, torch.tensor(lb), torch.tensor(ub), 3, pop, 0.9, 1.0, 0.9)
    assert torch.equal(ref["mppi/1"], m1) and torch.equal(ref["mppi/2"], m2)


def test_mppi_sigma_is_dead():
    """Appendix B5: sigma does not influence the sampled population."""
    H, A, pop = 4, 2, 16
    lb, ub = torch.full((H, A), -1.0), torch.full((H, A), 1.0)
    obj = rc.quadratic(torch.zeros(H, A))
    outs = []
    for sigma in (0.01, 5.0):
        torch.manual_seed(3)
        outs.append(po.mppi_optimize(obj, po.MPPIState(H, A), lb, ub, 2, pop, 0.9, sigma, 0.9))
    assert torch.equal(outs[0], outs[1])


def test_icem_bitwise_vs_reference_two_calls(ref):
    """Two plans: pins coloured noise, population decay, kept-elite shift / append, biased variance."""
    H, A, lb, ub, obj, kw = rc.icem_inputs()
    st = po.ICEMState()
    torch.manual_seed(2)
    m1 = po.icem_optimize(obj, st, torch.zeros(H, A), torch.tensor(lb), torch.tensor(ub), return_mean_elites=True,
                          population_size_module=5, **kw)
    m2 = po.icem_optimize(obj, st, m1.clone(), torch.tensor(lb), torch.tensor(ub), return_mean_elites=True,
                          population_size_module=5, **kw)
    assert torch.equal(ref["icem/1"], m1) and torch.equal(ref["icem/2"], m2)


@pytest.mark.parametrize("n", rc.POWERLAW_N)
def test_powerlaw_noise_bitwise(ref, n):
    torch.manual_seed(0)
    mine = po.powerlaw_psd_gaussian(2.0, size=(7, 3, n))
    assert torch.equal(ref[f"powerlaw/{n}"], mine)


def test_truncated_normal_bitwise(ref):
    torch.manual_seed(0)
    mine = po.truncated_normal_(torch.empty(50, 7))
    assert torch.equal(ref["truncated_normal"], mine)


def test_trajectory_optimizer_shift(ref):
    """trajectory_opt.py:563-568: warm start rolled by replan_freq and refilled with (lb+ub)/2."""
    H, A, lbv, ubv, obj = rc.shift_inputs()
    st = po.TrajectoryOptimizerState(lbv, ubv, H, replan_freq=2)
    torch.manual_seed(0)
    opt = lambda x0: po.cem_optimize(obj, x0, st.lower, st.upper, 2, 0.2, 20, 0.1, return_mean_elites=True)  # noqa: E731
    m = [st.step(opt), st.step(opt)]
    assert np.array_equal(ref["shift/1"].numpy(), m[0]) and np.array_equal(ref["shift/2"].numpy(), m[1])
    assert torch.equal(ref["shift/previous_solution"], st.previous_solution)


def test_spec_from_checkpoint_written_by_the_reference():
    """A checkpoint saved by the real OneDTransitionRewardModel.save loads into the ModelSpec of the model it was saved from."""
    import hipets

    om = rc.checkpoint_model()
    disk = hipets.spec_from_checkpoint(rc.CHECKPOINT_DIR, 17, 6)
    assert disk.members == [0, 1, 3, 4, 6] and disk.in_dim == 23
    for a, b in zip(disk.weights + disk.biases, om.weights + om.biases):
        assert torch.equal(a, b)
    assert torch.equal(disk.norm_mean, om.norm_mean) and disk.norm_mean.dtype == torch.float64
    assert torch.equal(disk.norm_std, om.norm_std)
    assert torch.equal(disk.min_logvar, om.min_logvar) and torch.equal(disk.max_logvar, om.max_logvar)


@pytest.mark.parametrize("sample", [False, True])
def test_oracle_step_bitwise_vs_reference_model_env_step(ref, sample):
    """ModelEnv.reset/step (model_env.py:62-140), the MBPO-style one-transition path."""
    om, obs0, act = rc.step_inputs()
    torch.manual_seed(5)
    gen = torch.Generator().manual_seed(2)
    x = torch.from_numpy(obs0.astype(np.float32))
    for i in (1, 2):
        perm = torch.randperm(40)
        eps = torch.empty(40, 11).normal_(0, 1, generator=gen) if sample else None
        x, r, d = po.step(om, x, act, perm=perm, eps=eps, sample=sample)
        assert torch.equal(ref[f"step/{sample}/next_obs_{i}"], x)
        assert torch.equal(ref[f"step/{sample}/reward_{i}"], r) and torch.equal(ref[f"step/{sample}/done_{i}"], d)


# ---- PlaNet latent planning path -------------------------------------------------------------
@pytest.mark.parametrize("P", rc.PLANET_P)
def test_planet_rollout_bitwise_vs_reference(ref, P):
    from oracle import planet_oracle as pl

    pm, latent0, belief0, actions, (lat, bel, act) = rc.planet_inputs()
    mine = pl.planet_rollout(pm, actions, latent0, belief0, P, generator=torch.Generator().manual_seed(5))
    assert torch.equal(ref[f"planet/{P}/returns"], mine)
    # one step, against PlaNetModel.sample directly (deterministic and sampled)
    for det in (True, False):
        o_lat, o_rew, o_bel = pl.planet_step(pm, lat, bel, act, generator=torch.Generator().manual_seed(8), deterministic=det)
        assert torch.equal(ref[f"planet/{P}/{det}/latent"], o_lat) and torch.equal(ref[f"planet/{P}/{det}/reward"], o_rew)
        assert torch.equal(ref[f"planet/{P}/{det}/belief"], o_bel)


def test_port_plan_equals_the_reference_plan_on_cfg2(ref):
    """bench.py's cpu_baseline times the oracle ("kind": "port").  On a full cfg2 plan (BASELINE.json configs[1]) the port returns
    bitwise the plan the UNMODIFIED reference classes (CEMOptimizer + ModelEnv.evaluate_action_sequences) returned."""
    c = rc.CFG2
    om, s0, lb, ub = rc.cfg2_inputs()
    gen = torch.Generator().manual_seed(0)
    obj = lambda a: po.rollout(om, a, s0, c["P"], global_rng=True, generator=gen)  # noqa: E731
    torch.manual_seed(5)
    p = po.cem_optimize(obj, torch.zeros(c["H"], c["act"]), torch.tensor(lb), torch.tensor(ub), c["iters"], 0.1, c["pop"], 0.1,
                        return_mean_elites=True)
    assert torch.equal(ref["cfg2_plan"], p)


def test_propagate_helpers_equal_the_reference(ref):
    """hipets.propagate* vs mbrl.util.math.propagate* (util/math.py:179-303), bitwise, same global-generator consumption."""
    import hipets

    preds, idx = rc.propagate_inputs()
    assert torch.equal(hipets.propagate_from_indices(preds[0], idx), ref["propagate/from_indices"])
    for method in rc.PROPAGATIONS:
        torch.manual_seed(3)
        mine = hipets.propagate(preds, method, idx)
        assert all(torch.equal(a, ref[f"propagate/{method}/{i}"]) for i, a in enumerate(mine)), method
    with pytest.raises(ValueError, match="Invalid propagation method"):
        hipets.propagate(preds, "nope")
