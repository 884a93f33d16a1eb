"""precision='bf16x3' (a SEPARATELY reported arithmetic mode, include/hipets.h HIPETS_PREC_BF16X3): the ensemble MLP's linear layers
with fp32 operands carried as three bf16 pieces and six exact partial products per product on v_mfma_f32_16x16x32_bf16, fp32
accumulate.  Its own parity evidence, against the SAME oracle and the SAME tolerances as the fp32-MFMA mode (T2: |err| <= 1e-4
max(1, |v|); one step: rtol 1e-5, atol 2e-6), plus the measured error against fp32 MFMA results."""
import numpy as np
import pytest
import torch

import hipets
from bf16_restatement import B3_TOO_WIDE, EDGE_CASES_B3, SEED, SID
from conftest import to_spec
from hipets.planning import _BoundObjective
from oracle import pets_oracle as po
from oracle import device_draws
from test_gpu_bf16 import REFUSED, assert_refused_then_accepted, edge_parity_line, edge_replay
from test_gpu_rollout import SIZES, _random_case, assert_returns_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (cfg1's shape -- one-tile workgroups only -- lost its bf16x3 instances in round 6's trim of the build: the mode runs R = 3 instances)
B3_CASES = [SIZES[0], SIZES[3], SIZES[4], (17, 6, 7, 5, 4, dict(ensemble_size=5, hid=200))]


@pytest.mark.parametrize("mode", ["fast", "device"])
@pytest.mark.parametrize("case", B3_CASES, ids=lambda c: f"obs{c[0]}_pop{c[2]}x{c[3]}_H{c[4]}")
def test_bf16x3_rollouts_replayed_through_the_oracle(engine, case, mode):
    """Stock synthetic weights: returns within T2 of the oracle.  What this comparison cannot see: on the small case (17, 6, 7, 5, 4)
    zeroing the last input row, the last hidden row of layer 1, the last mean column or the last log-variance column moves the oracle's
    returns by at most 3.0 / 1.9 / 0.01 / 0.00 x T2 (DEVICE; FAST 1.7 / 1.6 / 0.01 / 0.00) -- the reward reads state dim 0 alone.  Its
    gained variant, on which each of the four moves a return by >= 34 x T2, is EDGE_CASES_B3's A_pop7 below."""
    obs, act, pop, P, H, mkw = case
    om, actions, s0, _, _ = _random_case(obs, act, pop, P, H, **mkw)
    engine.set_model(to_spec(om, obs, act, precision="bf16x3"))
    seed, sid = 31, 4
    out = engine.rollout(actions.to(DEV), s0, P, mode=mode, seed=seed, stream_id=sid)
    eps = engine.fast_normals(H, pop * P, seed, sid).cpu()
    nwg, r = engine.fast_geometry(pop, P, H)  # (of the bf16x3 model: the row-tile counts that have a bf16x3 instance)
    tr = {}
    if mode == "device":
        ref = po.rollout(om, actions, s0, P, perms=engine.device_perms(H, pop * P, seed, sid).cpu(), eps=eps, trace=tr)
    else:
        sched = engine.fast_schedule(H, nwg, seed, sid).cpu()
        rows = torch.arange(pop * P)
        wg = device_draws.fast_row_workgroup(rows, P, r)
        ref = po.rollout(om, actions, s0, P, members=torch.stack([sched[t][wg].long() for t in range(H)]), eps=eps, trace=tr)
    keep = torch.ones(pop, dtype=torch.bool)
    if om.termination == "humanoid":
        # a termination threshold is a discontinuity: a row whose height lands within an ulp of 1.0 / 2.0 (termination_fns.py:88-95) ends
        # on one side in the oracle and may end on the other on the device.  Round 5's FAST row dealing put such a row into this case
        # (candidate 567, step 1: z = 2.0000002, re-derived on the CPU from oracle/device_draws.py); candidates with a row within 2e-5 of a
        # threshold are not compared -- a handful of 1036 (20 720 rows x 4 steps over a range of ~4)
        z = torch.stack([n[:, 0] for n in tr["next_obs"]])
        keep = ~(torch.minimum((z - 1.0).abs(), (z - 2.0).abs()) < 2e-5).any(0).view(pop, P).any(1)
        assert int((~keep).sum()) <= 8
    assert_returns_close(out.cpu()[keep], ref[keep])  # T2, the fp32 mode's own tolerance
    # against the fp32-MFMA kernel on the same draws (FAST: and the same geometry -- the member schedule is per workgroup, and the fp32
    # model is free to pick another row-tile count): the two arithmetic modes agree far inside T2
    engine.set_model(to_spec(om, obs, act))
    f32 = engine.rollout(actions.to(DEV), s0, P, mode=mode, seed=seed, stream_id=sid, rows_per_group=r if mode == "fast" else 0)
    err = ((out - f32).abs() / torch.clamp(f32.abs(), min=1.0)).cpu()[keep].max().item()
    assert err < 2e-5, err


def test_bf16x3_one_step_accuracy(engine):
    """One transition (H = 1: the return is the step's reward s'[0] - 0.1 |a|^2, i.e. one MLP evaluation + sampling) at the one-step
    tolerance T1 (rtol 1e-5, atol 2e-6).  At H = 1 the return sees output columns 0 (mean) and obs (log-variance) only: zeroing the last
    mean or log-variance column moves no return at all, the last input row moves one by 34 x T1 and the last hidden row of layer 1 by
    11 x (CPU, bf16_restatement.mutated).  The other output columns are the edge cases' business (EDGE_CASES_B3, H = 4)."""
    obs, act, pop, P = 17, 6, 500, 20
    om, actions, s0, _, _ = _random_case(obs, act, pop, P, 1, ensemble_size=5, hid=200)
    engine.set_model(to_spec(om, obs, act, precision="bf16x3"))
    out = engine.rollout(actions.to(DEV), s0, P, mode="device", seed=3, stream_id=1).cpu()
    ref = po.rollout(om, actions, s0, P, perms=engine.device_perms(1, pop * P, 3, 1).cpu(), eps=engine.fast_normals(1, pop * P, 3, 1).cpu())
    assert torch.allclose(out, ref, rtol=1e-5, atol=2e-6), float((out - ref).abs().max())


def test_bf16x3_fused_plan_equals_per_iteration_path_and_needs_a_specialised_shape(engine):
    obs, act, H, P, pop = 17, 6, 10, 5, 120
    om = po.make_synthetic_model(obs, act, ensemble_size=5, hid=200, seed=3)
    fn = hipets.make_eval_fn(to_spec(om, obs, act, precision="bf16x3"), P, engine=engine, seed=13, mode="device")
    obj = _BoundObjective(fn, (np.random.default_rng(1).standard_normal(obs) * 0.1).astype(np.float32))
    lb, ub = [[-1.0] * act] * H, [[1.0] * act] * H
    a = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    b = hipets.CEMOptimizer(4, 0.1, pop, lb, ub, 0.1, DEV, return_mean_elites=True, seed=21)
    x0 = torch.zeros(H, act)
    assert torch.equal(a.optimize(obj, x0=x0), b.optimize(obj, x0=x0, callback=lambda *_: None))
    # no instance for other shapes / calls: fails loudly, never falls back to another arithmetic
    om2 = po.make_synthetic_model(obs, act, ensemble_size=5, hid=64, seed=3)
    engine.set_model(to_spec(om2, obs, act, precision="bf16x3"))
    with pytest.raises(hipets.HipetsError, match="bf16x3"):
        engine.rollout(torch.zeros(40, 3, act, device=DEV), np.zeros(obs, np.float32), 5, mode="device")
    engine.set_model(to_spec(om, obs, act, precision="bf16x3"))
    with pytest.raises(hipets.HipetsError, match="bf16x3"):  # injected eps need the generic kernel
        engine.rollout(torch.zeros(40, 3, act, device=DEV), np.zeros(obs, np.float32), 5, mode="exact",
                       perms=torch.stack([torch.randperm(200) for _ in range(3)]).to(DEV), eps=torch.zeros(3, 200, obs, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------
# The edges of the two instance families (tests/bf16_restatement.py EDGE_CASES_B3; tests/test_bf16_host.py holds the CPU conditions
# of every case: each single-column loss moves a return by >= 4 x T2, the oracle's own summation order uses <= T2 / 4)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("case", EDGE_CASES_B3, ids=lambda c: c.name)
def test_bf16x3_edge_cases_replayed_through_the_oracle(engine, monkeypatch, case, mode):
    """|hip_i - oracle_i| <= 1e-4 max(1, |oracle_i|) (T2) for EVERY candidate, all values finite, the bf16x3 instance at three row
    tiles; and against the fp32-MFMA kernel on the same draws (FAST: the same row-tile count) err < 2e-5."""
    hip, ref, D, tol, om, actions, s0 = edge_replay(engine, monkeypatch, case, "bf16x3", mode)
    err = (hip - ref).abs()
    edge_parity_line("BF16X3_PARITY", case, "bf16x3", mode, err, D, tol)
    bad = err > tol
    assert not bad.any(), f"max |hip - oracle| {err.max():.3e} ({(err / tol).max():.2f} x T2) at candidate {int(bad.nonzero()[0])}"
    engine.set_model(to_spec(om, case.obs, case.act))
    f32 = engine.rollout(actions.to(DEV), s0, case.P, mode=mode, seed=SEED, stream_id=SID, rows_per_group=3 if mode == "fast" else 0).cpu()
    rel = ((hip - f32).abs() / torch.clamp(f32.abs(), min=1.0)).max().item()
    assert rel < 2e-5, rel


@pytest.mark.parametrize("name", list(REFUSED))
def test_bf16x3_refuses_models_next_to_its_families(engine, name):
    assert_refused_then_accepted(engine, "bf16x3", "bf16x3", *REFUSED[name])


@pytest.mark.parametrize("obs,act,mkw", B3_TOO_WIDE, ids=[f"obs{o}_act{a}" for o, a, _ in B3_TOO_WIDE])
def test_bf16x3_refuses_inputs_too_wide_for_three_row_tiles(engine, obs, act, mkw):
    """The mode's only instances run three row tiles, whose three-plane activation rows leave LDS for act_dim <= 64 (obs 24) / 55
    (obs 41): one column more, and the bf16 table's four- and five-chunk widths, raise."""
    assert_refused_then_accepted(engine, "bf16x3", "bf16x3", obs, act, {k: v for k, v in mkw.items() if k != "ensemble_size"})
