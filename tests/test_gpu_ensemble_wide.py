"""The wide form of hipets_ensemble_predict (csrc/ensemble_wide.hip; EnsemblePredictor(..., kernel="wide")) on the GPU.

Parity under the tile form's own rule and cases (tests/test_gpu_ensemble.py: per element within T1 x max(1, 4 u) of the float64
restatement; the references are that module's, computed once), and two shapes only the wide form distinguishes: an input so wide that a
workgroup owns 32 rows instead of 64, and a model for which the wide setting runs the tile form.  The other checks compare bits: a
row across batches, positions and requested outputs, a NaN row's neighbours, the default route around a wide call."""
import numpy as np
import pytest
import torch

import ensemble_restatement as er
import hipets
from test_gpu_ensemble import check, dev, reference

pytestmark = pytest.mark.gpu
EDGES = {  # in 448: 64 rows of it do not fit beside the hidden buffer; hid 1024 beside in 248: 32 rows do not either
    "wide_r2": dict(E=2, obs=440, act=8, hid=200, layers=3, activation="silu", learned=True, normalizer="none", rows=40),
    "wide_fallback": dict(E=2, obs=8, act=240, hid=1024, layers=3, activation="relu", learned=True, normalizer="none", rows=40),
}


def bits(t):
    return t.view(torch.int32)


def parity(engine, name):
    case, refs = reference(name)
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine, kernel="wide")
    obs, act = dev(case["obs"]), dev(case["act"])
    for elite, ((m64, l64, s64), f) in refs.items():
        mean, logvar = predictor.predict(obs, act, only_elite=elite)
        stats = predictor.uncertainty(obs, act, only_elite=elite)
        tag = f"wide {name} elite={elite}"
        assert mean.shape == m64.shape and stats.shape == (len(obs), 4)
        check(mean, m64, f["mean"], tag + " mean")
        if case["deterministic"]:
            s = stats.cpu().numpy()
            assert logvar is None and (s[:, 0] == 0).all() and np.array_equal(s[:, 2], s[:, 1])
        else:
            check(logvar, l64, f["logvar"], tag + " logvar")
        for k, stat in enumerate(er.STATS):
            check(stats[:, k], s64[:, k], f["stats"][k], f"{tag} {stat}")
    return case, predictor


@pytest.mark.parametrize("name", list(er.GPU_CASES))
def test_parity_with_the_float64_restatement(engine, name):
    parity(engine, name)


def test_a_wide_input_runs_two_row_tiles(engine, monkeypatch):
    monkeypatch.setitem(er.GPU_CASES, "wide_r2", EDGES["wide_r2"])
    _, predictor = parity(engine, "wide_r2")  # 40 rows: a full workgroup of 32 and a ragged one; four mean tiles per wave
    assert predictor.geometry(40) == predictor.geometry(1) == (2, 16 * 2 * 4 * (448 + 4 + 208 + 4 + 16))


def test_a_model_too_wide_for_two_row_tiles_runs_the_tile_form(engine, monkeypatch):
    monkeypatch.setitem(er.GPU_CASES, "wide_fallback", EDGES["wide_fallback"])
    case, predictor = parity(engine, "wide_fallback")
    obs, act = dev(case["obs"]), dev(case["act"])
    assert predictor.geometry(40) == engine.ensemble_geometry(40, kernel="tile") == (1, hipets._pack.ensemble_lds_bytes(248, 1024, 9, False, 3))
    for a, b in zip(engine.ensemble_predict(obs, act, stats=True, kernel="wide"), engine.ensemble_predict(obs, act, stats=True, kernel="tile")):
        assert torch.equal(bits(a), bits(b))


def test_rows_do_not_depend_on_batch_position_or_requested_outputs(engine):
    case, _ = reference("stock")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine, kernel="wide")
    obs, act = dev(case["obs"]), dev(case["act"])
    run = lambda o, a, **kw: engine.ensemble_predict(o, a, only_elite=True, kernel="wide", **kw)  # noqa: E731
    full = run(obs, act, stats=True)
    for B in (1, 65, 100):  # one row; the first row of a second workgroup as its only live one; a ragged workgroup's last live row
        assert predictor.geometry(B)[0] == 4
        for p, f in zip(run(obs[:B], act[:B], stats=True), full):
            assert torch.equal(bits(p), bits(f[:, :B] if f.ndim == 3 else f[:B]))
    tail = run(obs[990:].contiguous(), act[990:].contiguous(), stats=True)  # row 990 from place 30 of its workgroup to place 0
    assert torch.equal(bits(tail[0]), bits(full[0][:, 990:])) and torch.equal(bits(tail[2]), bits(full[2][990:]))
    alone = run(obs, act, mean=False, logvar=False, stats=True)  # the statistics alone: another kernel instance than all three
    assert alone[0] is None and alone[1] is None and torch.equal(bits(alone[2]), bits(full[2]))
    assert torch.equal(bits(run(obs, act)[0]), bits(full[0]))


def test_a_nan_row_stays_in_its_row(engine):
    case, _ = reference("small_silu")
    hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    obs, act = dev(case["obs"]), dev(case["act"])
    clean = engine.ensemble_predict(obs, act, stats=True, kernel="wide")
    bad = obs.clone()
    bad[5, 1] = float("nan")
    bad[37] = float("inf")
    dirty = engine.ensemble_predict(bad, act, stats=True, kernel="wide")
    keep = torch.ones(len(obs), dtype=torch.bool, device=obs.device)
    keep[[5, 37]] = False
    for c, d in zip(clean, dirty):
        rows = (lambda t: t[:, keep]) if c.ndim == 3 else (lambda t: t[keep])
        assert torch.equal(bits(rows(c)), bits(rows(d)))
    assert torch.isnan(dirty[0][:, 5]).all() and torch.isnan(dirty[2][5, 1:]).all()


def test_the_switch_keeps_its_setting_and_the_default_route_its_bits(engine):
    case, _ = reference("stock")
    hipets.EnsemblePredictor(er.case_spec(case), engine=engine)
    obs, act = dev(case["obs"][:100]), dev(case["act"][:100])
    before = engine.ensemble_predict(obs, act, stats=True)
    wide = engine.ensemble_predict(obs, act, stats=True, kernel="wide")  # set for the call and put back:
    assert engine.ensemble_kernel == "tile" and engine.ensemble_geometry(1)[0] == 1 and engine.ensemble_geometry(1, kernel="wide")[0] == 4
    assert not torch.equal(bits(wide[0]), bits(before[0]))  # (another summation order)
    for a, b in zip(before, engine.ensemble_predict(obs, act, stats=True)):
        assert torch.equal(bits(a), bits(b))
    engine.set_ensemble_kernel("wide")
    try:
        with pytest.raises(hipets.HipetsError, match="ensemble kernel") as exc:
            engine._query("hipets_set_ensemble_kernel", kind=7)
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT and engine.ensemble_geometry(1)[0] == 4  # refused, and still the wide form
        for a, b in zip(wide, engine.ensemble_predict(obs, act, stats=True)):
            assert torch.equal(bits(a), bits(b))
    finally:
        engine.set_ensemble_kernel("tile")
    with pytest.raises(ValueError, match="kernel"):
        hipets.EnsemblePredictor(er.case_spec(case), engine=engine, kernel="broad")


def test_penalised_populate_stores_the_wide_forms_penalty(engine):
    """One populate call with ensemble_kernel="wide" on the shape of tests/test_gpu_penalised_populate.py, staging path, against that
    module's numpy restatement of the loop over float64 statistics of the recorded steps.  The stored reward is fl(r - fl(c u)) with u
    within F x T1 of the float64 u64 (F: the parity rule's factor for this model), so it lies within c F (atol + rtol u64) + 2^-22 (|r| +
    c u64) of r - c u64; the halt threshold sits in the widest gap of the upper half of all steps' u64, which the test finds wider than
    four times the bound, so every flag is decided; rows, actions and next observations do not depend on the penalty: bit for bit."""
    import test_gpu_penalised_populate as tp

    spec, steps, coef = tp.model_spec(), tp.trajectory(engine), 0.5
    case = dict(weights=[w.numpy() for w in spec.weights], biases=[b.numpy() for b in spec.biases], activation=spec.activation, slope=spec.leaky_slope,
                deterministic=False, out_dim=spec.out_dim, E=spec.ensemble_size, elites=list(spec.members), min_logvar=spec.min_logvar.numpy(),
                max_logvar=spec.max_logvar.numpy())
    mu, sd = spec.norm_mean.double().numpy(), spec.norm_std.double().numpy()
    u64, factor = [], 1.0
    for obs, action, *_ in steps:
        x = (np.concatenate([obs, action], axis=1).astype(np.float64) - mu) / sd
        s64, s32 = er.ensemble_f64(case, x, True)[2][:, 1], er.ensemble_f32_torch(case, x.astype(np.float32), True)[2][:, 1]
        u64.append(s64)
        factor = max(factor, er.bound_factor(s32, s64))
    bound = lambda u: factor * (er.T1["atol"] + er.T1["rtol"] * np.abs(u))  # noqa: E731
    order = np.sort(np.concatenate(u64))[len(u64) * tp.N // 2:]  # (every step's rows meet the threshold)
    at = int(np.argmax(np.diff(order)))
    threshold = float(0.5 * (order[at] + order[at + 1]))
    assert min(np.abs(u - threshold).min() for u in u64) > 2 * bound(threshold), "no row's statistic may sit within the bound of the threshold"
    penalty = hipets.UncertaintyPenalty("disagreement", coef=coef, halt_threshold=threshold)
    wide64 = [s[:5] + ({True: np.stack([u] * 4, axis=1)},) for s, u in zip(steps, u64)]  # (the restatement reads column 1 of [B, 4])
    counts, want = tp.expected(wide64, penalty)
    got_counts, got = tp.populate(engine, False, uncertainty=penalty, ensemble_kernel="wide")
    assert got_counts == counts and 0 < counts[1] < tp.N
    tp.same([got[i] for i in (0, 1, 2, 4)], [want[i] for i in (0, 1, 2, 4)], "rows other than the reward")
    kept = keeps(wide64, penalty)
    plain, u_rows = (np.concatenate([a[k] for a, k in zip(arrays, kept)]) for arrays in ([s[3] for s in steps], u64))
    want_r = plain.astype(np.float64) - coef * u_rows
    err, lim = np.abs(got[3] - want_r), coef * bound(u_rows) + 2.0 ** -22 * (np.abs(plain) + coef * u_rows)
    print(f"stored rewards: largest share of the bound {float((err / lim).max()):.3f} (factor {factor:.2f})")
    assert (err <= lim).all()


def keeps(wide64, penalty):
    """the rows each step stores under `penalty` (mbpo.py:53-63): not done or halted before"""
    accum, out = np.zeros(len(wide64[0][0]), bool), []
    for (_, _, _, rew, done, stats) in wide64:
        out.append(~accum)
        accum = accum | (er.penalty_np(stats[True], penalty.stat, penalty.coef, rew, done, penalty.halt_threshold)[1] != 0)
    return out
