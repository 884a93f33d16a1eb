"""The bf16 form of hipets_ensemble_predict (csrc/ensemble_bf16.hip; EnsemblePredictor(..., kernel="bf16")) on the GPU.

Parity against a float64 restatement of the form's stated arithmetic (include/hipets.h): the float32 model input; per linear layer both
operands rounded to bf16 nearest-even, matmul, bias and activation in float64, a hidden result cast to float32 before the next
rounding; clamps and statistics as tests/ensemble_restatement.py.  Per output tensor an element may differ by max(F (atol + rtol |ref|),
D): F the case's fp32 bound factor, D the largest |ref - fp32 float64 reference| of that tensor -- the bf16 error itself, because an
activation within a few fp32 ulps of a bf16 rounding boundary lands on the other side under another summation order.  The means must
also sit at least D / 2 from the fp32 reference somewhere: an fp32 route behind the name fails.  The other checks compare bits."""
import numpy as np
import pytest
import torch

import ensemble_restatement as er
import hipets
from bf16_restatement import bf16_rne_bits
from hipets.ensemble import ensemble_bf16_geometry
from test_gpu_ensemble import dev, reference

pytestmark = pytest.mark.gpu
EDGES = {  # one column in a second k chunk of the input and of the hidden layers; full chunks; eight hidden tiles per wave
    "bf16_in33_hid33": dict(E=2, obs=30, act=3, hid=33, layers=3, activation="silu", learned=True, normalizer="none", rows=40),
    "bf16_in32_hid64": dict(E=2, obs=24, act=8, hid=64, layers=3, activation="silu", learned=True, normalizer="none", rows=40),
    "bf16_hid1024": dict(E=2, obs=8, act=4, hid=1024, layers=3, activation="relu", learned=True, normalizer="none", rows=40),
}


def bits(t):
    return t.view(torch.int32)


def bf16_f64(case, x32, only_elite):
    """(mean, logvar | None, stats) of the bf16 form's arithmetic in float64 from the float32 model input"""
    members = er.member_list(case, only_elite)
    rnd = lambda a: np.asarray(bf16_rne_bits(np.asarray(a, np.float32)), np.float32).astype(np.float64)  # noqa: E731
    h = np.broadcast_to(np.asarray(x32, np.float32), (len(members),) + x32.shape)
    for l, (w, b) in enumerate(zip(case["weights"], case["biases"])):
        z = rnd(h) @ rnd(w[members]) + b[members].astype(np.float64)
        h = er._act_np(case["activation"], z, case["slope"]).astype(np.float32)
    out = case["out_dim"]
    if case["deterministic"]:
        return z, None, er.statistics_f64(z, None)
    lo, hi = er._bounds(case, members, np.float64)
    lv = hi - er._softplus64(hi - z[..., out:])
    lv = lo + er._softplus64(lv - lo)
    return z[..., :out], lv, er.statistics_f64(z[..., :out], lv)


def check(got, ref, f64, factor, what, told=False):
    got, D = got.cpu().numpy().astype(np.float64), float(np.abs(ref - f64).max())
    err, lim = np.abs(got - ref), np.maximum(factor * (er.T1["atol"] + er.T1["rtol"] * np.abs(ref)), D)
    print(f"{what}: largest share of the bound {float((err / lim).max()):.3f}, D {D:.3e}, max |got - fp32 reference| {float(np.abs(got - f64).max()):.3e}")
    assert (err <= lim).all(), (what, float((err / lim).max()))
    if told:
        assert np.abs(got - f64).max() >= D / 2, (what, "the result does not carry the bf16 rounding")


def parity(engine, name):
    case, refs = reference(name)
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine, kernel="bf16")
    obs, act = dev(case["obs"]), dev(case["act"])
    x32 = er.model_input(case, case["obs"], case["act"])
    for elite, ((m64, l64, s64), f) in refs.items():
        mb, lb, sb = bf16_f64(case, x32, elite)
        mean, logvar = predictor.predict(obs, act, only_elite=elite)
        stats = predictor.uncertainty(obs, act, only_elite=elite)
        tag = f"bf16 {name} elite={elite}"
        assert mean.shape == m64.shape and stats.shape == (len(obs), 4)
        check(mean, mb, m64, f["mean"], tag + " mean", told=True)
        if case["deterministic"]:
            s = stats.cpu().numpy()
            assert logvar is None and (s[:, 0] == 0).all() and np.array_equal(s[:, 2], s[:, 1])
        else:
            check(logvar, lb, l64, f["logvar"], tag + " logvar")
        for k, stat in enumerate(er.STATS):
            check(stats[:, k], sb[:, k], s64[:, k], f["stats"][k], f"{tag} {stat}")
    assert predictor.geometry(len(obs)) == predictor.geometry(1) == ensemble_bf16_geometry(case["in_dim"], case["hid"], case["out_dim"])[::3]


@pytest.mark.parametrize("name", list(er.GPU_CASES) + list(EDGES))
def test_parity_with_the_float64_restatement_of_the_bf16_arithmetic(engine, monkeypatch, name):
    if name in EDGES:
        monkeypatch.setitem(er.GPU_CASES, name, EDGES[name])
    parity(engine, name)


def test_rows_do_not_depend_on_batch_position_or_requested_outputs(engine):
    case, _ = reference("stock")
    predictor = hipets.EnsemblePredictor(er.case_spec(case), engine=engine, kernel="bf16")
    obs, act = dev(case["obs"]), dev(case["act"])
    run = lambda o, a, **kw: engine.ensemble_predict(o, a, only_elite=True, kernel="bf16", **kw)  # noqa: E731
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
    clean = engine.ensemble_predict(obs, act, stats=True, kernel="bf16")
    bad = obs.clone()
    bad[5, 1] = float("nan")
    bad[37] = float("inf")
    dirty = engine.ensemble_predict(bad, act, stats=True, kernel="bf16")
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
    low = engine.ensemble_predict(obs, act, stats=True, kernel="bf16")  # set for the call and put back:
    assert engine.ensemble_kernel == "tile" and engine.ensemble_geometry(1)[0] == 1 and engine.ensemble_geometry(1, kernel="bf16")[0] == 4
    assert not torch.equal(bits(low[0]), bits(before[0]))
    for a, b in zip(before, engine.ensemble_predict(obs, act, stats=True)):
        assert torch.equal(bits(a), bits(b))
    engine.set_ensemble_kernel("bf16")
    try:
        for a, b in zip(low, engine.ensemble_predict(obs, act, stats=True)):
            assert torch.equal(bits(a), bits(b))
    finally:
        engine.set_ensemble_kernel("tile")
    with pytest.raises(hipets.UnsupportedModelError):  # the fp32 snapshot is what the form reads: a bf16 spec stays refused
        hipets.EnsemblePredictor(er.case_spec(case, precision="bf16"), engine=engine, kernel="bf16")


def test_penalised_populate_stores_the_bf16_forms_penalty(engine):
    """One populate call with ensemble_kernel="bf16" on the shape of tests/test_gpu_penalised_populate.py, staging path, no halt: the
    stored rewards are the penalty's restatement on the predictor's own uncertainty() of the recorded steps, bit for bit; every other
    stored array is the unpenalised call's."""
    import test_gpu_penalised_populate as tp

    penalty = hipets.UncertaintyPenalty("disagreement", coef=0.5)
    predictor = hipets.EnsemblePredictor(tp.model_spec(), engine=engine, kernel="bf16")
    steps = [s[:5] + ({penalty.only_elite: predictor.uncertainty(dev(s[0]), dev(s[1]), only_elite=penalty.only_elite).cpu().numpy()},)
             for s in tp.trajectory(engine)]
    assert not np.array_equal(steps[0][5][penalty.only_elite], tp.trajectory(engine)[0][5][penalty.only_elite])  # (not the tile form's)
    counts, want = tp.expected(steps, penalty)
    got_counts, got = tp.populate(engine, False, uncertainty=penalty, ensemble_kernel="bf16")
    plain_counts, plain = tp.populate(engine, False)
    assert got_counts == counts == plain_counts
    tp.same(got, want, "bf16 penalty")
    tp.same([got[i] for i in (0, 1, 2, 4)], [plain[i] for i in (0, 1, 2, 4)], "rows other than the reward")
