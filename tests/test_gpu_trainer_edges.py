"""hipets_train_eval / hipets_train_steps / hipets.ModelTrainer at the shape limits, on every evaluate path and across the launch
cuts, against the float64 / float32 restatement (tests/train_restatement.py) and the reference trainer's recording of two train()
calls on a growing buffer (tests/golden/trainer_c_two_calls.npz).  The yardsticks are tests/test_gpu_trainer.py's: tr.check
(|hip - f64| <= 4 |f32 - f64| + 1e-7) for training, rtol 1e-5 (rows: + atol 1e-6) for evaluate; every case prints its distances."""
import functools
import json

import numpy as np
import pytest
import torch

import hipets
import train_restatement as tr
from test_gpu_trainer import TWO_CALLS, _golden, _setup_two_calls

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, WD = tr.LR, tr.WD


# ---- A. train_eval ---------------------------------------------------------------------------------------------------------
EVAL_ROWS = {  # (E, in, hid, out, n_layers, N, activation)
    "limits_e16_in512_hid256_out512": (16, 512, 256, 512, 3, 70, "silu"),  # every limit: 128 KB of dynamic LDS
    "humanoid_e3_in393_hid200_out376": (3, 393, 200, 376, 5, 70, "relu"),  # 100 KB
    "tiles257_hid37": (2, 5, 37, 4, 3, 8200, "sigmoid"),                   # the reduce kernel's strided loop takes a second trip
    "all_ones": (1, 1, 1, 1, 2, 1, "tanh"),
    "l8_n33": (2, 8, 16, 4, 8, 33, "leaky_relu"),                          # one full tile and one row
    "l2_n31": (2, 8, 16, 4, 2, 31, "silu"),                                # one partial tile
    "l2_n32": (2, 8, 16, 4, 2, 32, "silu"),                                # one exact tile
    "l2_n64": (2, 8, 16, 4, 2, 64, "silu"),                                # two exact tiles
}


@functools.lru_cache(maxsize=None)
def _eval_case(key):
    """The row's model and data (float64) and its restatement, computed once: scores [E] and row scores [E, N] in float64 and
    float32, dataset order."""
    E, in_dim, hid, out, L, N, act = EVAL_ROWS[key]
    g = torch.Generator().manual_seed(40 + sorted(EVAL_ROWS).index(key))
    ws, bs = tr.random_model(E, in_dim, hid, out, L, 4)
    x = torch.randn(N, in_dim, generator=g, dtype=torch.float64)
    y = torch.randn(N, out, generator=g, dtype=torch.float64)
    perm = torch.randperm(N, generator=g).to(torch.int32)
    ref = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        w, b, xd, yd = [t.to(dt) for t in ws], [t.to(dt) for t in bs], x.to(dt), y.to(dt)
        _, _, o = tr.forward(w, b, xd.unsqueeze(0).expand(E, -1, -1), act)
        ref[name] = (tr.eval_score(w, b, xd, yd, act), ((o[..., :out] - yd) ** 2).sum(-1))
    return ws, bs, x, y, perm, ref


def _rel(a, b):
    return ((a.double().cpu() - b.double()).abs() / b.double().abs()).max().item()


def _eval_checks(engine, key):
    E, in_dim, hid, out, L, N, act = EVAL_ROWS[key]
    ws, bs, x, y, perm, ref = _eval_case(key)
    w, b = [t.float().to(DEV) for t in ws], [t.float().to(DEV) for t in bs]
    xd, yd = x.float().to(DEV), y.float().to(DEV)
    got = {}
    for name, order in (("none", None), ("perm", perm.to(DEV)), ("arange", torch.arange(N, dtype=torch.int32, device=DEV))):
        score, rs = engine.train_eval(w, b, xd, yd, order, activation=act, row_scores=True)
        only = engine.train_eval(w, b, xd, yd, order, activation=act)  # the row_score == NULL path
        torch.cuda.synchronize()
        assert torch.equal(only, score), f"order={name}: score with and without row scores"
        got[name] = (score.cpu(), rs.cpu())
    ref_score, ref_rows = ref["f64"]
    print(f"{key}: score rel |hip - f64| = {_rel(got['none'][0], ref_score):.2e} (order None), {_rel(got['perm'][0], ref_score):.2e} "
          f"(permuted), |f32 - f64| = {_rel(ref['f32'][0], ref_score):.2e}; row scores abs |hip - f64| = "
          f"{tr.dist(got['none'][1], ref_rows):.2e}, |f32 - f64| = {tr.dist(ref['f32'][1], ref_rows):.2e}")
    for name, rows_ref in (("none", ref_rows), ("perm", ref_rows[:, perm.long()])):
        score, rs = got[name]
        assert torch.allclose(score.double(), ref_score, rtol=1e-5, atol=0), f"order={name}: score"
        assert torch.allclose(rs.double(), rows_ref, rtol=1e-5, atol=1e-6), f"order={name}: row scores"
    # a row's arithmetic depends neither on its tile nor on its place in the tile
    assert torch.equal(got["perm"][1], got["none"][1][:, perm.long()]), "row_scores(order=perm) != row_scores(order=None)[:, perm]"
    assert torch.equal(got["arange"][1], got["none"][1]) and torch.equal(got["arange"][0], got["none"][0]), "order=arange(N) != order=None"


def test_evaluate_widest_model_first_in_a_fresh_engine(engine):
    """The widest model (128 KB of dynamic LDS: the opt-in beyond the default 64 KB window) is a fresh engine's first evaluate
    launch, a narrow one follows it.  (The session's engine only says that there is a GPU.)"""
    eng = hipets.Engine(DEV)
    _eval_checks(eng, "limits_e16_in512_hid256_out512")
    _eval_checks(eng, "l2_n31")


@pytest.mark.parametrize("key", sorted(EVAL_ROWS))
def test_evaluate_matches_restatement_at_edges(engine, key):
    _eval_checks(engine, key)


def test_evaluate_order_entries_outside_the_dataset_score_zero(engine):
    """hipets.h (hipets_train_eval): an order entry outside [0, n_rows) contributes exactly zero to its row score and to the
    sum; the divisor of score stays n_rows * out_dim."""
    E, in_dim, hid, out, L, N, act = 2, 8, 16, 4, 2, 40, "silu"
    g = torch.Generator().manual_seed(9)
    ws, bs = tr.random_model(E, in_dim, hid, out, L, 4)
    x = torch.randn(N, in_dim, generator=g, dtype=torch.float64)
    y = torch.randn(N, out, generator=g, dtype=torch.float64)
    order = torch.randperm(N, generator=g).to(torch.int32)
    bad = [3, 31, 32, 39]  # in both tiles, the last (partial) tile's last row included
    order[bad] = torch.tensor([-1, N, 2 ** 31 - 1, -(2 ** 31)], dtype=torch.int32)
    keep = torch.ones(N, dtype=torch.bool)
    keep[bad] = False
    w, b = [t.float().to(DEV) for t in ws], [t.float().to(DEV) for t in bs]
    xd, yd = x.float().to(DEV), y.float().to(DEV)
    score, rs = engine.train_eval(w, b, xd, yd, order.to(DEV), activation=act, row_scores=True)
    _, rs_none = engine.train_eval(w, b, xd, yd, None, activation=act, row_scores=True)
    torch.cuda.synchronize()
    rs, rs_none = rs.cpu(), rs_none.cpu()
    assert (rs[:, bad] == 0).all()
    assert torch.equal(rs[:, keep], rs_none[:, order[keep].long()])
    _, _, o = tr.forward(ws, bs, x.unsqueeze(0).expand(E, -1, -1), act)
    ref_rows = ((o[..., :out] - y) ** 2).sum(-1)[:, order[keep].long()]
    ref_score = ref_rows.sum(1) / (N * out)
    print(f"outside order entries: score rel |hip - f64| = {_rel(score, ref_score):.2e}")
    assert torch.allclose(score.cpu().double(), ref_score, rtol=1e-5, atol=0)


# ---- B. train_steps --------------------------------------------------------------------------------------------------------
def _check_scaled(hip, f32, f64, what):
    """tr.check, and a bound that scales with the quantity.  Gradients shrink as 1 / (B out): at the limit shapes the first moments
    are ~1e-6 and the second ~1e-13, far below the rule's 1e-7 floor, which alone would let any value pass.  A misplaced tile, a
    wrong stride or a dropped k-block changes some element by about its own size, while float32 rounding of a contraction over
    K <= 512 terms stays below K 2^-24 = 3e-5 of the terms' absolute sum: 1 % of the tensor's largest float64 magnitude separates
    the two with two decades on either side."""
    tr.check(hip, f32, f64, what)
    d_hip, top = tr.dist(hip, f64), f64.abs().max().item()
    print(f"{what}: |hip - f64| / max |f64| = {d_hip / top:.2e}")
    assert d_hip <= 1e-2 * top, f"{what}: |hip - f64| = {d_hip:.3e} > 1 % of max |f64| = {top:.3e}"


def _one_step_checks(r, what="", shifted_biases=False):
    """The checks of test_gpu_trainer.test_one_step_matches_restatement: loss and grad_sq by the rule, the gradient through both
    moments by the rule, the parameters against Adam's formula applied to the kernel's own moments to 1e-7.  That absolute bound
    presumes parameters below ~1 (half a float32 ulp of the stored parameter is then <= 6e-8); the softplus cases shift biases to
    -22 / -30, where storing the parameter alone rounds by up to 2e-6: shifted_biases allows one float32 ulp of the parameter
    (2^-23 |p|) where that exceeds 1e-7."""
    for k, nm in ((4, "loss"), (5, "grad_sq")):
        _check_scaled(r["hip"][k], r["f32"][k], r["f64"][k], f"{what}{nm}")
    ws0, bs0 = r["inputs"]["ws"], r["inputs"]["bs"]
    bc2s = (1 - 0.999) ** 0.5
    for li in range(len(ws0)):
        for k, nm in ((2, "m"), (3, "v")):
            _check_scaled(r["hip"][k][0][li], r["f32"][k][0][li], r["f64"][k][0][li], f"{what}{nm} W{li}")
            _check_scaled(r["hip"][k][1][li], r["f32"][k][1][li], r["f64"][k][1][li], f"{what}{nm} b{li}")
        for j, (p0, nm) in enumerate(((ws0[li], "W"), (bs0[li], "b"))):
            m, v = r["hip"][2][j][li].double().cpu(), r["hip"][3][j][li].double().cpu()
            expect = p0.float().double() - (LR / (1 - 0.9)) * m / (v.sqrt() / bc2s + 1e-8)
            got = r["hip"][j][li].double().cpu()
            bound = torch.clamp(expect.abs() * 2.0 ** -23, min=1e-7) if shifted_biases else 1e-7
            assert ((got - expect).abs() <= bound).all(), f"{what}{nm}{li}: Adam step off its own moments"


def _flat(r):
    """Every tensor of a run's "hip" result, for bitwise comparisons."""
    w, b, m, v, loss, gsq = r["hip"]
    return list(w) + list(b) + list(m[0]) + list(m[1]) + list(v[0]) + list(v[1]) + [loss, gsq]


def _same_bits(r1, r2):
    return all(torch.equal(a, b) for a, b in zip(_flat(r1), _flat(r2)))


LIMITS = (16, 256, 512, 256, 512, 3, "silu")  # E, B, in, hid, out, n_layers: the largest slab and slab stride, every tile full
_limit_runs = {}


def _limit_run(engine):
    if "r" not in _limit_runs:
        _limit_runs["r"] = tr.run_steps(engine, *LIMITS, 1)
    return _limit_runs["r"]


def test_one_step_at_every_limit(engine):
    _one_step_checks(_limit_run(engine))


@pytest.mark.parametrize("e", [0, 15])
def test_member_of_the_limit_case_equals_a_one_member_call(engine, e):
    """Members never communicate: member e of the E 16 call is, bit for bit, an E 1 call on its parameters and its rows."""
    r = _limit_run(engine)
    i = r["inputs"]
    w, b, m, v = tr.fresh_state([t[e:e + 1] for t in i["ws"]], [t[e:e + 1] for t in i["bs"]], torch.float32, DEV)
    loss, gsq = engine.train_steps(w, b, m, v, i["lo"].float().reshape(-1).to(DEV), i["hi"].float().reshape(-1).to(DEV), i["x"].float().to(DEV),
                                   i["y"].float().to(DEV), i["idx"][:, e:e + 1].contiguous().to(DEV), i["rows"].to(DEV), 0, lr=LR, weight_decay=WD,
                                   activation=LIMITS[-1])
    torch.cuda.synchronize()
    one = list(w) + list(b) + list(m[0]) + list(m[1]) + list(v[0]) + list(v[1])
    full = _flat(r)
    assert torch.equal(loss[:, 0], full[-2][:, e]) and torch.equal(gsq[:, 0], full[-1][:, e])
    assert all(torch.equal(a[0], f[e]) for a, f in zip(one, full[:-2]))


@pytest.mark.parametrize("shape", [(2, 16, 8, 16, 4, 8), (2, 16, 8, 16, 4, 2), (1, 1, 1, 1, 1, 2)], ids=["l8", "l2", "all_ones"])
def test_one_step_at_the_small_limits(engine, shape):
    _one_step_checks(tr.run_steps(engine, *shape, "silu", 1))


@pytest.mark.parametrize("B", [3, 16, 20])
def test_one_step_k_tail_sweep(engine, B):
    """hid is the K of the forward products of layers 1, 2 and of the dA product of layer 1, B the K of every dW product: 4 / 12 /
    15 / 16 / 17 / 28 and 3 / 16 / 20 take every combination of mm_tile's three loops (blocks of 16, of 8, the guarded blocks of 4)."""
    for hid in (4, 12, 15, 16, 17, 28):
        _one_step_checks(tr.run_steps(engine, 2, B, 5, hid, 3, 3, "silu", 1), f"hid {hid} B {B}: ")


def _softplus_arguments(r, act):
    """u = max_logvar - raw and w = logvar - min_logvar of the NLL tail (both softplus arguments) at the initial parameters, float64."""
    i = r["inputs"]
    sel = i["idx"][0, :, :int(i["rows"][0])].long()
    _, _, o = tr.forward(i["ws"], i["bs"], i["x"][sel], act)
    out = i["y"].shape[1]
    u = i["hi"] - o[..., out:]
    return u, (i["hi"] - tr.softplus(u)) - i["lo"]


SOFTPLUS_SHAPE = (3, 32, 24, 200, 18, 5, "silu")


def test_saturated_softplus_both_branches(engine):
    """Output-layer logvar biases of columns 1..5 shifted by -30 (u > 20: softplus(u) = u, gradient factor 1) and min_logvar of
    the last column at -25 (w > 20 there); measured on the CPU: 28 % of the elements take u > 20, 5.6 % w > 20."""
    out = SOFTPLUS_SHAPE[4]

    def params(ws, bs):
        bs[-1][:, 0, out + 1:out + 6] -= 30.0

    def bounds(lo, hi):
        lo[0, -1] = -25.0

    r = tr.run_steps(engine, *SOFTPLUS_SHAPE, 1, edit_params=params, bounds=bounds)
    u, w = _softplus_arguments(r, "silu")
    print(f"softplus (a): u > 20 in {(u > 20).double().mean().item():.3f}, w > 20 in {(w > 20).double().mean().item():.3f} of the elements")
    assert (u > 20).any() and (u <= 20).any() and (w > 20).any() and (w <= 20).any()
    assert all(torch.isfinite(t).all() for t in r["f32"][4:6])
    _one_step_checks(r, "softplus (a): ", shifted_biases=True)


def test_saturated_softplus_unattenuated_gradient(engine):
    """One logvar column shifted by -22 with its min_logvar at -25: u > 20 with w ~ 3, so the gradient factor 1 of the saturated
    branch reaches the weights unattenuated (inverse variance ~ e^22: loss ~ 1e8, finite in float32)."""
    out, col = SOFTPLUS_SHAPE[4], 2

    def params(ws, bs):
        bs[-1][:, 0, out + col] -= 22.0

    def bounds(lo, hi):
        lo[0, col] = -25.0

    r = tr.run_steps(engine, *SOFTPLUS_SHAPE, 1, edit_params=params, bounds=bounds)
    u, w = _softplus_arguments(r, "silu")
    assert (u[..., col] > 20).all() and (w[..., col] < 20).all() and (w[..., col] > 0).all()
    print(f"softplus (b): loss {r['f64'][4].max().item():.3e}, grad_sq {r['f64'][5].max().item():.3e}")
    assert all(torch.isfinite(t).all() for t in r["f32"][4:6]) and all(torch.isfinite(t).all() for t in r["f32"][0])
    _one_step_checks(r, "softplus (b): ", shifted_biases=True)


def _multi_step_checks(r, what=""):
    others = [r[k] for k in ("f32r", "f32m") if k in r]  # further float32 summation orders, where the run made them (tr.check)
    tr.check(r["hip"][4], r["f32"][4], r["f64"][4], f"{what}losses", [o[4] for o in others])
    for li in range(len(r["hip"][0])):
        tr.check(r["hip"][0][li], r["f32"][0][li], r["f64"][0][li], f"{what}W{li}", [o[0][li] for o in others])
        tr.check(r["hip"][1][li], r["f32"][1][li], r["f64"][1][li], f"{what}b{li}", [o[1][li] for o in others])


ODD = (3, 17, 5, 37, 4, 3, "silu")


def test_indices_outside_the_dataset_read_zeros(engine):
    """hipets.h (hipets_train_steps): an index outside [0, n_rows) reads zeros.  The restatement runs on a row of zeros in those
    slots; a second run gives the same bits (nothing else was read)."""
    N = 64

    def edit(idx):
        idx[0, 0, 0], idx[0, 1, 5], idx[0, 1, 16] = -1, N, 2 ** 31 - 1
        idx[1, 2, 16], idx[1, 2, 0] = N, -(2 ** 31)
        idx[2, :, 3] = -1

    r = tr.run_steps(engine, *ODD, 3, N=N, edit_idx=edit)
    assert ((r["inputs"]["idx"] < 0) | (r["inputs"]["idx"] >= N)).sum().item() == 8
    _multi_step_checks(r, "outside idx: ")
    assert _same_bits(r, tr.run_steps(engine, *ODD, 3, N=N, edit_idx=edit, restate=False))


def test_ragged_steps_in_the_middle_of_a_launch(engine):
    """A short minibatch followed by a full one inside one launch: the rows the short step left in the slab are not read."""
    B = ODD[1]
    rows = [B, B // 3, B, 1, B]
    r = tr.run_steps(engine, *ODD, None, rows=rows, steps_per_launch=0)
    _multi_step_checks(r, "ragged middle: ")
    assert _same_bits(r, tr.run_steps(engine, *ODD, None, rows=rows, steps_per_launch=1, restate=False))


def test_300_steps_across_the_256_step_launch_cap(engine):
    """More steps than one launch's Adam scalars hold (256): the library's own chunk, a request above the cap, chunks of 7 and
    of 1, and two calls (123 steps, then 177 with step0 = 123) give the same bits; one of them is the restatement's trajectory."""
    shape = (3, 16, 6, 32, 4, 4, "silu", 300)
    r = tr.run_steps(engine, *shape, N=150, steps_per_launch=0, ragged_last=True)
    _multi_step_checks(r, "300 steps: ")
    for spl in (1000, 7, 1):
        assert _same_bits(r, tr.run_steps(engine, *shape, N=150, steps_per_launch=spl, ragged_last=True, restate=False)), f"steps_per_launch={spl}"
    assert _same_bits(r, tr.run_steps(engine, *shape, N=150, ragged_last=True, calls=[123, 177], restate=False)), "two calls"


def test_20_steps_at_a_shipped_width(engine):
    """Twenty steps at the shipped width (the one-step tests' pets_halfcheetah shape), losses and final parameters by the rule.

    With the plain float32 restatement alone this case missed the rule narrowly on ONE tensor, the first layer's bias: |hip - f64|
    = 1.23e-6 against 4 x 1.11e-7 + 1e-7 (rows reversed: 9.6e-8) on one host CPU, while another host's float32 restatement of the
    same run lay 9.9e-7 from float64 (rows reversed 1.05e-6, mirrored 7.7e-7).  The whole distance is one element of 1400 (member 4,
    unit 96): its first-step gradient cancels to 1.0e-6 (float64) where its later ones are 5e-5 .. 3e-3, so float32 rounding of that
    first sum sets Adam's v for the element and with it every later step's size.  So the run makes two further float32 restatements
    in other summation orders (run_steps f32_orders); the mirrored one lies 1.49e-6 from float64 at that same element on the host
    where the plain one lies 1.11e-7: the float32 orders differ among themselves by more than the rule allows, and tr.check then
    measures the HIP result against the largest of their distances (1.23e-6 <= 4 x 1.49e-6 + 1e-7).  Every other tensor passes
    against the plain restatement."""
    _multi_step_checks(tr.run_steps(engine, 7, 32, 24, 200, 18, 5, "silu", 20, N=400, f32_orders=True), "20 steps, width 200: ")


# ---- C. ModelTrainer ---------------------------------------------------------------------------------------------------------
def _small_model():
    """The model and data of test_gpu_trainer.test_model_env_repacks_after_train."""
    E, obs_dim, act_dim, hid, L = 5, 6, 2, 32, 3
    mlp = tr.TinyGaussianMLP(E, obs_dim + act_dim, hid, obs_dim, L, act="silu")
    ws, bs = tr.random_model(E, obs_dim + act_dim, hid, obs_dim, L, 11, dtype=torch.float32)
    tr.load_params(mlp, ws, bs)
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((300, obs_dim)).astype(np.float32)
    act = rng.uniform(-1, 1, (300, act_dim)).astype(np.float32)
    data = tr.Batch(obs=obs, act=act, next_obs=obs + 0.1 * rng.standard_normal(obs.shape).astype(np.float32))
    return mlp, tr.TinyDynamicsModel(mlp), data


def _train(engine, make_dataset, **kw):
    mlp, model, data = _small_model()
    batches = []
    trainer = hipets.ModelTrainer(model, optim_lr=1e-2, engine=engine)
    losses, scores = trainer.train(make_dataset(data), num_epochs=2, batch_callback=lambda ep, l, m, mode: batches.append((ep, float(l), m.get("grad_norm"), mode)),
                                   **kw)
    return losses, scores, batches, [l.weight.detach().clone() for l in mlp.layers()] + [l.bias.detach().clone() for l in mlp.layers()], trainer


def test_train_on_a_list_of_2d_batches_equals_the_transition_iterator(engine):
    """Any other iterable (here a list), 2-D batches: every member trains on the batch's rows, as on a TransitionIterator over the
    same rows in the same order; the evaluation passes (on the list, too) give the same bits."""
    as_list = _train(engine, lambda data: [data[i:i + 32] for i in range(0, len(data), 32)])
    as_iter = _train(engine, lambda data: tr.TransitionIterator(data, 32, shuffle_each_epoch=False))
    assert len(as_list[2]) == len(as_iter[2]) == 2 * 2 * 10  # 2 epochs x (10 train + 10 eval batches), the last of 12 rows
    assert as_list[0] == as_iter[0] and as_list[1] == as_iter[1] and as_list[2] == as_iter[2]
    assert all(torch.equal(a, b) for a, b in zip(as_list[3], as_iter[3]))
    assert as_list[4]._step == as_iter[4]._step == 20


def test_train_on_a_list_of_3d_batches_equals_the_bootstrap_iterator(engine):
    """[E, B, .] batches: member e trains on its own rows, as on a BootstrapIterator with the same member indices."""
    mi = np.stack([np.random.default_rng(5).permutation(300) for _ in range(5)])
    mi[1] = np.random.default_rng(6).integers(0, 300, 300)  # one member bootstrapped with replacement

    def boot(data):
        return tr.BootstrapIterator(data, 32, 5, shuffle_each_epoch=False, member_indices=mi)

    as_list = _train(engine, lambda data: list(boot(data)), evaluate=False)
    as_iter = _train(engine, boot, evaluate=False)
    assert len(as_list[2]) == len(as_iter[2]) == 2 * 10
    assert as_list[0] == as_iter[0] and as_list[2] == as_iter[2]
    assert all(torch.equal(a, b) for a, b in zip(as_list[3], as_iter[3]))


def test_evaluate_on_a_list_equals_the_iterator_and_rejects_3d_batches(engine):
    mlp, model, data = _small_model()
    trainer = hipets.ModelTrainer(model, engine=engine)
    got = {}
    for name, ds in (("list", [data[i:i + 32] for i in range(0, len(data), 32)]), ("iter", tr.TransitionIterator(data, 32, shuffle_each_epoch=False))):
        cb = []
        score = trainer.evaluate(ds, batch_callback=lambda s, m, mode: cb.append((float(s), mode)))
        got[name] = (score, cb, trainer.evaluate(ds))
    assert torch.equal(got["list"][0], got["iter"][0]) and torch.equal(got["list"][2], got["iter"][2]) and torch.equal(got["list"][0], got["list"][2])
    assert got["list"][1] == got["iter"][1] and len(got["list"][1]) == 10
    with pytest.raises(hipets.UnsupportedModelError):
        trainer.evaluate(list(tr.BootstrapIterator(data, 32, 5, shuffle_each_epoch=False, rng=np.random.default_rng(1))))


def test_two_train_calls_on_a_growing_buffer_match_reference_trainer(engine):
    """One trainer, as pets.train keeps it: 2 epochs on 300 stored transitions, then new iterators over 517 and 2 more epochs.
    Adam's moments and step count carry over, the second call's dataset and slab replace the first's.  Against the reference
    trainer's recording, with the tolerances of test_gpu_trainer.test_train_matches_reference_trainer."""
    meta, arr = _golden(TWO_CALLS)
    mlp, model, iterators = _setup_two_calls(meta, arr)
    trainer = hipets.ModelTrainer(model, optim_lr=meta["lr"], weight_decay=meta["weight_decay"], engine=engine)
    for c, m in enumerate(meta["calls"]):
        train, val, rng = iterators(c)
        batches = []
        losses, scores = trainer.train(train, val, num_epochs=meta["num_epochs"], patience=meta["patience"],
                                       batch_callback=lambda ep, l, mm, mode: batches.append((ep, float(l), mm.get("grad_norm"), mode)))
        assert len(losses) == m["epochs_run"]
        assert np.allclose(losses, arr[f"c{c}_train_losses"], rtol=1e-4, atol=0)
        assert np.allclose(scores, arr[f"c{c}_val_scores"], rtol=1e-4, atol=0)
        tb = [b for b in batches if b[3] == "train"]
        assert len(tb) == len(arr[f"c{c}_batch_losses"])
        print(f"call {c}: batch loss rel distance {np.abs(np.array([b[1] for b in tb]) / arr[f'c{c}_batch_losses'] - 1).max():.2e}, final weights abs "
              f"{max(np.abs(lin.weight.detach().numpy() - arr[f'c{c}_w1_{i}']).max() for i, lin in enumerate(mlp.layers())):.2e}")
        assert np.allclose([b[1] for b in tb], arr[f"c{c}_batch_losses"], rtol=1e-4, atol=1e-6)
        assert np.allclose([b[2] for b in tb], arr[f"c{c}_batch_grad_norms"], rtol=1e-3, atol=1e-9)
        assert sorted(int(i) for i in mlp.elite_models) == sorted(int(i) for i in arr[f"c{c}_elites"])
        for i, lin in enumerate(mlp.layers()):
            assert np.abs(lin.weight.detach().numpy() - arr[f"c{c}_w1_{i}"]).max() < 2e-5
            assert np.abs(lin.bias.detach().numpy() - arr[f"c{c}_b1_{i}"]).max() < 2e-5
        assert json.dumps(rng.bit_generator.state, sort_keys=True) == json.dumps(json.loads(m["rng_state_after"]), sort_keys=True)
    assert float(next(iter(trainer.optimizer.state_dict()["state"].values()))["step"]) == meta["adam_step"]
