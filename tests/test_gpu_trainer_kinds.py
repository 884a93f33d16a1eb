"""hipets_train_steps_loss / hipets_train_eval_loss and hipets.ModelTrainer(..., extended=True) on the MI355X: the MSE loss of
deterministic models, and the NLL loss with per-member logvar bounds and the 1 / E gradient scale of a BasicEnsemble, against the
float64 / float32 restatements (tests/train_loss_restatement.py) by the suite's self-calibrated rule (|hip - f64| <= 4 |f32 - f64|
+ 1e-7, train_restatement.check) and against the reference ModelTrainer's recordings (tests/golden/trainerx_*.npz, written by
tests/make_trainer_loss_golden.py)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import hipets
import train_loss_restatement as tlr
import train_restatement as tr
from conftest import GOLDEN
from hipets import _lib
from hipets._pack import pack_train_desc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("trainerx_basic_nll", "trainerx_gmlp_mse", "trainerx_basic_mse")
E3, IN9, HID24, L3 = 3, 9, 24, 3


# ---- one step against the restatements ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 16, 33])
@pytest.mark.parametrize("out", [5, 17])
@pytest.mark.parametrize("act", ["silu", "relu", "tanh"])
@pytest.mark.parametrize("kind", ["mse", "nll"])
def test_one_step_matches_restatements(engine, kind, act, out, B):
    """E 3, in 9, hid 24: an out that is no multiple of 16 (and, under MSE, a last layer out and not 2 out wide), a ragged row tile
    (B 7, 33), one row, more than one row tile.  NLL runs with per-member bounds (member 1 clamps column 0) and grad_scale 1 / 3.
    Loss, grad_sq, every weight and bias and both moments by the self-calibrated rule; the float32 yardstick is taken in four
    summation orders (plain, rows reversed, rows reversed and network mirrored as in train_restatement.run_steps, and every
    contraction summed one product after the other), as train_restatement.check provides for quantities that float32 rounding
    decides.  Two kinds of them occur here.  After ONE Adam step a parameter moves by lr g / (|g| + 1e-8) whatever the size of
    g = dW + wd p: at nll-relu-17-33 one output-layer weight has dW = 8.763e-7 against wd p = -8.784e-7, a 5e-12 difference
    in the 33-term sum dW moves it by 3e-7, and torch's three blocked orders land 5.5e-8 from float64 there, the sequential
    order 3.4e-7, the kernel 3.3e-7.  And the MSE loss is a sum, so its loss and grad_sq are O(100) numbers whose last float32
    bit is far above the rule's 1e-7 floor."""
    scale = 1.0 / 3.0 if kind == "nll" else 1.0
    r = tlr.run_steps_kind(engine, kind, E3, B, IN9, HID24, out, L3, act, 1, grad_scale=scale, f32_orders=True)
    assert r["hip"][0][-1].shape[2] == (out if kind == "mse" else 2 * out)
    for k, what in ((4, "loss"), (5, "grad_sq")):
        tr.check(r["hip"][k], r["f32"][k], r["f64"][k], what, f32_others=(r["f32r"][k], r["f32m"][k], r["f32s"][k]))
    for li in range(L3):
        for j, p in ((0, "W"), (1, "b")):
            tr.check(r["hip"][j][li], r["f32"][j][li], r["f64"][j][li], f"{p}{li}", f32_others=(r["f32r"][j][li], r["f32m"][j][li], r["f32s"][j][li]))
            for k, nm in ((2, "m"), (3, "v")):
                tr.check(r["hip"][k][j][li], r["f32"][k][j][li], r["f64"][k][j][li], f"{nm} {p}{li}", f32_others=(r["f32r"][k][j][li], r["f32m"][k][j][li], r["f32s"][k][j][li]))


def test_member_bounds_and_grad_scale_are_read(engine):
    """What the one-step test pins is sensitive to the new arguments: against the float64 restatement with member 0's bounds for
    every member, the kernel's loss of member 1 (whose column 0 clamps) is off by far more than any rounding, and without the 1 / 3
    its grad_sq is 9x the kernel's."""
    r = tlr.run_steps_kind(engine, "nll", E3, 16, IN9, HID24, 5, L3, "silu", 1, grad_scale=1 / 3, restate=False)
    i = r["inputs"]
    sel = i["idx"][0].long()
    w, b, m, v = tr.fresh_state(i["ws"], i["bs"], torch.float64, "cpu")
    loss_shared, gsq_unscaled = tlr.train_step_kind("nll", w, b, m, v, i["x"][sel], i["y"][sel], i["lo"][:1], i["hi"][:1], "silu", 1, tr.LR, tr.WD)
    loss, gsq = r["hip"][4][0].double().cpu(), r["hip"][5][0].double().cpu()
    assert abs(loss[1] - loss_shared[1]).item() > 1e-2 and abs(loss[0] - loss_shared[0]).item() < 1e-5
    assert torch.allclose(gsq[0] * 9, gsq_unscaled[0], rtol=1e-4)


# ---- the old entry points are the new ones at (NLL, shared bounds, 1.0f) -------------------------------------------------------
def test_old_entry_points_equal_new_ones_bit_for_bit(engine):
    E, B, in_dim, hid, out, L, S, N = 5, 32, 8, 32, 6, 3, 20, 200
    g = torch.Generator().manual_seed(2)
    ws, bs = tr.random_model(E, in_dim, hid, out, L, 2)
    x, y = torch.randn(N, in_dim, generator=g).to(DEV), (torch.randn(N, out, generator=g) * 0.3).to(DEV)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:B] for _ in range(E)]) for _ in range(S)]).to(torch.int32).to(DEV)
    rows = torch.full((S,), B, dtype=torch.int32)
    rows[-1] = 11
    rows = rows.to(DEV)
    lo, hi = -10 * torch.ones(out, device=DEV), 0.5 * torch.ones(out, device=DEV)
    lo[0], hi[0] = -2.0, -1.0
    order = torch.randperm(N, generator=g).to(torch.int32).to(DEV)
    got = {}
    for which in ("old", "new"):
        w, b, m, v = tr.fresh_state(ws, bs, torch.float32, DEV)
        if which == "old":
            loss, gsq = engine.train_steps(w, b, m, v, lo, hi, x, y, idx, rows, 0, lr=tr.LR, weight_decay=tr.WD, activation="silu")
            score, rs = engine.train_eval(w, b, x, y, order, activation="silu", row_scores=True)
        else:
            d, keep = pack_train_desc(engine.device, w, b, "silu", 0.01, out, B, adam=(m[0], m[1], v[0], v[1], lo, hi, tr.LR, 0.9, 0.999, 1e-8, tr.WD, 0))
            loss, gsq = torch.empty(S, E, device=DEV), torch.empty(S, E, device=DEV)
            engine._call("hipets_train_steps_loss", d=d, x=x, y=y, n_rows=N, idx=idx, rows=rows, n_steps=S, step0=0, loss=loss, grad_sq=gsq,
                         loss_kind=_lib.TRAIN_LOSS["nll"], bounds_per_member=0, grad_scale=1.0)
            score, rs = torch.empty(E, device=DEV), torch.empty(E, N, device=DEV)
            engine._call("hipets_train_eval_loss", d=d, x=x, y=y, n_rows=N, order=order, score=score, row_score=rs, loss_kind=_lib.TRAIN_LOSS["nll"])
            del keep
        torch.cuda.synchronize()
        got[which] = [loss, gsq, score, rs] + w + b + m[0] + m[1] + v[0] + v[1]
    assert torch.isfinite(got["old"][0]).all() and len(got["old"]) == len(got["new"])
    for a, b_ in zip(got["old"], got["new"]):
        assert torch.equal(a, b_)


# ---- launch cuts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "nll"])
def test_launch_cuts_change_no_bit(engine, kind):
    """40 steps (the last one ragged) in launches of 1, of 7 and of the library's own choice: every result bit for bit the same."""
    scale = 1.0 / 3.0 if kind == "nll" else 1.0
    runs = [tlr.run_steps_kind(engine, kind, E3, 16, 6, 32, 5, 4, "silu", 40, N=150, steps_per_launch=spl, ragged_last=True, grad_scale=scale,
                               restate=False)["hip"] for spl in (1, 7, 0)]
    assert torch.isfinite(runs[0][4]).all() and not torch.equal(runs[0][4][0], runs[0][4][-1])
    for other in runs[1:]:
        assert torch.equal(runs[0][4], other[4]) and torch.equal(runs[0][5], other[5])
        for k in (0, 1):
            assert all(torch.equal(a, b) for a, b in zip(runs[0][k], other[k]))
        for k in (2, 3):
            assert all(torch.equal(a, b) for j in (0, 1) for a, b in zip(runs[0][k][j], other[k][j]))


# ---- evaluate under MSE ----------------------------------------------------------------------------------------------------------
def test_evaluate_mse_reads_an_out_wide_last_layer(engine):
    """E 3, out 17, N 70 (three row tiles, the last ragged) with an order permutation; the last layer's weights are random, so reading
    it with a row stride of 2 out instead of out gives another score."""
    E, in_dim, hid, out, L, N = 3, 9, 24, 17, 3, 70
    g = torch.Generator().manual_seed(4)
    ws, bs = tlr.random_model_kind("mse", E, in_dim, hid, out, L, 4)
    x = torch.randn(N, in_dim, generator=g, dtype=torch.float64)
    y = torch.randn(N, out, generator=g, dtype=torch.float64)
    ref = tr.eval_score(ws, bs, x, y, "silu")
    order = torch.randperm(N, generator=g).to(torch.int32)
    score, rs = engine.train_eval([w.float().to(DEV) for w in ws], [b.float().to(DEV) for b in bs], x.float().to(DEV), y.float().to(DEV),
                                  order.to(DEV), activation="silu", row_scores=True, loss="mse")
    assert torch.allclose(score.cpu().double(), ref, rtol=1e-5, atol=0)
    _, _, o = tr.forward(ws, bs, x[order.long()].unsqueeze(0).expand(E, -1, -1), "silu")
    assert o.shape[-1] == out
    ref_rows = ((o - y[order.long()]) ** 2).sum(-1)
    assert torch.allclose(rs.cpu().double(), ref_rows, rtol=1e-5, atol=1e-6)
    # what a row stride of 2 out would have read of the same [hid, out] weights (zeros past their end): another score
    flat = torch.cat([ws[-1].reshape(E, -1), torch.zeros(E, hid * out, dtype=torch.float64)], dim=1)
    misread = flat.reshape(E, hid, 2 * out)[:, :, :out]
    _, _, o_mis = tr.forward(ws[:-1] + [misread], bs, x[order.long()].unsqueeze(0).expand(E, -1, -1), "silu")
    assert not torch.allclose(ref, tr.eval_score(ws[:-1] + [misread], bs, x, y, "silu"), rtol=1e-5, atol=0)  # the bounds above tell them apart
    assert not torch.allclose(((o_mis - y[order.long()]) ** 2).sum(-1), ref_rows, rtol=1e-5, atol=1e-6)


# ---- full train() against the reference's recordings ---------------------------------------------------------------------------
def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return json.loads(bytes(z["meta_json"]).decode()), {k: z[k] for k in z.files if k != "meta_json"}


def _train(meta, arr, engine):
    mlp, model, train, val, rng = tlr.golden_setup(meta, arr)
    trainer = hipets.ModelTrainer(model, optim_lr=meta["lr"], weight_decay=meta["weight_decay"], engine=engine, extended=True)
    batches = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # a BasicEnsemble's set_elite warns
        losses, scores = trainer.train(train, val, num_epochs=meta["num_epochs"], patience=meta["patience"],
                                       batch_callback=lambda ep, l, m, mode: batches.append((ep, float(l), m.get("grad_norm"), mode)))
    return mlp, rng, losses, scores, [b for b in batches if b[3] == "train"]


def _weight_distance(mlp, meta, arr):
    ws, bs = tlr.stacked_params(mlp)
    return max(max(np.abs(ws[i].numpy() - arr[f"w1_{i}"]).max(), np.abs(bs[i].numpy() - arr[f"b1_{i}"]).max()) for i in range(meta["n_layers"]))


@pytest.mark.parametrize("name", KINDS)
def test_train_matches_reference_trainer(engine, name):
    """Epochs run, every batch's loss and grad_norm, per-epoch losses and validation scores, the RNG and the final weights in the live
    (member) parameters.  The final-weight bound is measured here: the float32 restatement of the same training in two summation
    orders (plain; mirrored network, reversed rows) lands 3e-8 .. 6e-8 from the recording's final weights, the kernel 3e-8 .. 7.5e-8 (DESIGN.md section 21
    lists the figures per recording); 10x the larger of the two distances is allowed, the margin tests/test_gpu_trainer.py took over its
    measured 2e-6."""
    meta, arr = _golden(name)
    measured = [_weight_distance(_train(meta, arr, tlr.CpuEngineKinds(mirrored=mirrored))[0], meta, arr) for mirrored in (False, True)]
    bound = 10 * max(measured)
    mlp, rng, losses, scores, tb = _train(meta, arr, engine)
    got = _weight_distance(mlp, meta, arr)
    print(f"{name}: final weights |f32 - golden| = {measured[0]:.3e} (plain), {measured[1]:.3e} (mirrored); |hip - golden| = {got:.3e}; bound {bound:.3e}")
    assert len(losses) == meta["epochs_run"]
    assert np.allclose(losses, arr["train_losses"], rtol=1e-4, atol=0)
    assert np.allclose(scores, arr["val_scores"], rtol=1e-4, atol=0)
    assert len(tb) == len(arr["batch_losses"])
    assert np.allclose([b[1] for b in tb], arr["batch_losses"], rtol=1e-4, atol=1e-6)
    assert np.allclose([b[2] for b in tb], arr["batch_grad_norms"], rtol=1e-3, atol=1e-9)
    assert json.dumps(rng.bit_generator.state, sort_keys=True) == json.dumps(json.loads(meta["rng_state_after"]), sort_keys=True)
    if meta["basic"]:
        assert mlp.elite_models is None
    else:
        assert sorted(int(i) for i in mlp.elite_models) == sorted(int(i) for i in arr["elites"])
    assert 0 < max(measured) < 1e-4 and got <= bound


# ---- a fused objective built on the same BasicEnsemble re-packs -------------------------------------------------------------------
def test_model_env_repacks_after_training_a_basic_ensemble(engine):
    """As test_model_env_repacks_after_train (tests/test_gpu_trainer.py), on a BasicEnsemble: the write-back copies member by member
    into the live parameters, their _version changes, and a fused eval fn built BEFORE train() returns what a freshly built one of
    the trained weights returns."""
    from test_gpu_trainer import _model_env

    E, obs_dim, act_dim, hid, L = 5, 6, 2, 32, 3

    def ensemble(ws, bs):
        mlp = tlr.TinyBasicEnsemble(E, obs_dim + act_dim, hid, obs_dim, L, act="silu")
        mlp.propagation_method = "expectation"
        tlr.load_params_kind(mlp, ws, bs)
        return mlp

    mlp = ensemble(*tr.random_model(E, obs_dim + act_dim, hid, obs_dim, L, 11, dtype=torch.float32))
    model = tr.TinyDynamicsModel(mlp)
    me = _model_env(model, obs_dim, act_dim)
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((300, obs_dim)).astype(np.float32)
    act = rng.uniform(-1, 1, (300, act_dim)).astype(np.float32)
    data = tr.Batch(obs=obs, act=act, next_obs=obs + 0.1 * rng.standard_normal(obs.shape).astype(np.float32))
    it = tr.BootstrapIterator(data, 32, E, shuffle_each_epoch=True, rng=rng)
    s0 = np.zeros(obs_dim, np.float32)
    actions = (torch.rand(10, 4, act_dim, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)

    def call(fn):
        torch.manual_seed(8)
        return fn(s0, actions).cpu()

    live_fn = hipets.make_eval_fn(me, 5, engine=engine, mode="exact", rng=torch.Generator().manual_seed(3))
    before = call(live_fn)
    v0 = hipets.model_version(me)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hipets.make_model_trainer(model, optim_lr=1e-2, engine=engine).train(it, num_epochs=2)
    assert hipets.model_version(me) != v0
    after = call(live_fn)
    fresh_fn = hipets.make_eval_fn(_model_env(tr.TinyDynamicsModel(ensemble(*tlr.stacked_params(mlp))), obs_dim, act_dim), 5,
                                   engine=hipets.Engine(DEV), mode="exact", rng=torch.Generator().manual_seed(3))
    call(fresh_fn)  # the live fn made one call before training: the same number of draws from its generator first
    fresh = call(fresh_fn)
    assert not torch.equal(before, after)
    assert torch.equal(after, fresh)


# ---- argument errors: nothing is launched ----------------------------------------------------------------------------------------
def test_bad_loss_arguments_are_refused(engine):
    E, out, L = 3, 4, 3
    ws, bs = tr.random_model(E, 5, 37, out, L, 0, dtype=torch.float32)
    w, b, m, v = tr.fresh_state(ws, bs, torch.float32, DEV)
    w0 = [t.clone() for t in w]
    lo, hi = -10 * torch.ones(out, device=DEV), 0.5 * torch.ones(out, device=DEV)
    x, y = torch.zeros(10, 5, device=DEV), torch.zeros(10, out, device=DEV)
    rows = torch.ones(1, dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, E, 4, dtype=torch.int32, device=DEV)
    loss, gsq = torch.full((1, E), -7.0, device=DEV), torch.full((1, E), -7.0, device=DEV)

    def steps(lo_, hi_, **kw):
        d, keep = pack_train_desc(engine.device, w, b, "silu", 0.01, out, 4, adam=(m[0], m[1], v[0], v[1], lo_, hi_, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0))
        args = dict(loss_kind=0, bounds_per_member=0, grad_scale=1.0)
        args.update(kw)
        with pytest.raises(hipets.HipetsError) as ei:
            engine._call("hipets_train_steps_loss", d=d, x=x, y=y, n_rows=10, idx=idx, rows=rows, n_steps=1, step0=0, loss=loss, grad_sq=gsq, **args)
        assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT, kw
        del keep

    steps(lo, hi, loss_kind=2)
    steps(lo, hi, loss_kind=-1)
    steps(lo, hi, grad_scale=0.0)
    steps(lo, hi, grad_scale=-0.5)
    steps(lo, hi, grad_scale=float("nan"))
    steps(lo, hi, grad_scale=float("inf"))
    steps(None, None)  # NULL bounds under NLL
    steps(lo, None)
    for bad in (dict(grad_scale=0.0), dict(grad_scale=float("nan"))):  # and through the keyword interface
        with pytest.raises(hipets.HipetsError) as ei:
            engine.train_steps(w, b, m, v, lo, hi, x, y, idx, rows, 0, lr=1e-3, **bad)
        assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        engine.train_steps(w, b, m, v, lo, hi, x, y, idx, rows, 0, lr=1e-3, loss="huber")
    d, keep = pack_train_desc(engine.device, w, b, "silu", 0.01, out, 1)
    with pytest.raises(hipets.HipetsError) as ei:
        engine._call("hipets_train_eval_loss", d=d, x=x, y=y, n_rows=10, order=None, score=torch.empty(E, device=DEV), row_score=None, loss_kind=5)
    assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(w, w0)) and (loss == -7.0).all() and (gsq == -7.0).all()  # nothing ran
