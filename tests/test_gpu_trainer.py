"""hipets.ModelTrainer / hipets_train_steps / hipets_train_eval on the MI355X against our float64 / float32 restatement
(tests/train_restatement.py) and against the reference ModelTrainer's recordings (tests/golden/trainer_*.npz, written by
tests/make_trainer_golden.py).  Tolerances are self-calibrated: the HIP result's distance from the float64 restatement may be
at most 4x the float32 restatement's own distance, plus a 1e-7 floor."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import hipets
import train_restatement as tr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, WD = tr.LR, tr.WD
_dist, _check, _state, _run = tr.dist, tr.check, tr.fresh_state, tr.run_steps  # shared with tests/test_gpu_trainer_edges.py


SHAPES = {  # (E, B, in, hid, out, n_layers)
    "pets_halfcheetah": (7, 32, 24, 200, 18, 5),
    "mbpo_halfcheetah": (7, 256, 23, 200, 18, 5),
    "humanoid_widths": (3, 32, 393, 200, 376, 5),
    "odd_hid37_in5_b17": (3, 17, 5, 37, 4, 3),
    "odd_b1": (2, 1, 5, 37, 4, 3),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("act", tr.ACTS)
def test_one_step_matches_restatement(engine, shape, act):
    E, B, in_dim, hid, out, L = SHAPES[shape]
    r = _run(engine, E, B, in_dim, hid, out, L, act, 1)
    for k, what in ((4, "loss"), (5, "grad_sq")):
        _check(r["hip"][k], r["f32"][k], r["f64"][k], what)
    # The gradient is pinned through the moments (m = (1 - b1)(g + wd p), v = (1 - b2)(g + wd p)^2 after one step) with the
    # self-calibrated rule.  The parameters are pinned to Adam's formula applied to the kernel's own moments: after ONE step
    # p moves by lr g / (|g| + eps / ...), which for a gradient that cancels to ~eps (a dead ReLU column's bias, a saturated
    # sigmoid) is anywhere in [-lr, lr] depending on the summation order -- a float32 restatement is no yardstick there.
    ws0, bs0 = tr.random_model(E, in_dim, hid, out, L, 0)
    bc2s = (1 - 0.999) ** 0.5
    for li in range(L):
        for k, nm in ((2, "m"), (3, "v")):
            _check(r["hip"][k][0][li], r["f32"][k][0][li], r["f64"][k][0][li], f"{nm} W{li}")
            _check(r["hip"][k][1][li], r["f32"][k][1][li], r["f64"][k][1][li], f"{nm} b{li}")
        for j, (p0, nm) in enumerate(((ws0[li], "W"), (bs0[li], "b"))):
            m, v = r["hip"][2][j][li].double().cpu(), r["hip"][3][j][li].double().cpu()
            expect = p0.float().double() - (LR / (1 - 0.9)) * m / (v.sqrt() / bc2s + 1e-8)
            got = r["hip"][j][li].double().cpu()
            assert (got - expect).abs().max().item() <= 1e-7, f"{nm}{li}: Adam step off its own moments"


def test_200_steps_across_small_launches(engine):
    """Chunks of 7 steps: launch boundaries fall mid-run (and a ragged last minibatch); losses and final params as the restatement."""
    r = _run(engine, 3, 16, 6, 32, 4, 4, "silu", 200, N=150, steps_per_launch=7, ragged_last=True)
    _check(r["hip"][4], r["f32"][4], r["f64"][4], "losses")
    for li in range(4):
        _check(r["hip"][0][li], r["f32"][0][li], r["f64"][0][li], f"W{li}")
        _check(r["hip"][1][li], r["f32"][1][li], r["f64"][1][li], f"b{li}")
    # and the launch geometry does not change a bit
    r2 = _run(engine, 3, 16, 6, 32, 4, 4, "silu", 200, N=150, steps_per_launch=0, ragged_last=True)
    assert torch.equal(r["hip"][4], r2["hip"][4]) and all(torch.equal(a, b) for a, b in zip(r["hip"][0], r2["hip"][0]))


@pytest.mark.parametrize("act", ["silu", "tanh"])
def test_evaluate_matches_restatement(engine, act):
    E, in_dim, hid, out, L, N = 5, 24, 200, 18, 5, 1037
    g = torch.Generator().manual_seed(4)
    ws, bs = tr.random_model(E, in_dim, hid, out, L, 4)
    x = torch.randn(N, in_dim, generator=g, dtype=torch.float64)
    y = torch.randn(N, out, generator=g, dtype=torch.float64)
    ref = tr.eval_score(ws, bs, x, y, act)
    order = torch.randperm(N, generator=g).to(torch.int32)
    score, rs = engine.train_eval([w.float().to(DEV) for w in ws], [b.float().to(DEV) for b in bs], x.float().to(DEV), y.float().to(DEV),
                                  order.to(DEV), activation=act, row_scores=True)
    assert torch.allclose(score.cpu().double(), ref, rtol=1e-5, atol=0)
    _, _, o = tr.forward(ws, bs, x[order.long()].unsqueeze(0).expand(E, -1, -1), act)
    ref_rows = ((o[..., :out] - y[order.long()]) ** 2).sum(-1)
    assert torch.allclose(rs.cpu().double(), ref_rows, rtol=1e-5, atol=1e-6)


# ---- full train() against the reference's recordings ---------------------------------------------------------------------
def _golden(path):
    z = np.load(path)
    meta = json.loads(bytes(z["meta_json"]).decode())
    return meta, {k: z[k] for k in z.files if k != "meta_json"}


def _setup(meta, arr, device="cpu"):
    E, L = meta["E"], meta["n_layers"]
    mlp = tr.TinyGaussianMLP(E, meta["in_dim"], meta["hid"], meta["out"], L, act=meta["act"])
    tr.load_params(mlp, [arr[f"w0_{i}"] for i in range(L)], [arr[f"b0_{i}"] for i in range(L)])
    model = tr.TinyDynamicsModel(mlp, num_elites=meta["num_elites"]).to(device)
    data = tr.Batch(obs=arr["obs"], act=arr["act"], next_obs=arr["next_obs"])
    rng = np.random.default_rng()
    rng.bit_generator.state = json.loads(meta["rng_state_after_split"])
    train = tr.BootstrapIterator(data[arr["train_rows"]], meta["batch_size"], E, shuffle_each_epoch=True, rng=rng,
                                 member_indices=arr["member_indices"])
    val = None
    if len(arr["val_rows"]):
        val = tr.TransitionIterator(data[arr["val_rows"]], meta["batch_size"], shuffle_each_epoch=False, rng=rng)
    return mlp, model, train, val, rng


TWO_CALLS = os.path.join(GOLDEN, "trainer_c_two_calls.npz")  # two train() calls of one trainer: its own layout and tests
GOLDENS = sorted(p for p in glob.glob(os.path.join(GOLDEN, "trainer_*.npz")) if p != TWO_CALLS)


def _setup_two_calls(meta, arr):
    """The model of tests/golden/trainer_c_two_calls.npz at its initial weights, and iterators(c) -> (train, val, rng) of call c:
    the reference's split and member indices of that call over the transitions stored by then, the RNG where the reference's
    stood after building them."""
    E, L = meta["E"], meta["n_layers"]
    mlp = tr.TinyGaussianMLP(E, meta["in_dim"], meta["hid"], meta["out"], L, act=meta["act"])
    tr.load_params(mlp, [arr[f"w0_{i}"] for i in range(L)], [arr[f"b0_{i}"] for i in range(L)])
    model = tr.TinyDynamicsModel(mlp, num_elites=meta["num_elites"])
    data = tr.Batch(obs=arr["obs"], act=arr["act"], next_obs=arr["next_obs"])

    def iterators(c):
        assert max(arr[f"c{c}_train_rows"].max(), arr[f"c{c}_val_rows"].max()) < meta["stored"][c]
        rng = np.random.default_rng()
        rng.bit_generator.state = json.loads(meta["calls"][c]["rng_state_after_split"])
        train = tr.BootstrapIterator(data[arr[f"c{c}_train_rows"]], meta["batch_size"], E, shuffle_each_epoch=True, rng=rng,
                                     member_indices=arr[f"c{c}_member_indices"])
        val = tr.TransitionIterator(data[arr[f"c{c}_val_rows"]], meta["batch_size"], shuffle_each_epoch=False, rng=rng)
        return train, val, rng

    return mlp, model, iterators


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p) for p in GOLDENS])
def test_train_matches_reference_trainer(engine, path):
    meta, arr = _golden(path)
    mlp, model, train, val, rng = _setup(meta, arr)
    trainer = hipets.ModelTrainer(model, optim_lr=meta["lr"], weight_decay=meta["weight_decay"], engine=engine)
    batches = []
    losses, scores = trainer.train(train, val, num_epochs=meta["num_epochs"], patience=meta["patience"],
                                   batch_callback=lambda ep, l, m, mode: batches.append((ep, float(l), m.get("grad_norm"), mode)))
    assert len(losses) == meta["epochs_run"]
    assert np.allclose(losses, arr["train_losses"], rtol=1e-4, atol=0)
    assert np.allclose(scores, arr["val_scores"], rtol=1e-4, atol=0)
    tb = [b for b in batches if b[3] == "train"]
    assert len(tb) == len(arr["batch_losses"])
    assert np.allclose([b[1] for b in tb], arr["batch_losses"], rtol=1e-4, atol=1e-6)
    assert np.allclose([b[2] for b in tb], arr["batch_grad_norms"], rtol=1e-3, atol=1e-9)
    assert sorted(int(i) for i in mlp.elite_models) == sorted(int(i) for i in arr["elites"])
    # final weights: 3 epochs of Adam at lr 1e-3 move a weight by <= ~lr per step; float32 rounding differences between two
    # summation orders grow through the trajectory to a few 1e-6 (measured ~2e-6): 2e-5 absolute is 10x that margin
    for i, lin in enumerate(mlp.layers()):
        assert np.abs(lin.weight.detach().numpy() - arr[f"w1_{i}"]).max() < 2e-5
        assert np.abs(lin.bias.detach().numpy() - arr[f"b1_{i}"]).max() < 2e-5
    assert json.dumps(rng.bit_generator.state, sort_keys=True) == json.dumps(json.loads(meta["rng_state_after"]), sort_keys=True)


@pytest.mark.parametrize("path", GOLDENS[:1], ids=[os.path.basename(p) for p in GOLDENS[:1]])
def test_adam_state_from_epoch_1_reproduces_epoch_2(engine, path):
    """load_state_dict with the reference optimizer's state after epoch 1 (step > 1 in the bias corrections), the weights after
    epoch 1 and the RNG at that point: one more epoch reproduces the reference's epoch-2 batch losses."""
    meta, arr = _golden(path)
    mlp, model, train, val, rng = _setup(meta, arr)
    L = meta["n_layers"]
    tr.load_params(mlp, [arr[f"we1_{i}"] for i in range(L)], [arr[f"be1_{i}"] for i in range(L)])
    rng.bit_generator.state = json.loads(meta["rng_state_epoch1"])
    trainer = hipets.ModelTrainer(model, optim_lr=meta["lr"], weight_decay=meta["weight_decay"], engine=engine)
    sd = trainer.optimizer.state_dict()
    n = len(sd["param_groups"][0]["params"])
    ref_sd = {"state": {int(k): {"step": torch.tensor(float(meta["adam_step_epoch1"])), "exp_avg": torch.from_numpy(arr[f"m_{k}"]),
                                 "exp_avg_sq": torch.from_numpy(arr[f"v_{k}"])} for k in meta["adam_state_keys"]},
              "param_groups": [dict(sd["param_groups"][0], params=list(range(n)))]}
    trainer.optimizer.load_state_dict(ref_sd)
    got = []
    trainer.train(train, None, num_epochs=1, evaluate=False, batch_callback=lambda ep, l, m, mode: got.append(l))
    nb = len(got)
    epoch2 = arr["batch_losses"][nb:2 * nb]
    assert np.allclose(got, epoch2, rtol=1e-4, atol=1e-6)


def _model_env(model, obs_dim, act_dim):
    from test_host_logic import _Space, halfcheetah, no_termination

    class _ME:
        pass

    me = _ME()
    me.dynamics_model = model
    model.input_normalizer, model.obs_process_fn, model.target_is_delta, model.no_delta_list, model.learned_rewards = None, None, True, [], False
    me.reward_fn, me.termination_fn = halfcheetah, no_termination
    me.observation_space, me.action_space = _Space(obs_dim), _Space(act_dim)
    return me


def test_model_env_repacks_after_train(engine):
    """After train(), a fused eval fn built BEFORE it on the same live model returns what a freshly built one of the trained
    weights returns (the write-back changes the parameters' _version, so the fn re-packs)."""
    E, obs_dim, act_dim, hid, L = 5, 6, 2, 32, 3
    mlp = tr.TinyGaussianMLP(E, obs_dim + act_dim, hid, obs_dim, L, act="silu")
    mlp.propagation_method = "expectation"
    ws, bs = tr.random_model(E, obs_dim + act_dim, hid, obs_dim, L, 11, dtype=torch.float32)
    tr.load_params(mlp, ws, bs)
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
    hipets.ModelTrainer(model, optim_lr=1e-2, engine=engine).train(it, num_epochs=2)
    assert hipets.model_version(me) != v0
    after = call(live_fn)
    mlp2 = tr.TinyGaussianMLP(E, obs_dim + act_dim, hid, obs_dim, L, act="silu")
    mlp2.propagation_method = "expectation"
    tr.load_params(mlp2, [l.weight.detach().clone() for l in mlp.layers()], [l.bias.detach().clone() for l in mlp.layers()])
    mlp2.set_elite(mlp.elite_models)
    fresh_fn = hipets.make_eval_fn(_model_env(tr.TinyDynamicsModel(mlp2), obs_dim, act_dim), 5, engine=hipets.Engine(DEV), mode="exact",
                                   rng=torch.Generator().manual_seed(3))
    call(fresh_fn)  # the live fn made one call before training: the same number of draws from its generator first
    fresh = call(fresh_fn)
    assert not torch.equal(before, after)
    assert torch.equal(after, fresh)


def test_bad_arguments_and_unsupported_models(engine):
    E, L = 3, 3
    ws, bs = tr.random_model(E, 5, 37, 4, L, 0, dtype=torch.float32)
    w, b, m, v = _state(ws, bs, torch.float32, DEV)
    lo, hi = -10 * torch.ones(4, device=DEV), 0.5 * torch.ones(4, device=DEV)
    x, y = torch.zeros(10, 5, device=DEV), torch.zeros(10, 4, device=DEV)
    rows = torch.ones(1, dtype=torch.int32, device=DEV)
    big = torch.zeros(1, E, 300, dtype=torch.int32, device=DEV)  # max_batch 300 > 256
    with pytest.raises(hipets.HipetsError) as ei:
        engine.train_steps(w, b, m, v, lo, hi, x, y, big, rows, 0, lr=1e-3)
    assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
    idx = torch.zeros(1, E, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(hipets.HipetsError) as ei:
        engine.train_steps(w, b, m, v, lo, hi, x, y, idx, rows, 0, lr=1e-3, betas=(1.5, 0.999))
    assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
    with pytest.raises(hipets.HipetsError) as ei:
        engine.train_steps(w, b, m, v, lo, hi, x, y, idx, rows, -1, lr=1e-3)
    assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
    for kw in (dict(deterministic=True), dict(learn_logvar_bounds=True), dict(act="silu")):
        mlp = tr.TinyGaussianMLP(E, 5, 37, 4, L, **{"act": "silu", **kw})
        if kw == dict(act="silu"):
            mlp.hidden_layers[0][1] = torch.nn.GELU()
        with pytest.raises(hipets.UnsupportedModelError, match="keep mbrl.models.ModelTrainer"):
            hipets.ModelTrainer(tr.TinyDynamicsModel(mlp), engine=engine)
    with pytest.raises(hipets.UnsupportedModelError):
        hipets.ModelTrainer(tr.TinyDynamicsModel(tr.TinyGaussianMLP(E, 5, 300, 4, L)), engine=engine)  # hid 300 > 256

    class _Basic(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.members = torch.nn.ModuleList([tr.TinyGaussianMLP(1, 5, 8, 4, 2)])

    class _DM:
        model = _Basic()

        def _process_batch(self, batch):
            raise AssertionError

    with pytest.raises(hipets.UnsupportedModelError, match="BasicEnsemble"):
        hipets.ModelTrainer(_DM(), engine=engine)
