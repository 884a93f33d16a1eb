"""The wide training step and evaluate pass (Engine.train_steps(kernel="wide"), Engine.train_eval(kernel="wide"),
hipets.ModelTrainer(step_kernel="wide"); csrc/train_wide.hip) on the MI355X against the float64 / float32 restatement
(tests/train_restatement.py), by the suite's self-calibrated rule: |hip - f64| <= 4 |f32 - f64| + 1e-7 (tr.check).  The checks are
those of the member and split kernels' tests (test_gpu_trainer_edges, test_gpu_trainer_split)."""
import numpy as np
import pytest
import torch

import hipets
import train_restatement as tr
from test_gpu_trainer_edges import _multi_step_checks, _one_step_checks, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Wide:
    """the engine with every train_steps call on the wide kernels (tr.run_steps passes no keyword through)"""

    def __init__(self, engine):
        self.train_steps = lambda *a, **kw: engine.train_steps(*a, kernel="wide", **kw)


class _CpuEngine(tr.CpuEngine):  # (the restatement has one way to run a step and one to evaluate)
    def train_steps(self, *a, kernel="member", **kw):
        return super().train_steps(*a, **kw)

    def train_eval(self, *a, kernel="tile", **kw):
        return super().train_eval(*a, **kw)


# (E, B, in, hid, out, n_layers, activation): one row, one column past the old limit, K = 1 mod 4, 17 column tiles over 8 waves; a second
# row block of one row; fewer column tiles than waves; batches past 256; the batch limit; mbpo_halfcheetah; every limit at once (the
# 131 KB panel, 1024 output columns); either side of the boundary between the two compiled instances (results up to 512 / 1024 wide)
ONE_STEP = [(2, 1, 5, 257, 4, 3, "silu"), (3, 33, 5, 300, 4, 3, "relu"), (3, 31, 5, 37, 4, 3, "leaky_relu"), (2, 257, 5, 272, 4, 3, "tanh"),
            (2, 1024, 5, 272, 4, 3, "sigmoid"), (7, 256, 23, 200, 18, 5, "silu"), (2, 40, 512, 1024, 512, 3, "silu"),
            (2, 33, 5, 512, 4, 3, "silu"), (2, 33, 5, 513, 4, 3, "silu")]
TWENTY = (3, 40, 6, 272, 4, 4, "silu")


@pytest.mark.parametrize("shape", ONE_STEP, ids=lambda s: "e{}_b{}_in{}_hid{}_out{}_l{}_{}".format(*s))
def test_one_step_matches_restatement(engine, shape):
    _one_step_checks(tr.run_steps(_Wide(engine), *shape, 1))


@pytest.mark.parametrize("kw", [dict(kind="mse"), dict(per_member_bounds=True, grad_scale=1 / 3)], ids=["mse", "member_bounds_third"])
def test_one_step_of_every_kind(engine, kw):
    _one_step_checks(tr.run_steps(_Wide(engine), 3, 300, 5, 300, 4, 3, "silu", 1, **kw))


def test_twenty_steps_whatever_the_calls(engine):
    """Ragged last minibatch, Adam resumed at step 123: the restatement's trajectory; the same bits from three calls and from a rerun."""
    r = tr.run_steps(_Wide(engine), *TWENTY, 20, N=150, ragged_last=True, step0=123, f32_orders=True)
    _multi_step_checks(r, "20 wide steps: ")
    assert _same_bits(r, tr.run_steps(_Wide(engine), *TWENTY, 20, N=150, ragged_last=True, step0=123, calls=[7, 7, 6], restate=False)), "three calls"
    assert _same_bits(r, tr.run_steps(_Wide(engine), *TWENTY, 20, N=150, ragged_last=True, step0=123, restate=False)), "rerun"


def test_indices_outside_the_dataset_read_zeros(engine):
    N = 150

    def edit(idx):
        idx[0, 0, 0], idx[0, 1, 33], idx[0, 2, 39] = -1, N, -1  # (in both row blocks, the last row included)

    _one_step_checks(tr.run_steps(_Wide(engine), *TWENTY, 1, N=N, edit_idx=edit), "outside idx: ")


@pytest.mark.parametrize("shape", [(2, 5, 257, 4, 3), (2, 512, 1024, 512, 3)], ids=lambda s: "e{}_in{}_hid{}_out{}_l{}".format(*s))
def test_evaluate_matches_restatement(engine, shape):
    E, in_dim, hid, out, L = shape
    N, act = 70, "silu"
    g = torch.Generator().manual_seed(5)
    ws, bs = tr.random_model(E, in_dim, hid, out, L, 4)
    x, y = torch.randn(N, in_dim, generator=g, dtype=torch.float64), torch.randn(N, out, generator=g, dtype=torch.float64)
    perm = torch.randperm(N, generator=g).to(torch.int32)
    ref = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        w, b, xd, yd = [t.to(dt) for t in ws], [t.to(dt) for t in bs], x.to(dt), y.to(dt)
        _, _, o = tr.forward(w, b, xd.unsqueeze(0).expand(E, -1, -1), act)
        ref[name] = (tr.eval_score(w, b, xd, yd, act), ((o[..., :out] - yd) ** 2).sum(-1))
    w, b = [t.float().to(DEV) for t in ws], [t.float().to(DEV) for t in bs]
    xd, yd = x.float().to(DEV), y.float().to(DEV)
    for name, order, pick in (("none", None, slice(None)), ("perm", perm.to(DEV), perm.long())):
        score, rs = engine.train_eval(w, b, xd, yd, order, activation=act, row_scores=True, kernel="wide")
        assert torch.equal(engine.train_eval(w, b, xd, yd, order, activation=act, kernel="wide"), score), f"order={name}: score without row scores"
        tr.check(score, ref["f32"][0], ref["f64"][0], f"order={name}: score")
        tr.check(rs, ref["f32"][1][:, pick], ref["f64"][1][:, pick], f"order={name}: row scores")


def _trainer_run(engine, batch_size, hid=272, **kw):
    E, obs_dim, act_dim, L = 3, 6, 2, 3
    mlp = tr.TinyGaussianMLP(E, obs_dim + act_dim, hid, obs_dim, L, act="silu")
    tr.load_params(mlp, *tr.random_model(E, obs_dim + act_dim, hid, obs_dim, L, 11, dtype=torch.float32))
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((700, obs_dim)).astype(np.float32)
    data = tr.Batch(obs=obs, act=rng.uniform(-1, 1, (700, act_dim)).astype(np.float32),
                    next_obs=obs + 0.1 * rng.standard_normal(obs.shape).astype(np.float32))
    trainer = hipets.ModelTrainer(tr.TinyDynamicsModel(mlp), optim_lr=1e-3, engine=engine, **kw)
    ds = tr.BootstrapIterator(data, batch_size, E, shuffle_each_epoch=True, rng=np.random.default_rng(3))
    losses, scores = trainer.train(ds, num_epochs=2)
    return losses, scores, [p.detach().clone() for lin in mlp.layers() for p in (lin.weight, lin.bias)]


@pytest.mark.parametrize("batch_size", [32, 300])
def test_trainer_matches_the_float32_trainer(engine, batch_size):
    """Two epochs through hipets.ModelTrainer(step_kernel="wide") at hidden 272 against the same trainer over the float32 restatement;
    the bounds are those of test_gpu_trainer_split.test_trainer_matches_the_float32_trainer."""
    losses, scores, params = _trainer_run(engine, batch_size, step_kernel="wide")
    ref_losses, ref_scores, ref_params = _trainer_run(_CpuEngine(), batch_size, step_kernel="wide")
    assert np.allclose(losses, ref_losses, rtol=1e-4, atol=0) and np.allclose(scores, ref_scores, rtol=1e-4, atol=0)
    assert all((a - b).abs().max().item() < 2e-5 for a, b in zip(params, ref_params))


def test_limits_and_the_setting(engine):
    with pytest.raises(hipets.UnsupportedModelError, match='step_kernel="wide"'):
        _trainer_run(engine, 32, hid=300)
    with pytest.raises(hipets.UnsupportedModelError, match="hid <= 1024"):
        _trainer_run(engine, 32, hid=1025, step_kernel="wide")
    E, in_dim, out, L = 2, 5, 3, 3
    lo, hi = torch.full((out,), -10.0, device=DEV), torch.full((out,), 0.5, device=DEV)
    x, y = torch.randn(64, in_dim, device=DEV), torch.randn(64, out, device=DEV)

    def steps(hid, **kw):
        w, b, m, v = tr.fresh_state(*tr.random_model(E, in_dim, hid, out, L, 0), torch.float32, DEV)
        idx = (torch.arange(E * 16, dtype=torch.int32, device=DEV) % 64).reshape(1, E, 16)
        res = engine.train_steps(w, b, m, v, lo, hi, x, y, idx, torch.tensor([16], dtype=torch.int32, device=DEV), 0, lr=tr.LR, **kw)
        return list(w) + list(b) + list(res)

    before = steps(16)
    for hid, kw in ((1025, dict(kernel="wide")), (300, {})):
        with pytest.raises(hipets.HipetsError) as ei:
            steps(hid, **kw)
        assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
    steps(16, kernel="wide")
    assert all(torch.equal(p, q) for p, q in zip(before, steps(16))), "the engine's setting was not put back"
    with pytest.raises(hipets.HipetsError) as ei:
        engine._query("hipets_set_train_width", kind=2)
    assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
