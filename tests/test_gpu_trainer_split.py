"""The row-split training step (Engine.train_steps(kernel="split"), hipets.ModelTrainer(step_kernel=...)) on the MI355X against the
float64 / float32 restatement (tests/train_restatement.py), by the suite's self-calibrated rule: |hip - f64| <= 4 |f32 - f64| + 1e-7.
The checks are those of the member kernel's tests (test_gpu_trainer_edges: one step through loss, grad_sq, both moments and Adam's
formula on the kernel's own moments; several steps through losses and final parameters)."""
import numpy as np
import pytest
import torch

import hipets
import train_restatement as tr
from test_gpu_trainer_edges import _multi_step_checks, _one_step_checks, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Split:
    """the engine with every train_steps call on the split kernels (tr.run_steps passes no keyword through)"""

    def __init__(self, engine):
        self.train_steps = lambda *a, **kw: engine.train_steps(*a, kernel="split", **kw)


class _CpuEngine(tr.CpuEngine):
    def train_steps(self, *a, kernel="member", **kw):  # (the restatement has one way to run a step)
        return super().train_steps(*a, **kw)


# (E, B, in, hid, out, n_layers, activation): one row; one below and one above a 32-row block, which is the dW product's K-chunk too;
# the first batch size the member kernel refuses and the limit; mbpo_halfcheetah; the LDS / width limit with 1024 output columns
ONE_STEP = [(2, 1, 5, 37, 4, 3, "silu"), (3, 31, 5, 37, 4, 3, "relu"), (3, 33, 5, 37, 4, 3, "leaky_relu"), (2, 257, 5, 37, 4, 3, "tanh"),
            (2, 1024, 5, 37, 4, 3, "sigmoid"), (7, 256, 23, 200, 18, 5, "silu"), (2, 64, 512, 256, 512, 3, "silu")]


@pytest.mark.parametrize("shape", ONE_STEP, ids=lambda s: "e{}_b{}_in{}_hid{}_out{}_l{}_{}".format(*s))
def test_one_step_matches_restatement(engine, shape):
    _one_step_checks(tr.run_steps(_Split(engine), *shape, 1))


@pytest.mark.parametrize("kw", [dict(kind="mse"), dict(per_member_bounds=True, grad_scale=1 / 3)], ids=["mse", "member_bounds_third"])
def test_one_step_of_every_kind(engine, kw):
    _one_step_checks(tr.run_steps(_Split(engine), 3, 300, 5, 37, 4, 3, "silu", 1, **kw))


def test_twenty_steps_whatever_the_calls(engine):
    """Ragged last minibatch, Adam resumed at step 123: the restatement's trajectory; the same bits from three calls and from a rerun."""
    shape = (3, 40, 6, 32, 4, 4, "silu", 20)
    r = tr.run_steps(_Split(engine), *shape, N=150, ragged_last=True, step0=123, f32_orders=True)
    _multi_step_checks(r, "20 split steps: ")
    assert _same_bits(r, tr.run_steps(_Split(engine), *shape, N=150, ragged_last=True, step0=123, calls=[7, 7, 6], restate=False)), "three calls"
    assert _same_bits(r, tr.run_steps(_Split(engine), *shape, N=150, ragged_last=True, step0=123, restate=False)), "rerun"


def test_indices_outside_the_dataset_read_zeros(engine):
    N = 150

    def edit(idx):
        idx[0, 0, 0], idx[0, 1, 33], idx[0, 2, 39] = -1, N, -1  # (in both row blocks, the last row included)

    _one_step_checks(tr.run_steps(_Split(engine), 3, 40, 6, 32, 4, 4, "silu", 1, N=N, edit_idx=edit), "outside idx: ")


def _trainer_run(engine, batch_size, **kw):
    E, obs_dim, act_dim, hid, L = 3, 6, 2, 32, 3
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


@pytest.mark.parametrize("batch_size, kw", [(300, {}), (32, dict(step_kernel="split"))], ids=["auto_b300", "split_b32"])
def test_trainer_matches_the_float32_trainer(engine, batch_size, kw):
    """Two epochs through hipets.ModelTrainer on the split kernels against the same trainer over the float32 restatement; the bounds are
    those of test_gpu_trainer.test_train_matches_reference_trainer, whose yardstick is a float32 run as well (rtol 1e-4 on losses and
    scores; 2e-5 absolute on the final parameters)."""
    losses, scores, params = _trainer_run(engine, batch_size, **kw)
    ref_losses, ref_scores, ref_params = _trainer_run(_CpuEngine(), batch_size, **kw)
    assert np.allclose(losses, ref_losses, rtol=1e-4, atol=0) and np.allclose(scores, ref_scores, rtol=1e-4, atol=0)
    assert all((a - b).abs().max().item() < 2e-5 for a, b in zip(params, ref_params))


def test_limits_and_the_setting(engine):
    with pytest.raises(hipets.UnsupportedModelError, match="batch size 300 > 256"):
        _trainer_run(engine, 300, step_kernel="member")
    E, in_dim, hid, out, L = 2, 5, 16, 3, 3
    ws, bs = tr.random_model(E, in_dim, hid, out, L, 0)
    lo, hi = torch.full((out,), -10.0, device=DEV), torch.full((out,), 0.5, device=DEV)
    x, y = torch.randn(64, in_dim, device=DEV), torch.randn(64, out, device=DEV)

    def steps(B, **kw):
        w, b, m, v = tr.fresh_state(ws, bs, torch.float32, DEV)
        idx = (torch.arange(E * B, dtype=torch.int32, device=DEV) % 64).reshape(1, E, B)
        res = engine.train_steps(w, b, m, v, lo, hi, x, y, idx, torch.tensor([B], dtype=torch.int32, device=DEV), 0, lr=tr.LR, **kw)
        return list(w) + list(b) + list(res)

    before = steps(16)
    with pytest.raises(hipets.HipetsError) as ei:
        steps(1025, kernel="split")
    assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
    steps(16, kernel="split")
    assert all(torch.equal(p, q) for p, q in zip(before, steps(16))), "the engine's setting was not put back"
    with pytest.raises(hipets.HipetsError) as ei:
        engine._query("hipets_set_train_kernel", kind=2)
    assert ei.value.kind == hipets.ERR_INVALID_ARGUMENT
