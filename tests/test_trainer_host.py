"""hipets.ModelTrainer's host side without a GPU: the restatement of one update (tests/train_restatement.py) against the
reference's own Model.update + torch.optim.Adam in float64, the index schedule the trainer builds against the batches the
reference's iterators yielded, the replay buffer's RNG after a train() against the reference trainer's, and the optimizer's
state_dict against torch.optim.Adam's.  The reference's side is recorded in tests/golden/trainer_*.npz
(tests/make_trainer_golden.py); the device steps run here on a CPU stand-in of the engine that applies the restatement."""
import json
import os

import numpy as np
import pytest
import torch

import hipets
import train_restatement as tr
from conftest import GOLDEN
from test_gpu_trainer import GOLDENS, TWO_CALLS, _golden, _setup, _setup_two_calls

HOST = os.path.join(GOLDEN, "train_host_cases.npz")


def _host():
    z = np.load(HOST)
    return json.loads(bytes(z["meta_json"]).decode()), {k: z[k] for k in z.files if k != "meta_json"}


def CpuEngine():
    """Engine.train_steps / train_eval in float32 on the CPU through the restatement (host-logic tests only), with the keywords the
    engine had before the loss kinds and no others."""
    return tr.CpuEngine(kinds=False)


@pytest.mark.parametrize("act", tr.ACTS)
def test_restatement_equals_reference_update_float64(act):
    meta, a = _host()
    L = 3
    ws = [torch.from_numpy(a[f"u_{act}_w0_{i}"]).clone() for i in range(L)]
    bs = [torch.from_numpy(a[f"u_{act}_b0_{i}"]).clone() for i in range(L)]
    ms = ([torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs])
    vs = ([torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs])
    lo, hi = torch.from_numpy(a[f"u_{act}_min_logvar"]), torch.from_numpy(a[f"u_{act}_max_logvar"])
    const = 0.01 * (hi.sum() - lo.sum()).item()
    for step in range(2):
        x, y = torch.from_numpy(a[f"u_{act}_x{step}"]), torch.from_numpy(a[f"u_{act}_y{step}"])
        loss, gsq = tr.train_step(ws, bs, ms, vs, x, y, lo, hi, act, step + 1, 1e-2, 1e-3)
        assert abs(loss.sum().item() + const - meta["update"][act]["loss"][step]) < 1e-12
        assert abs(gsq.sum().item() - meta["update"][act]["grad_norm"][step]) < 1e-12 * max(1.0, gsq.sum().item())
        for i in range(L):
            assert (ws[i] - torch.from_numpy(a[f"u_{act}_w{step + 1}_{i}"])).abs().max().item() < 1e-12
            assert (bs[i] - torch.from_numpy(a[f"u_{act}_b{step + 1}_{i}"])).abs().max().item() < 1e-12
            assert (ms[0][i] - torch.from_numpy(a[f"u_{act}_m{step + 1}_{i}"])).abs().max().item() < 1e-12
            assert (vs[0][i] - torch.from_numpy(a[f"u_{act}_v{step + 1}_{i}"])).abs().max().item() < 1e-12


def _small_trainer(E=5):
    mlp = tr.TinyGaussianMLP(E, 8, 16, 6, 3)
    return hipets.ModelTrainer(tr.TinyDynamicsModel(mlp), optim_lr=1e-3, engine=CpuEngine()), mlp


@pytest.mark.parametrize("key", ["p0_r0", "p0_r2", "p1_r0", "p1_r2"])
def test_index_schedule_equals_reference_iterator_batches(key):
    """3 epochs of the trainer's schedule (built by the iterator's own __iter__) = the rows of the batches the reference's
    BootstrapIterator yielded, for bootstrap_permutes False / True and validation ratios 0 / 0.2; the RNG ends where it did."""
    meta, a = _host()
    m = meta["schedule"][key]
    rng = np.random.default_rng()
    rng.bit_generator.state = json.loads(m["rng_state_after_split"])
    data = tr.Batch(obs=a["s_obs"], act=a["s_act"], next_obs=a["s_obs"])
    it = tr.BootstrapIterator(data[a[f"s_{key}_train_rows"].astype(np.int64)], 32, 5, shuffle_each_epoch=True, rng=rng,
                              member_indices=a[f"s_{key}_member_indices"].astype(np.int64))
    trainer, _ = _small_trainer()
    got = []
    for _ in range(3):
        idx, rows = trainer._schedule(it)
        got += [idx[i, :, :rows[i]] for i in range(len(rows))]
    assert [g.shape[1] for g in got] == m["batch_sizes"]
    assert np.array_equal(np.concatenate(got, axis=1), a[f"s_{key}_batches"].astype(np.int64))
    assert json.dumps(rng.bit_generator.state, sort_keys=True) == json.dumps(json.loads(m["rng_state_after"]), sort_keys=True)


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p) for p in GOLDENS])
def test_train_host_logic_and_rng_match_reference_trainer(path):
    """A whole train() with the device steps replaced by the float32 restatement: the replay buffer's RNG ends bit for bit where
    the reference trainer's did, with the same epochs run, elites and (to float32 noise) losses and scores."""
    meta, arr = _golden(path)
    mlp, model, train, val, rng = _setup(meta, arr)
    trainer = hipets.ModelTrainer(model, optim_lr=meta["lr"], weight_decay=meta["weight_decay"], engine=CpuEngine())
    losses, scores = trainer.train(train, val, num_epochs=meta["num_epochs"], patience=meta["patience"])
    assert json.dumps(rng.bit_generator.state, sort_keys=True) == json.dumps(json.loads(meta["rng_state_after"]), sort_keys=True)
    assert len(losses) == meta["epochs_run"]
    assert np.allclose(losses, arr["train_losses"], rtol=1e-5) and np.allclose(scores, arr["val_scores"], rtol=1e-5)
    assert sorted(int(i) for i in mlp.elite_models) == sorted(int(i) for i in arr["elites"])
    assert trainer._train_iteration == 1


def test_two_train_calls_on_a_growing_buffer_host_logic():
    """One trainer, two train() calls (300 stored transitions, then 517, new iterators each time: a PETS loop), the device steps
    replaced by the float32 restatement: Adam's moments and step count carry over, the dataset of the second call replaces the
    first's, and after each call the RNG, epochs, elites and (to float32 noise) losses and scores are the reference trainer's."""
    meta, arr = _golden(TWO_CALLS)
    mlp, model, iterators = _setup_two_calls(meta, arr)
    trainer = hipets.ModelTrainer(model, optim_lr=meta["lr"], weight_decay=meta["weight_decay"], engine=CpuEngine())
    for c, m in enumerate(meta["calls"]):
        train, val, rng = iterators(c)
        losses, scores = trainer.train(train, val, num_epochs=meta["num_epochs"], patience=meta["patience"])
        assert json.dumps(rng.bit_generator.state, sort_keys=True) == json.dumps(json.loads(m["rng_state_after"]), sort_keys=True)
        assert len(losses) == m["epochs_run"]
        assert np.allclose(losses, arr[f"c{c}_train_losses"], rtol=1e-5) and np.allclose(scores, arr[f"c{c}_val_scores"], rtol=1e-5)
        assert sorted(int(i) for i in mlp.elite_models) == sorted(int(i) for i in arr[f"c{c}_elites"])
        for i, lin in enumerate(mlp.layers()):
            assert np.abs(lin.weight.detach().numpy() - arr[f"c{c}_w1_{i}"]).max() < 2e-5
        assert trainer._train_iteration == c + 1
    assert trainer._step == int(meta["adam_step"])
    assert float(next(iter(trainer.optimizer.state_dict()["state"].values()))["step"]) == meta["adam_step"]


def test_optimizer_state_dict_round_trips_through_torch_adam():
    trainer, mlp = _small_trainer()
    rng = np.random.default_rng(3)
    obs = rng.standard_normal((100, 6)).astype(np.float32)
    data = tr.Batch(obs=obs, act=rng.uniform(-1, 1, (100, 2)).astype(np.float32), next_obs=obs * 1.1)
    trainer.train(tr.BootstrapIterator(data, 16, 5, shuffle_each_epoch=True, rng=rng), num_epochs=2, evaluate=False)
    sd = trainer.optimizer.state_dict()
    assert set(sd["state"]) == set(range(2, 2 + 2 * 3))  # min_logvar / max_logvar (indices 0, 1) never get a gradient
    opt = torch.optim.Adam(trainer.model.parameters(), lr=1e-3)
    opt.load_state_dict(sd)
    back = opt.state_dict()
    assert back["param_groups"][0]["lr"] == 1e-3 and back["param_groups"][0]["params"] == sd["param_groups"][0]["params"]
    for k, st in sd["state"].items():
        assert float(back["state"][k]["step"]) == float(st["step"]) == 2 * 7
        assert torch.equal(back["state"][k]["exp_avg"], st["exp_avg"]) and torch.equal(back["state"][k]["exp_avg_sq"], st["exp_avg_sq"])
    trainer2, _ = _small_trainer()
    trainer2.optimizer.load_state_dict(back)
    assert trainer2._step == 14
    sd2 = trainer2.optimizer.state_dict()
    for k in sd["state"]:
        assert torch.equal(sd2["state"][k]["exp_avg_sq"], sd["state"][k]["exp_avg_sq"])
    trainer2.optimizer.param_groups[0]["lr"] = 0.5  # honoured at the next train()
    assert trainer2.optimizer.state_dict()["param_groups"][0]["lr"] == 0.5


def test_unsupported_models_raise_at_construction():
    for kw in (dict(deterministic=True), dict(learn_logvar_bounds=True)):
        with pytest.raises(hipets.UnsupportedModelError, match="keep mbrl.models.ModelTrainer"):
            hipets.ModelTrainer(tr.TinyDynamicsModel(tr.TinyGaussianMLP(3, 5, 8, 4, 3, **kw)), engine=CpuEngine())
    with pytest.raises(hipets.UnsupportedModelError):
        hipets.ModelTrainer(tr.TinyDynamicsModel(tr.TinyGaussianMLP(17, 5, 8, 4, 3)), engine=CpuEngine())  # 17 members
