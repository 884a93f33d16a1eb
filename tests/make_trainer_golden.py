"""TEST INFRASTRUCTURE (not collected): record the unmodified reference ModelTrainer (mbrl/models/model_trainer.py) on the CPU
through oracle.ref_bridge and write tests/golden/trainer_*.npz for tests/test_gpu_trainer.py.

    python tests/make_trainer_golden.py

Each case: a replay buffer of 517 random transitions, mbrl.util.common.get_basic_buffer_iterators (bootstrap, shuffling),
a GaussianMLP in a OneDTransitionRewardModel (delta targets, no normaliser), 3 epochs of ModelTrainer.train.  Stored: the
initial weights, the transitions and the split, every batch's loss and grad_norm, per-epoch losses and validation scores,
epochs run, final weights, elites, the weights / Adam state / RNG state after epoch 1, and the RNG state afterwards.

trainer_c_two_calls: the same tiny model trained as a PETS loop trains it, by ONE ModelTrainer on a growing buffer: 300 stored
transitions, new iterators, 2 epochs; the other 217 added, new iterators, 2 more epochs.  Stored per call: the split, the member
indices, the RNG states, every batch's loss and grad_norm, per-epoch losses and scores, the weights and elites afterwards; and
the optimizer's step count at the end."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_bridge  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASES = [  # name, activation, validation ratio, patience, seed
    ("trainer_a_noval_silu", "silu", 0.0, None, 5),
    ("trainer_b_val_relu", "relu", 0.2, 1, 6),
]
E, OBS, ACT, HID, NUM_LAYERS, N, BATCH, EPOCHS, LR, WD = 5, 6, 2, 32, 2, 517, 32, 3, 1e-3, 1e-5
TARGETS = {"silu": "torch.nn.SiLU", "relu": "torch.nn.ReLU"}


def record(name, act, val_ratio, patience, seed):
    ref_bridge.import_reference()
    import mbrl.models as models
    import mbrl.util.common as common
    from mbrl.util.replay_buffer import ReplayBuffer

    torch.manual_seed(seed)
    gen = np.random.default_rng(seed + 100)
    obs = gen.standard_normal((N, OBS)).astype(np.float32)
    acts = gen.uniform(-1, 1, (N, ACT)).astype(np.float32)
    next_obs = (obs + 0.1 * np.tanh(obs @ gen.standard_normal((OBS, OBS)) + acts @ gen.standard_normal((ACT, OBS)))).astype(np.float32)
    rb = ReplayBuffer(N, (OBS,), (ACT,), rng=np.random.default_rng(seed))
    for i in range(N):
        rb.add(obs[i], acts[i], next_obs[i], 0.0, False, False)
    train_it, val_it = common.get_basic_buffer_iterators(rb, BATCH, val_ratio, ensemble_size=E, shuffle_each_epoch=True, bootstrap_permutes=False)
    rng_after_split = rb.rng.bit_generator.state
    row_of = {obs[i].tobytes(): i for i in range(N)}
    train_rows = np.array([row_of[o.tobytes()] for o in train_it.transitions.obs], np.int64)
    val_rows = np.array([row_of[o.tobytes()] for o in val_it.transitions.obs], np.int64) if val_it is not None else np.zeros(0, np.int64)

    mlp = models.GaussianMLP(OBS + ACT, OBS, "cpu", num_layers=NUM_LAYERS, ensemble_size=E, hid_size=HID,
                             activation_fn_cfg={"_target_": TARGETS[act]})
    dm = models.OneDTransitionRewardModel(mlp, target_is_delta=True, normalize=False, learned_rewards=False, num_elites=3)
    layers = [l[0] for l in mlp.hidden_layers] + [mlp.mean_and_logvar]
    arrays = {}
    for i, l in enumerate(layers):
        arrays[f"w0_{i}"] = l.weight.detach().numpy().copy()
        arrays[f"b0_{i}"] = l.bias.detach().numpy().copy()
    trainer = models.ModelTrainer(dm, optim_lr=LR, weight_decay=WD)
    batches, epoch1 = [], {}

    def batch_cb(epoch, loss, meta, mode):
        if mode == "train":
            batches.append((float(loss), float(meta["grad_norm"])))

    def epoch_cb(model, it, epoch, loss, score, best):
        if epoch == 0:
            for i, l in enumerate(layers):
                arrays[f"we1_{i}"] = l.weight.detach().numpy().copy()
                arrays[f"be1_{i}"] = l.bias.detach().numpy().copy()
            sd = trainer.optimizer.state_dict()
            epoch1["keys"] = sorted(int(k) for k in sd["state"])
            epoch1["step"] = float(next(iter(sd["state"].values()))["step"])
            for k in epoch1["keys"]:
                arrays[f"m_{k}"] = sd["state"][k]["exp_avg"].numpy().copy()
                arrays[f"v_{k}"] = sd["state"][k]["exp_avg_sq"].numpy().copy()
            epoch1["rng"] = json.dumps(rb.rng.bit_generator.state)

    losses, scores = trainer.train(train_it, val_it, num_epochs=EPOCHS, patience=patience, callback=epoch_cb, batch_callback=batch_cb)
    for i, l in enumerate(layers):
        arrays[f"w1_{i}"] = l.weight.detach().numpy().copy()
        arrays[f"b1_{i}"] = l.bias.detach().numpy().copy()
    arrays.update(obs=obs, act=acts, next_obs=next_obs, train_rows=train_rows, val_rows=val_rows,
                  member_indices=np.asarray(train_it.member_indices), batch_losses=np.array([b[0] for b in batches]),
                  batch_grad_norms=np.array([b[1] for b in batches]), train_losses=np.array(losses), val_scores=np.array(scores),
                  elites=np.array(mlp.elite_models, np.int64))
    meta = dict(E=E, n_layers=NUM_LAYERS + 1, in_dim=OBS + ACT, hid=HID, out=OBS, act=act, num_elites=dm.num_elites, batch_size=BATCH,
                lr=LR, weight_decay=WD, num_epochs=EPOCHS, patience=patience, epochs_run=len(losses),
                rng_state_after_split=json.dumps(rng_after_split), rng_state_after=json.dumps(rb.rng.bit_generator.state),
                rng_state_epoch1=epoch1["rng"], adam_step_epoch1=epoch1["step"], adam_state_keys=epoch1["keys"], val_ratio=val_ratio, seed=seed)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta_json=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes, epochs {len(losses)}, elites {mlp.elite_models}")


TWO_CALLS = ("trainer_c_two_calls", "silu", 0.2, 7, (300, N), 2)  # name, activation, validation ratio, seed, stored per call, epochs per call


def record_two_calls(name, act, val_ratio, seed, stored, epochs):
    ref_bridge.import_reference()
    import mbrl.models as models
    import mbrl.util.common as common
    from mbrl.util.replay_buffer import ReplayBuffer

    torch.manual_seed(seed)
    gen = np.random.default_rng(seed + 100)
    obs = gen.standard_normal((N, OBS)).astype(np.float32)
    acts = gen.uniform(-1, 1, (N, ACT)).astype(np.float32)
    next_obs = (obs + 0.1 * np.tanh(obs @ gen.standard_normal((OBS, OBS)) + acts @ gen.standard_normal((ACT, OBS)))).astype(np.float32)
    rb = ReplayBuffer(N, (OBS,), (ACT,), rng=np.random.default_rng(seed))
    row_of = {obs[i].tobytes(): i for i in range(N)}
    mlp = models.GaussianMLP(OBS + ACT, OBS, "cpu", num_layers=NUM_LAYERS, ensemble_size=E, hid_size=HID,
                             activation_fn_cfg={"_target_": TARGETS[act]})
    dm = models.OneDTransitionRewardModel(mlp, target_is_delta=True, normalize=False, learned_rewards=False, num_elites=3)
    layers = [l[0] for l in mlp.hidden_layers] + [mlp.mean_and_logvar]
    arrays = dict(obs=obs, act=acts, next_obs=next_obs)
    for i, l in enumerate(layers):
        arrays[f"w0_{i}"] = l.weight.detach().numpy().copy()
        arrays[f"b0_{i}"] = l.bias.detach().numpy().copy()
    trainer = models.ModelTrainer(dm, optim_lr=LR, weight_decay=WD)  # one trainer (one optimizer) for both calls, as pets.train
    calls, added = [], 0
    for c, n_stored in enumerate(stored):
        for i in range(added, n_stored):
            rb.add(obs[i], acts[i], next_obs[i], 0.0, False, False)
        added = n_stored
        train_it, val_it = common.get_basic_buffer_iterators(rb, BATCH, val_ratio, ensemble_size=E, shuffle_each_epoch=True, bootstrap_permutes=False)
        m = {"rng_state_after_split": json.dumps(rb.rng.bit_generator.state)}
        arrays[f"c{c}_train_rows"] = np.array([row_of[o.tobytes()] for o in train_it.transitions.obs], np.int64)
        arrays[f"c{c}_val_rows"] = np.array([row_of[o.tobytes()] for o in val_it.transitions.obs], np.int64)
        arrays[f"c{c}_member_indices"] = np.asarray(train_it.member_indices)
        batches = []
        losses, scores = trainer.train(train_it, val_it, num_epochs=epochs, patience=None,
                                       batch_callback=lambda ep, loss, meta, mode: batches.append((float(loss), float(meta["grad_norm"])))
                                       if mode == "train" else None)
        m["rng_state_after"] = json.dumps(rb.rng.bit_generator.state)
        m["epochs_run"] = len(losses)
        arrays[f"c{c}_batch_losses"] = np.array([b[0] for b in batches])
        arrays[f"c{c}_batch_grad_norms"] = np.array([b[1] for b in batches])
        arrays[f"c{c}_train_losses"], arrays[f"c{c}_val_scores"] = np.array(losses), np.array(scores)
        arrays[f"c{c}_elites"] = np.array(mlp.elite_models, np.int64)
        for i, l in enumerate(layers):
            arrays[f"c{c}_w1_{i}"] = l.weight.detach().numpy().copy()
            arrays[f"c{c}_b1_{i}"] = l.bias.detach().numpy().copy()
        calls.append(m)
    sd = trainer.optimizer.state_dict()
    steps = sorted({float(st["step"]) for st in sd["state"].values()})
    assert len(steps) == 1
    meta = dict(E=E, n_layers=NUM_LAYERS + 1, in_dim=OBS + ACT, hid=HID, out=OBS, act=act, num_elites=dm.num_elites, batch_size=BATCH,
                lr=LR, weight_decay=WD, num_epochs=epochs, patience=None, stored=list(stored), calls=calls, adam_step=steps[0],
                val_ratio=val_ratio, seed=seed)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta_json=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes, Adam step {steps[0]}, elites {mlp.elite_models}")


def record_host_cases():
    """train_host_cases.npz: (1) one and two float64 Model.update + torch.optim.Adam steps of a small GaussianMLP for every
    activation; (2) the dataset rows of every batch the reference's iterators yield over 3 epochs, for both bootstrap_permutes
    values and validation ratios 0 / 0.2, with what it takes to rebuild the iterators (split, member indices, RNG state)."""
    ref_bridge.import_reference()
    import mbrl.models as models
    import mbrl.util.common as common
    from mbrl.util.replay_buffer import ReplayBuffer

    arrays, meta = {}, {"update": {}, "schedule": {}}
    acts = {"silu": "torch.nn.SiLU", "relu": "torch.nn.ReLU", "leaky_relu": "torch.nn.LeakyReLU", "tanh": "torch.nn.Tanh",
            "sigmoid": "torch.nn.Sigmoid"}
    for ai, (act, target) in enumerate(acts.items()):
        torch.manual_seed(20 + ai)
        mlp = models.GaussianMLP(5, 3, "cpu", num_layers=2, ensemble_size=3, hid_size=8, activation_fn_cfg={"_target_": target}).double()
        with torch.no_grad():
            mlp.min_logvar[0, 0], mlp.max_logvar[0, 0] = -2.0, -1.0  # one column with active bounds
        layers = [l[0] for l in mlp.hidden_layers] + [mlp.mean_and_logvar]
        for i, l in enumerate(layers):
            arrays[f"u_{act}_w0_{i}"] = l.weight.detach().numpy().copy()
            arrays[f"u_{act}_b0_{i}"] = l.bias.detach().numpy().copy()
        opt = torch.optim.Adam(mlp.parameters(), lr=1e-2, weight_decay=1e-3, eps=1e-8)
        g = torch.Generator().manual_seed(30 + ai)
        res = []
        for step in range(2):
            x = torch.randn(3, 7, 5, generator=g, dtype=torch.float64)
            y = torch.randn(3, 7, 3, generator=g, dtype=torch.float64)
            arrays[f"u_{act}_x{step}"], arrays[f"u_{act}_y{step}"] = x.numpy(), y.numpy()
            loss, m = mlp.update(x, opt, y)
            res.append((loss, m["grad_norm"]))
            for i, l in enumerate(layers):
                arrays[f"u_{act}_w{step + 1}_{i}"] = l.weight.detach().numpy().copy()
                arrays[f"u_{act}_b{step + 1}_{i}"] = l.bias.detach().numpy().copy()
                st = opt.state[l.weight]
                arrays[f"u_{act}_m{step + 1}_{i}"] = st["exp_avg"].numpy().copy()
                arrays[f"u_{act}_v{step + 1}_{i}"] = st["exp_avg_sq"].numpy().copy()
        arrays[f"u_{act}_min_logvar"] = mlp.min_logvar.detach().numpy().copy()
        arrays[f"u_{act}_max_logvar"] = mlp.max_logvar.detach().numpy().copy()
        meta["update"][act] = {"loss": [r[0] for r in res], "grad_norm": [r[1] for r in res]}
    gen = np.random.default_rng(1)
    obs = gen.standard_normal((N, OBS)).astype(np.float32)
    acts_ = gen.uniform(-1, 1, (N, ACT)).astype(np.float32)
    arrays.update(s_obs=obs, s_act=acts_)
    row_of = {obs[i].tobytes(): i for i in range(N)}
    for permutes in (False, True):
        for ratio in (0.0, 0.2):
            key = f"p{int(permutes)}_r{int(ratio * 10)}"
            rb = ReplayBuffer(N, (OBS,), (ACT,), rng=np.random.default_rng(7))
            for i in range(N):
                rb.add(obs[i], acts_[i], obs[i], 0.0, False, False)
            tr_it, val_it = common.get_basic_buffer_iterators(rb, BATCH, ratio, ensemble_size=E, shuffle_each_epoch=True, bootstrap_permutes=permutes)
            meta["schedule"][key] = {"rng_state_after_split": json.dumps(rb.rng.bit_generator.state)}
            arrays[f"s_{key}_train_rows"] = np.array([row_of[o.tobytes()] for o in tr_it.transitions.obs], np.int16)
            arrays[f"s_{key}_member_indices"] = np.asarray(tr_it.member_indices).astype(np.int16)
            local = {o.tobytes(): i for i, o in enumerate(tr_it.transitions.obs)}  # rows of the iterator's own dataset
            rows = []
            for _ in range(EPOCHS):
                for batch in tr_it:
                    rows.append(np.array([[local[o.tobytes()] for o in member] for member in batch.obs], np.int16).reshape(E, -1))
            arrays[f"s_{key}_batches"] = np.concatenate(rows, axis=1)
            meta["schedule"][key]["batch_sizes"] = [int(r.shape[1]) for r in rows]
            meta["schedule"][key]["rng_state_after"] = json.dumps(rb.rng.bit_generator.state)
    path = os.path.join(OUT, "train_host_cases.npz")
    np.savez_compressed(path, meta_json=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for case in CASES:
        record(*case)
    record_two_calls(*TWO_CALLS)
    record_host_cases()
