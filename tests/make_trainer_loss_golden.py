"""TEST INFRASTRUCTURE (not collected): record the unmodified reference ModelTrainer (mbrl/models/model_trainer.py) on the CPU
through oracle.ref_bridge for the model kinds hipets.ModelTrainer trains with ``extended=True``, and write
tests/golden/trainerx_*.npz for tests/test_trainer_kinds_host.py and tests/test_gpu_trainer_kinds.py.

    python tests/make_trainer_loss_golden.py

The recipe and the stored fields are those of tests/make_trainer_golden.py (517 random transitions, bootstrap + shuffling
iterators of mbrl.util.common.get_basic_buffer_iterators, a OneDTransitionRewardModel with delta targets and no normaliser, 3
epochs of ModelTrainer.train), for three models:

  trainerx_basic_nll  BasicEnsemble of 5 one-member GaussianMLPs, NLL; members 1 and 3 own bounds (-2, -1) in column 0, so the
                      bounds are active and differ by member; validation ratio 0.2, patience 1
  trainerx_gmlp_mse   GaussianMLP(deterministic=True) of 5 members
  trainerx_basic_mse  BasicEnsemble of 5 deterministic one-member GaussianMLPs

The weights of a BasicEnsemble are stored stacked: w0_i [E, in, out] = its members' [1, in, out] tensors in member order; the Adam
state is stored as the reference's state_dict has it (one entry per live parameter, [1, ., .] each), with the shapes of
model.parameters() in order (meta "param_shapes").  The prefix trainerx_ keeps these files out of the trainer_*.npz glob of
tests/test_gpu_trainer.py.

trainerx_host_cases.npz: one and two float64 Model.update + torch.optim.Adam steps of a small model of each kind."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_bridge  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASES = [  # name, basic ensemble?, deterministic?, activation, validation ratio, patience, seed
    ("trainerx_basic_nll", True, False, "silu", 0.2, 1, 15),
    ("trainerx_gmlp_mse", False, True, "relu", 0.0, None, 16),
    ("trainerx_basic_mse", True, True, "tanh", 0.0, None, 17),
]
E, OBS, ACT, HID, NUM_LAYERS, N, BATCH, EPOCHS, LR, WD = 5, 6, 2, 32, 2, 517, 32, 3, 1e-3, 1e-5
TARGETS = {"silu": "torch.nn.SiLU", "relu": "torch.nn.ReLU", "tanh": "torch.nn.Tanh"}
ACTIVE_BOUNDS = {1: (-2.0, -1.0), 3: (-2.0, -1.0)}  # member -> (min, max) of column 0 (NLL BasicEnsembles)


def build(models, basic, deterministic, act, in_size, out_size, hid, num_layers, ensemble_size):
    """(model, [member GaussianMLPs]) of the reference: a BasicEnsemble as conf/dynamics_model/basic_ensemble.yaml builds it."""
    if basic:
        member_cfg = {"_target_": "mbrl.models.GaussianMLP", "device": "cpu", "num_layers": num_layers, "in_size": in_size,
                      "out_size": out_size, "hid_size": hid, "deterministic": deterministic, "activation_fn_cfg": {"_target_": TARGETS[act]}}
        model = models.BasicEnsemble(ensemble_size, "cpu", member_cfg)
        members = list(model.members)
        if not deterministic:
            with torch.no_grad():
                for e, (lo, hi) in ACTIVE_BOUNDS.items():
                    if e < ensemble_size:
                        members[e].min_logvar[0, 0], members[e].max_logvar[0, 0] = lo, hi
        return model, members
    model = models.GaussianMLP(in_size, out_size, "cpu", num_layers=num_layers, ensemble_size=ensemble_size, hid_size=hid,
                               deterministic=deterministic, activation_fn_cfg={"_target_": TARGETS[act]})
    return model, [model]


def layers_of(members):
    """per linear layer, the members' EnsembleLinearLayers"""
    per_member = [[l[0] for l in m.hidden_layers] + [m.mean_and_logvar] for m in members]
    return [[pm[i] for pm in per_member] for i in range(len(per_member[0]))]


def stacked(layer, name):
    return np.concatenate([getattr(l, name).detach().numpy() for l in layer]).copy()


def record(name, basic, deterministic, act, val_ratio, patience, seed):
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

    model, members = build(models, basic, deterministic, act, OBS + ACT, OBS, HID, NUM_LAYERS, E)
    dm = models.OneDTransitionRewardModel(model, target_is_delta=True, normalize=False, learned_rewards=False, num_elites=3)
    layers = layers_of(members)
    arrays = {}
    for i, layer in enumerate(layers):
        arrays[f"w0_{i}"], arrays[f"b0_{i}"] = stacked(layer, "weight"), stacked(layer, "bias")
    if not deterministic:
        arrays["min_logvar"] = np.concatenate([m.min_logvar.detach().numpy() for m in members]).copy()
        arrays["max_logvar"] = np.concatenate([m.max_logvar.detach().numpy() for m in members]).copy()
    trainer = models.ModelTrainer(dm, optim_lr=LR, weight_decay=WD)
    batches, epoch1 = [], {}

    def batch_cb(epoch, loss, meta, mode):
        if mode == "train":
            batches.append((float(loss), float(meta["grad_norm"])))

    def epoch_cb(model_, it, epoch, loss, score, best):
        if epoch == 0:
            for i, layer in enumerate(layers):
                arrays[f"we1_{i}"], arrays[f"be1_{i}"] = stacked(layer, "weight"), stacked(layer, "bias")
            sd = trainer.optimizer.state_dict()
            epoch1["keys"] = sorted(int(k) for k in sd["state"])
            epoch1["step"] = float(next(iter(sd["state"].values()))["step"])
            for k in epoch1["keys"]:
                arrays[f"m_{k}"] = sd["state"][k]["exp_avg"].numpy().copy()
                arrays[f"v_{k}"] = sd["state"][k]["exp_avg_sq"].numpy().copy()
            epoch1["rng"] = json.dumps(rb.rng.bit_generator.state)

    losses, scores = trainer.train(train_it, val_it, num_epochs=EPOCHS, patience=patience, callback=epoch_cb, batch_callback=batch_cb)
    for i, layer in enumerate(layers):
        arrays[f"w1_{i}"], arrays[f"b1_{i}"] = stacked(layer, "weight"), stacked(layer, "bias")
    elites = getattr(model, "elite_models", None)
    arrays.update(obs=obs, act=acts, next_obs=next_obs, train_rows=train_rows, val_rows=val_rows,
                  member_indices=np.asarray(train_it.member_indices), batch_losses=np.array([b[0] for b in batches]),
                  batch_grad_norms=np.array([b[1] for b in batches]), train_losses=np.array(losses), val_scores=np.array(scores),
                  elites=np.array(elites if elites is not None else [], np.int64))
    meta = dict(E=E, n_layers=NUM_LAYERS + 1, in_dim=OBS + ACT, hid=HID, out=OBS, act=act, num_elites=dm.num_elites, batch_size=BATCH,
                lr=LR, weight_decay=WD, num_epochs=EPOCHS, patience=patience, epochs_run=len(losses), basic=basic, deterministic=deterministic,
                elites_set=elites is not None, param_shapes=[list(p.shape) for p in dm.parameters()],
                rng_state_after_split=json.dumps(rng_after_split), rng_state_after=json.dumps(rb.rng.bit_generator.state),
                rng_state_epoch1=epoch1["rng"], adam_step_epoch1=epoch1["step"], adam_state_keys=epoch1["keys"], val_ratio=val_ratio, seed=seed)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta_json=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes, epochs {len(losses)}, elites {elites}")


HOST_KINDS = [("basic_nll", True, False, "silu"), ("gmlp_mse", False, True, "tanh"), ("basic_mse", True, True, "relu")]


def record_host_cases():
    """trainerx_host_cases.npz: one and two float64 Model.update + torch.optim.Adam steps of a small model of every kind
    (E 3, in 5, hid 8, out 3, 7 rows per member): inputs, loss, grad_norm, and the weights and Adam moments after each step."""
    ref_bridge.import_reference()
    import mbrl.models as models

    arrays, meta = {}, {"update": {}}
    for ki, (kind, basic, deterministic, act) in enumerate(HOST_KINDS):
        torch.manual_seed(40 + ki)
        model, members = build(models, basic, deterministic, act, 5, 3, 8, 2, 3)
        model.double()
        layers = layers_of(members)
        for i, layer in enumerate(layers):
            arrays[f"u_{kind}_w0_{i}"], arrays[f"u_{kind}_b0_{i}"] = stacked(layer, "weight"), stacked(layer, "bias")
        if not deterministic:
            arrays[f"u_{kind}_min_logvar"] = np.concatenate([m.min_logvar.detach().numpy() for m in members]).copy()
            arrays[f"u_{kind}_max_logvar"] = np.concatenate([m.max_logvar.detach().numpy() for m in members]).copy()
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=1e-3, eps=1e-8)
        g = torch.Generator().manual_seed(50 + ki)
        res = []
        for step in range(2):
            x = torch.randn(3, 7, 5, generator=g, dtype=torch.float64)
            y = torch.randn(3, 7, 3, generator=g, dtype=torch.float64)
            arrays[f"u_{kind}_x{step}"], arrays[f"u_{kind}_y{step}"] = x.numpy(), y.numpy()
            loss, m = model.update(x, opt, y)
            res.append((loss, m["grad_norm"]))
            for i, layer in enumerate(layers):
                arrays[f"u_{kind}_w{step + 1}_{i}"], arrays[f"u_{kind}_b{step + 1}_{i}"] = stacked(layer, "weight"), stacked(layer, "bias")
                arrays[f"u_{kind}_m{step + 1}_{i}"] = np.concatenate([opt.state[l.weight]["exp_avg"].numpy() for l in layer]).copy()
                arrays[f"u_{kind}_v{step + 1}_{i}"] = np.concatenate([opt.state[l.weight]["exp_avg_sq"].numpy() for l in layer]).copy()
        meta["update"][kind] = {"loss": [r[0] for r in res], "grad_norm": [r[1] for r in res], "basic": basic, "deterministic": deterministic,
                                "act": act}
    path = os.path.join(OUT, "trainerx_host_cases.npz")
    np.savez_compressed(path, meta_json=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for case in CASES:
        record(*case)
    record_host_cases()
