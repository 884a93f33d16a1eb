"""TEST HELPER (not collected): what the tests of the loss kinds hipets.ModelTrainer trains with ``extended=True`` need next to
tests/train_restatement.py (which restates the update of either kind): TinyBasicEnsemble, a ``members`` ModuleList of one-member
TinyGaussianMLPs in the reference's parameter order, and golden_setup for the tests/golden/trainerx_*.npz recordings.  The ``*_kind``
names are the restatement's functions under the names and argument orders they had when this module held a copy of each."""
from __future__ import annotations

import json
import warnings

import numpy as np
import torch

import train_restatement as tr
from train_restatement import bounds_3d, member_bounds, mse_step, seq_matmul  # noqa: F401  (used through this module)

nll_step_kind = tr.nll_step
load_params_kind = tr.load_params
CpuEngineKinds = tr.CpuEngine


def train_step_kind(kind, ws, bs, ms, vs, x, y, min_lv, max_lv, act, step, lr, weight_decay, eps=1e-8, slope=0.01, grad_scale=1.0,
                    sequential=False):
    return tr.train_step(ws, bs, ms, vs, x, y, min_lv, max_lv, act, step, lr, weight_decay, eps, slope, grad_scale, sequential, kind=kind)


def random_model_kind(kind, E, in_dim, hid, out, n_layers, seed, dtype=torch.float64):
    return tr.random_model(E, in_dim, hid, out, n_layers, seed, dtype, kind=kind)


def run_steps_kind(engine, kind, E, B, in_dim, hid, out, n_layers, act, n_steps, N=None, seed=0, steps_per_launch=0, ragged_last=False, *,
                   grad_scale=1.0, restate=True, f32_orders=False, device="cuda:0"):
    """train_restatement.run_steps of loss ``kind``: "nll" with per-member bounds, f32_orders with the sequential order ("f32s") too,
    and the engine always told the kind."""
    return tr.run_steps(engine, E, B, in_dim, hid, out, n_layers, act, n_steps, N, seed, steps_per_launch, ragged_last, kind=kind,
                        per_member_bounds=kind == "nll", grad_scale=grad_scale, restate=restate, f32_orders=f32_orders,
                        sequential_order=f32_orders, device=device)


# ---- stand-ins for the live objects ------------------------------------------------------------------------------------
class TinyBasicEnsemble(torch.nn.Module):
    """The attributes hipets.ModelTrainer reads from a BasicEnsemble of one-member GaussianMLPs: ``members``, ``deterministic``,
    ``__len__``, a set_elite that warns and keeps every member (basic_ensemble.py:262-267).  parameters() runs member by member
    (min_logvar, max_logvar, then the layers' weight / bias), the reference's order."""

    def __init__(self, E, in_dim, hid, out, n_layers, act="silu", deterministic=False, learn_logvar_bounds=False):
        super().__init__()
        self.members = torch.nn.ModuleList([tr.TinyGaussianMLP(1, in_dim, hid, out, n_layers, act=act, deterministic=deterministic,
                                                               learn_logvar_bounds=learn_logvar_bounds) for _ in range(E)])
        self.num_members = E
        self.deterministic = deterministic
        self.elite_models = None

    def __len__(self):
        return len(self.members)

    def layers(self):
        """per linear layer, a stand-in whose weight / bias are the members' [1, ., .] parameters in member order"""
        per_member = [m.layers() for m in self.members]
        return [[pm[i] for pm in per_member] for i in range(len(per_member[0]))]

    def set_elite(self, elite):
        warnings.warn("BasicEnsemble does not support elite models yet. All models will be used.")


def stacked_params(mlp):
    """(ws, bs) [E, ., .] of the live parameters of either stand-in"""
    if not isinstance(mlp, TinyBasicEnsemble):
        return [l.weight.detach().clone() for l in mlp.layers()], [l.bias.detach().clone() for l in mlp.layers()]
    return ([torch.cat([l.weight.detach() for l in layer]) for layer in mlp.layers()],
            [torch.cat([l.bias.detach() for l in layer]) for layer in mlp.layers()])


def golden_setup(meta, arr):
    """The model of a tests/golden/trainerx_*.npz recording at its initial weights (and bounds) with the reference's split, member
    indices and RNG state: (mlp, dynamics model, train iterator, validation iterator or None, rng)."""
    E, L = meta["E"], meta["n_layers"]
    cls = TinyBasicEnsemble if meta["basic"] else tr.TinyGaussianMLP
    mlp = cls(E, meta["in_dim"], meta["hid"], meta["out"], L, act=meta["act"], deterministic=meta["deterministic"])
    tr.load_params(mlp, [arr[f"w0_{i}"] for i in range(L)], [arr[f"b0_{i}"] for i in range(L)])
    if not meta["deterministic"]:
        with torch.no_grad():
            for e, m in enumerate(mlp.members if meta["basic"] else [mlp]):
                m.min_logvar.copy_(torch.from_numpy(arr["min_logvar"][e:e + 1]))
                m.max_logvar.copy_(torch.from_numpy(arr["max_logvar"][e:e + 1]))
    model = tr.TinyDynamicsModel(mlp, num_elites=meta["num_elites"])
    data = tr.Batch(obs=arr["obs"], act=arr["act"], next_obs=arr["next_obs"])
    rng = np.random.default_rng()
    rng.bit_generator.state = json.loads(meta["rng_state_after_split"])
    train = tr.BootstrapIterator(data[arr["train_rows"]], meta["batch_size"], E, shuffle_each_epoch=True, rng=rng,
                                 member_indices=arr["member_indices"])
    val = None
    if len(arr["val_rows"]):
        val = tr.TransitionIterator(data[arr["val_rows"]], meta["batch_size"], shuffle_each_epoch=False, rng=rng)
    return mlp, model, train, val, rng
