"""ModelTrainer: a drop-in for ``mbrl.models.ModelTrainer`` (mbrl/models/model_trainer.py:31-297) whose minibatch steps and
evaluation passes run in libhipets (hipets_train_steps / hipets_train_eval):

    model_trainer = hipets.ModelTrainer(dynamics_model, optim_lr=..., weight_decay=..., logger=...)

Supported: a ``OneDTransitionRewardModel`` over one ``GaussianMLP`` (NLL loss, fixed logvar bounds).  Anything else raises
``UnsupportedModelError`` at construction: keep ``mbrl.models.ModelTrainer`` for it.  Torch is used for data preparation
and copies only; the update (forward, backward, Adam) never touches torch.autograd or torch.optim.

With ``extended=True`` (what ``hipets.make_model_trainer`` passes) two further kinds train in HIP: a ``GaussianMLP`` with
``deterministic=True`` (MSE loss) and a ``BasicEnsemble`` of one-member ``GaussianMLP``s of one shape (all NLL with fixed bounds, or
all deterministic).  ``learn_logvar_bounds=True``, mixed member kinds and members that are ensembles stay refused.

    model_trainer = hipets.make_model_trainer(dynamics_model, optim_lr=..., weight_decay=..., logger=...)
"""
from __future__ import annotations

import itertools
import warnings
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from ._lib import (TRAIN_MAX_BATCH as MAX_BATCH, TRAIN_MAX_HID as MAX_HID, TRAIN_MAX_IN as MAX_IN, TRAIN_MAX_MEMBERS as MAX_MEMBERS,
                   TRAIN_MAX_OUT as MAX_OUT)  # the library's shape limits (HIPETS_TRAIN_MAX_* of include/hipets.h) under this module's names
from .model import UnsupportedModelError, _ACT_BY_CLASS

# model_trainer.py:20-28 (the logger group's columns)
MODEL_LOG_FORMAT = [
    ("train_iteration", "I", "int"),
    ("epoch", "E", "int"),
    ("train_dataset_size", "TD", "int"),
    ("val_dataset_size", "VD", "int"),
    ("model_loss", "MLOSS", "float"),
    ("model_val_score", "MVSCORE", "float"),
    ("model_best_val_score", "MBVSCORE", "float"),
]

_KEEP_STOCK = "; keep mbrl.models.ModelTrainer for this model"


class _Kind:
    """What _read_model found: ``mlps`` = the GaussianMLPs that own the parameters (one vectorised model, or the E one-member
    members of a BasicEnsemble, ``basic``); ``layers[li]`` = the (weight, bias, member) live parameters that make up row ``member``
    of the stacked device tensor of linear layer li (member None: the whole [E, ., .] tensor); ``loss`` "nll" / "mse"."""

    def __init__(self, mlps, basic, layers, act, slope, loss):
        self.mlps, self.basic, self.layers, self.act, self.slope, self.loss = mlps, basic, layers, act, slope, loss


def _read_model(model, extended: bool = False) -> _Kind:
    """The model's kind and live parameters, or UnsupportedModelError.  ``extended``: deterministic GaussianMLPs (MSE loss) and
    BasicEnsembles of one-member GaussianMLPs are accepted as well."""
    mlp = getattr(model, "model", None)
    if mlp is None or not hasattr(model, "_process_batch"):
        raise UnsupportedModelError("hipets.ModelTrainer trains a OneDTransitionRewardModel" + _KEEP_STOCK)
    if hasattr(mlp, "members") and not hasattr(mlp, "hidden_layers"):
        if not extended:
            raise UnsupportedModelError("BasicEnsemble is not supported" + _KEEP_STOCK)
        return _read_basic_ensemble(mlp)
    layers, act, slope, loss = _read_mlp(mlp, extended)
    return _Kind([mlp], False, [[(lin.weight, lin.bias, None)] for lin in layers], act, slope, loss)


def _read_basic_ensemble(ens) -> _Kind:
    """A BasicEnsemble (mbrl/models/basic_ensemble.py) whose members are one-member GaussianMLPs of one shape, activation and loss."""
    members = list(ens.members)
    if not members:
        raise UnsupportedModelError("BasicEnsemble without members" + _KEEP_STOCK)
    if len(members) > MAX_MEMBERS:
        raise UnsupportedModelError(f"BasicEnsemble of {len(members)} members exceeds the trained shapes (E <= {MAX_MEMBERS})" + _KEEP_STOCK)
    read = []
    for i, m in enumerate(members):
        if hasattr(m, "members"):
            raise UnsupportedModelError(f"BasicEnsemble member {i} is an ensemble itself" + _KEEP_STOCK)
        try:
            read.append(_read_mlp(m, True))
        except UnsupportedModelError as exc:
            raise UnsupportedModelError(f"BasicEnsemble member {i}: {exc}") from None
        if int(read[-1][0][0].weight.shape[0]) != 1 or int(getattr(m, "num_members", 1)) != 1:
            raise UnsupportedModelError(f"BasicEnsemble member {i} is an ensemble itself (num_members != 1)" + _KEEP_STOCK)
    layers0, act, slope, loss = read[0]
    shapes0 = [tuple(lin.weight.shape) for lin in layers0]
    for i, (layers, a, s, l) in enumerate(read[1:], 1):
        if l != loss:
            raise UnsupportedModelError(f"BasicEnsemble mixes member kinds (member 0 trains with {loss}, member {i} with {l})" + _KEEP_STOCK)
        if [tuple(lin.weight.shape) for lin in layers] != shapes0:
            raise UnsupportedModelError(f"BasicEnsemble member {i} has other layer shapes than member 0" + _KEEP_STOCK)
        if a != act or s != slope:
            raise UnsupportedModelError(f"BasicEnsemble member {i} has another activation than member 0" + _KEEP_STOCK)
    stacked = [[(layers[li].weight, layers[li].bias, e) for e, (layers, _, _, _) in enumerate(read)] for li in range(len(layers0))]
    return _Kind(members, True, stacked, act, slope, loss)


def _read_mlp(mlp, extended: bool):
    """([linear layers], activation, slope, loss kind) of one GaussianMLP or UnsupportedModelError."""
    if not hasattr(mlp, "hidden_layers") or not hasattr(mlp, "mean_and_logvar"):
        raise UnsupportedModelError("dynamics_model.model is not a GaussianMLP" + _KEEP_STOCK)
    deterministic = bool(getattr(mlp, "deterministic", False))
    if deterministic and not extended:
        raise UnsupportedModelError("deterministic GaussianMLP (MSE loss) is not supported" + _KEEP_STOCK)
    if not deterministic and (mlp.min_logvar.requires_grad or mlp.max_logvar.requires_grad):
        raise UnsupportedModelError("learn_logvar_bounds=True is not supported (its gradient couples the members)" + _KEEP_STOCK)
    layers, act, slope = [], None, 0.01
    for layer in mlp.hidden_layers:
        lin, mod = layer[0], layer[1]
        name = _ACT_BY_CLASS.get(type(mod).__name__)
        if name is None or (act is not None and name != act):
            raise UnsupportedModelError(f"activation {type(mod).__name__} is not supported" + _KEEP_STOCK)
        act, slope = name, float(getattr(mod, "negative_slope", 0.01))
        layers.append(lin)
    layers.append(mlp.mean_and_logvar)
    for lin in layers:
        if not getattr(lin, "use_bias", True) or getattr(lin, "bias", None) is None:
            raise UnsupportedModelError("EnsembleLinearLayer without bias is not supported" + _KEEP_STOCK)
    w0 = layers[0].weight
    if w0.ndim != 3 or len(layers) < 2 or len(layers) > 8:
        raise UnsupportedModelError("expected 1..7 hidden ensemble layers of weights [E, in, out]" + _KEEP_STOCK)
    E, in_dim, hid = (int(v) for v in w0.shape)
    out2 = int(layers[-1].weight.shape[2])
    max_cols = MAX_OUT if deterministic else 2 * MAX_OUT
    if E > MAX_MEMBERS or hid > MAX_HID or in_dim > MAX_IN or out2 > max_cols:
        raise UnsupportedModelError(f"ensemble {E} x in {in_dim} x hid {hid} x out {out2} exceeds the trained shapes (E <= {MAX_MEMBERS}, "
                                    f"in <= {MAX_IN}, hid <= {MAX_HID}, out <= {max_cols} columns)" + _KEEP_STOCK)
    return layers, act or "relu", slope, "mse" if deterministic else "nll"


def _iterator_kind(ds) -> Optional[str]:
    """"bootstrap" / "transition" for mbrl.util.replay_buffer's own iterators (whose batches are index gathers of
    ``transitions``), None for any other iterable (iterated in Python)."""
    name = type(ds).__name__
    if not all(hasattr(ds, a) for a in ("transitions", "_order", "batch_size", "num_stored")):
        return None
    if name == "BootstrapIterator" and hasattr(ds, "member_indices") and hasattr(ds, "_bootstrap_iter"):
        return "bootstrap"
    if name == "TransitionIterator":
        return "transition"
    return None


class _AdamState:
    """``trainer.optimizer``: torch.optim.Adam's param_groups and state_dict format over the model's parameters; the moments
    live on the engine's GPU in the trainer.  The update itself is libhipets'."""

    def __init__(self, trainer, params, lr, weight_decay, eps):
        self._t = trainer
        self.param_groups = [dict(params=list(params), lr=lr, betas=(0.9, 0.999), eps=eps, weight_decay=weight_decay, amsgrad=False,
                                  maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                                  decoupled_weight_decay=False)]

    def state_dict(self) -> Dict:
        t = self._t
        params = self.param_groups[0]["params"]
        state = {}
        if t._step > 0:
            pos = {id(p): i for i, p in enumerate(params)}
            for li, e, k, p in t._slots():
                state[pos[id(p)]] = {"step": torch.tensor(float(t._step)), "exp_avg": t._rows(t._m[k][li], e).detach().to(p.device).clone(),
                                     "exp_avg_sq": t._rows(t._v[k][li], e).detach().to(p.device).clone()}
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(params)))
        return {"state": dict(sorted(state.items())), "param_groups": [group]}

    def load_state_dict(self, sd: Dict):
        t = self._t
        params = self.param_groups[0]["params"]
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(params):
            raise ValueError("state_dict does not match the model's parameters")
        for k, v in groups[0].items():
            if k != "params":
                self.param_groups[0][k] = v
        pos = {id(p): i for i, p in enumerate(params)}
        steps = set()
        for li, e, k, p in t._slots():
            st = sd["state"].get(groups[0]["params"][pos[id(p)]])
            if st is None:
                t._rows(t._m[k][li], e).zero_()
                t._rows(t._v[k][li], e).zero_()
                steps.add(0)
                continue
            t._rows(t._m[k][li], e).copy_(st["exp_avg"])
            t._rows(t._v[k][li], e).copy_(st["exp_avg_sq"])
            steps.add(int(float(st["step"])))
        if len(steps) != 1:
            raise ValueError("hipets.ModelTrainer keeps one Adam step count for all parameters")
        t._step = steps.pop()


class ModelTrainer:
    """Drop-in for ``mbrl.models.ModelTrainer``: same constructor, ``train`` / ``evaluate`` signatures and return values, the
    same patience / best-weights / elite logic, logger group and callbacks.  Minibatch steps run in chunks inside one
    kernel launch per chunk; ``batch_callback`` is replayed in order after each epoch from one device read per epoch.
    Training runs on ``engine``'s GPU (default: ``device`` or cuda:current) whatever device the model lives on; the trained
    weights are written back into the live parameters (their ``_version`` changes, so fused agents re-pack)."""

    _LOG_GROUP_NAME = "model_train"

    def __init__(self, model, optim_lr: float = 1e-4, weight_decay: float = 1e-5, optim_eps: float = 1e-8, logger=None, *,
                 engine=None, device=None, steps_per_launch: int = 0, extended: bool = False):
        from .engine import get_engine

        self.model = model
        self._kind = _read_model(model, extended)
        self._act, self._slope = self._kind.act, self._kind.slope
        self._train_iteration = 0
        self.logger = logger
        if self.logger:
            self.logger.register_group(self._LOG_GROUP_NAME, MODEL_LOG_FORMAT, color="blue", dump_frequency=1)
        self.engine = engine if engine is not None else get_engine(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.steps_per_launch = int(steps_per_launch)
        dev = self.engine.device
        layers = self._kind.layers
        self._param_device = layers[0][0][0].device
        mse = self._kind.loss == "mse"
        self._out = int(layers[-1][0][0].shape[2]) // (1 if mse else 2)
        E = len(self._kind.mlps) if self._kind.basic else int(layers[0][0][0].shape[0])
        # what the engine is told beyond today's arguments (nothing for one NLL GaussianMLP): the loss kind, per-member bounds and
        # the 1 / E of BasicEnsemble.loss, computed in float32 as torch's backward of `loss / E` computes it
        self._engine_kw = {"loss": "mse"} if mse else {}
        if self._kind.basic and not mse:
            self._engine_kw["bounds_per_member"] = True
        if self._kind.basic and E > 1:
            self._engine_kw["grad_scale"] = float(np.float32(1.0) / np.float32(E))
        # the device copies: a BasicEnsemble's [1, in, out] member tensors stacked into [E, in, out]
        self._w = [[torch.cat([slot[k].detach().to(dev, torch.float32) for slot in slots]).contiguous().clone() for slots in layers]
                   for k in (0, 1)]
        self._m = [[torch.zeros_like(t) for t in ts] for ts in self._w]
        self._v = [[torch.zeros_like(t) for t in ts] for ts in self._w]
        self._step = 0
        self.optimizer = _AdamState(self, self.model.parameters(), optim_lr, weight_decay, optim_eps)
        self._data: Dict[int, Tuple] = {}

    # ---- device copies of the parameters ------------------------------------------------------------------------------
    def _slots(self):
        """(layer, member or None, 0 weight / 1 bias, live parameter) of every trained parameter"""
        for li, slots in enumerate(self._kind.layers):
            for w, b, e in slots:
                yield li, e, 0, w
                yield li, e, 1, b

    @staticmethod
    def _rows(stacked, e):
        """the part of a stacked device tensor one live parameter owns: all of it, or member e's [1, ., .]"""
        return stacked if e is None else stacked[e:e + 1]

    def _pull(self):
        with torch.no_grad():
            for li, e, k, p in self._slots():
                self._rows(self._w[k][li], e).copy_(p.detach())

    def _push(self):
        with torch.no_grad():
            for li, e, k, p in self._slots():
                p.copy_(self._rows(self._w[k][li], e))

    def _bounds(self):
        """DEVICE (min_logvar, max_logvar): [out] of one GaussianMLP, [E, out] of a BasicEnsemble's members, (None, None) under MSE"""
        if self._kind.loss == "mse":
            return None, None
        dev = self.engine.device
        lo = torch.cat([m.min_logvar.detach().reshape(1, -1) for m in self._kind.mlps]).to(dev, torch.float32)
        hi = torch.cat([m.max_logvar.detach().reshape(1, -1) for m in self._kind.mlps]).to(dev, torch.float32)
        if not self._kind.basic:
            lo, hi = lo.reshape(-1), hi.reshape(-1)
        return lo.contiguous(), hi.contiguous()

    def _batch_losses(self, loss_h):
        """The reference's loss of every batch from the per-member losses [S, E] of the device (float32, summed in its order):
        GaussianMLP: sum_e nll_e + 0.01 (sum max_logvar - sum min_logvar) (gaussian_mlp.py:299-304), or sum_e sse_e (:289);
        BasicEnsemble: (sum_e member loss_e) / E with every NLL member's own bound term (basic_ensemble.py:214-221)."""
        mse = self._kind.loss == "mse"
        terms = [np.float32(0.0) if mse else np.float32((0.01 * (m.max_logvar.detach().float().cpu().sum() - m.min_logvar.detach().float().cpu().sum())).item())
                 for m in self._kind.mlps]
        if not self._kind.basic:
            return [float(np.float32(r.sum(dtype=np.float32)) + terms[0]) for r in loss_h]
        out = []
        for r in loss_h:
            acc = np.float32(0.0)
            for e, t in enumerate(terms):
                acc = np.float32(acc + (r[e] if mse else np.float32(r[e] + t)))
            out.append(float(acc / np.float32(len(terms))))
        return out

    def _processed(self, ds):
        """(x [N, in], y [N, out]) on the engine's GPU: the model's own _process_batch over the whole dataset, once per train()."""
        key = id(ds)
        if key not in self._data:
            with torch.no_grad():
                x, y = self.model._process_batch(ds.transitions)
            dev = self.engine.device
            self._data[key] = (x.to(dev, torch.float32).contiguous(), y.to(dev, torch.float32).contiguous())
        return self._data[key]

    # ---- one epoch of minibatch steps -----------------------------------------------------------------------------------
    def _schedule(self, ds):
        """iter(ds) (the reference's draws, exactly where the reference makes them), then the epoch's index schedule:
        idx int32 [n_batches, E, B] and rows int32 [n_batches] (numpy)."""
        kind = _iterator_kind(ds)
        iter(ds)
        E = int(self._w[0][0].shape[0])
        N, B = int(ds.num_stored), int(ds.batch_size)
        n_batches = (N - 1) // B + 1 if N > 0 else 0
        order = np.asarray(ds._order)
        idx = np.zeros((n_batches, E, B), np.int32)
        rows = np.zeros(n_batches, np.int32)
        boot = kind == "bootstrap" and bool(ds._bootstrap_iter)
        mi = np.asarray(ds.member_indices) if boot else None
        if boot and mi.shape[0] != E:
            raise UnsupportedModelError(f"the iterator bootstraps {mi.shape[0]} members, the model has {E}")
        for i in range(n_batches):
            sel = order[i * B:min((i + 1) * B, N)]
            rows[i] = len(sel)
            idx[i, :, :len(sel)] = mi[:, sel] if boot else sel[None, :]
        return idx, rows

    def _run_steps(self, x, y, idx, rows):
        g = self.optimizer.param_groups[0]
        dev = self.engine.device
        if idx.shape[2] > MAX_BATCH:
            raise UnsupportedModelError(f"batch size {idx.shape[2]} > {MAX_BATCH}" + _KEEP_STOCK)
        lo, hi = self._bounds()
        loss, gsq = self.engine.train_steps(
            self._w[0], self._w[1], (self._m[0], self._m[1]), (self._v[0], self._v[1]), lo, hi, x, y,
            torch.from_numpy(np.ascontiguousarray(idx)).to(dev), torch.from_numpy(np.ascontiguousarray(rows)).to(dev), self._step,
            lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], activation=self._act, leaky_slope=self._slope,
            steps_per_launch=self.steps_per_launch, **self._engine_kw)
        self._step += int(idx.shape[0])
        return loss, gsq

    def _epoch(self, ds):
        """Every minibatch step of one pass over ``ds``; returns (loss [S, E], grad_sq [S, E]) DEVICE tensors."""
        if _iterator_kind(ds) is not None:
            x, y = self._processed(ds)
            idx, rows = self._schedule(ds)
            if len(rows) == 0:
                return None, None
            return self._run_steps(x, y, idx, rows)
        losses, gsqs = [], []
        E = int(self._w[0][0].shape[0])
        for batch in ds:  # any other iterable: its batches in Python, every step still a libhipets step
            with torch.no_grad():
                xb, yb = self.model._process_batch(batch)
            dev = self.engine.device
            if xb.ndim == 3:  # [E, B, .]: member e's rows are e * B + b
                nb = int(xb.shape[1])
                idx = (np.arange(E, dtype=np.int32)[:, None] * nb + np.arange(nb, dtype=np.int32)[None, :])[None]
                xb, yb = xb.reshape(-1, xb.shape[-1]), yb.reshape(-1, yb.shape[-1])
            else:
                nb = int(xb.shape[0])
                idx = np.broadcast_to(np.arange(nb, dtype=np.int32), (1, E, nb))
            loss, gsq = self._run_steps(xb.to(dev, torch.float32).contiguous(), yb.to(dev, torch.float32).contiguous(), idx,
                                        np.array([nb], np.int32))
            losses.append(loss)
            gsqs.append(gsq)
        if not losses:
            return None, None
        return torch.cat(losses), torch.cat(gsqs)

    # ---- the reference's trainer logic ----------------------------------------------------------------------------------
    def train(self, dataset_train, dataset_val=None, num_epochs: Optional[int] = None, patience: Optional[int] = None,
              improvement_threshold: float = 0.01, callback: Optional[Callable] = None, batch_callback: Optional[Callable] = None,
              evaluate: bool = True, silent: bool = False) -> Tuple[List[float], List[float]]:
        """As ``mbrl.models.ModelTrainer.train`` (model_trainer.py:70-214)."""
        self._data = {}
        self._pull()
        try:
            return self._train(dataset_train, dataset_val, num_epochs, patience, improvement_threshold, callback, batch_callback, evaluate,
                               silent)
        finally:
            self._data = {}

    def _train(self, dataset_train, dataset_val, num_epochs, patience, improvement_threshold, callback, batch_callback, evaluate, silent):
        eval_dataset = dataset_train if dataset_val is None else dataset_val
        training_losses, val_scores = [], []
        best_weights = None
        epoch_iter = range(num_epochs) if num_epochs else itertools.count()
        epochs_since_update = 0
        best_val_score = self._evaluate(eval_dataset) if evaluate else None
        for epoch in epoch_iter:
            loss, gsq = self._epoch(dataset_train)
            if loss is None:
                batch_losses, grad_norms = [], []
            else:
                loss_h, gsq_h = loss.cpu().numpy(), gsq.cpu().numpy()  # the epoch's one synchronisation
                batch_losses = self._batch_losses(loss_h)
                grad_norms = [float(r.astype(np.float64).sum()) for r in gsq_h]
            if batch_callback:
                for bl, gn in zip(batch_losses, grad_norms):
                    batch_callback(epoch, bl, {"grad_norm": gn}, "train")
            total_avg_loss = np.mean(batch_losses).mean().item()
            training_losses.append(total_avg_loss)

            eval_score = None
            model_val_score = 0
            if evaluate:
                eval_score = self._evaluate(eval_dataset, batch_callback=(lambda *a: batch_callback(epoch, *a)) if batch_callback else None)
                val_scores.append(eval_score.mean().item())
                maybe_best_weights = self.maybe_get_best_weights(best_val_score, eval_score, improvement_threshold)
                if maybe_best_weights:
                    best_val_score = torch.minimum(best_val_score, eval_score)
                    best_weights = maybe_best_weights
                    epochs_since_update = 0
                else:
                    epochs_since_update += 1
                model_val_score = eval_score.mean()

            if self.logger and not silent:
                self.logger.log_data(self._LOG_GROUP_NAME, {
                    "iteration": self._train_iteration,
                    "epoch": epoch,
                    "train_dataset_size": dataset_train.num_stored,
                    "val_dataset_size": dataset_val.num_stored if dataset_val is not None else 0,
                    "model_loss": total_avg_loss,
                    "model_val_score": model_val_score,
                    "model_best_val_score": best_val_score.mean() if best_val_score is not None else 0,
                })
            if callback:
                self._push()  # the callback sees the model as the reference's would
                callback(self.model, self._train_iteration, epoch, total_avg_loss, eval_score, best_val_score)
            if patience and epochs_since_update >= patience:
                break

        if evaluate:
            self._maybe_set_best_weights_and_elite(best_weights, best_val_score)
        self._push()
        self._train_iteration += 1
        return training_losses, val_scores

    def evaluate(self, dataset, batch_callback: Optional[Callable] = None) -> torch.Tensor:
        """As ``mbrl.models.ModelTrainer.evaluate`` (model_trainer.py:216-262): the per-member mean squared error of the means."""
        outside = not self._data
        if outside:
            self._pull()
        try:
            return self._evaluate(dataset, batch_callback)
        finally:
            if outside:
                self._data = {}

    def _evaluate(self, dataset, batch_callback=None) -> torch.Tensor:
        kind = _iterator_kind(dataset)
        if kind == "bootstrap":
            dataset.toggle_bootstrap()
        dev = self.engine.device
        E = int(self._w[0][0].shape[0])
        if kind is not None:
            x, y = self._processed(dataset)
            iter(dataset)  # the reference's `for batch in dataset`: a shuffling iterator draws its order here
            N, B = int(dataset.num_stored), int(dataset.batch_size)
            order = torch.from_numpy(np.asarray(dataset._order, dtype=np.int32)).to(dev)
            sizes = [min(B, N - s) for s in range(0, N, B)]
        else:
            xs, ys, sizes = [], [], []
            for batch in dataset:
                with torch.no_grad():
                    xb, yb = self.model._process_batch(batch)
                if xb.ndim != 2:
                    raise UnsupportedModelError("evaluate needs 2-D batches (GaussianMLP.eval_score)" + _KEEP_STOCK)
                xs.append(xb)
                ys.append(yb)
                sizes.append(int(xb.shape[0]))
            x = torch.cat(xs).to(dev, torch.float32).contiguous()
            y = torch.cat(ys).to(dev, torch.float32).contiguous()
            order = None
        res = self.engine.train_eval(self._w[0], self._w[1], x, y, order, activation=self._act, leaky_slope=self._slope,
                                     row_scores=batch_callback is not None, **({"loss": "mse"} if self._kind.loss == "mse" else {}))
        score, rs = res if batch_callback is not None else (res, None)
        if batch_callback is not None:
            rs_h = rs.cpu().numpy()
            start = 0
            for n in sizes:  # batch_score.mean() of every batch in iteration order (model_trainer.py:245-246)
                batch_callback(torch.tensor(rs_h[:, start:start + n].sum(dtype=np.float64) / (E * n * self._out), dtype=torch.float32), {}, "eval")
                start += n
        if kind == "bootstrap":
            dataset.toggle_bootstrap()
        return score.to(self._param_device)

    def maybe_get_best_weights(self, best_val_score: torch.Tensor, val_score: torch.Tensor, threshold: float = 0.01) -> Optional[Dict]:
        """As the reference (model_trainer.py:264-286), with the snapshot a device copy of the trained parameters."""
        improvement = (best_val_score - val_score) / torch.abs(best_val_score)
        improved = (improvement > threshold).any().item()
        return {"weights": [t.clone() for t in self._w[0]], "biases": [t.clone() for t in self._w[1]]} if improved else None

    def _maybe_set_best_weights_and_elite(self, best_weights: Optional[Dict], best_val_score: torch.Tensor):
        if best_weights is not None:
            for li in range(len(self._kind.layers)):
                self._w[0][li].copy_(best_weights["weights"][li])
                self._w[1][li].copy_(best_weights["biases"][li])
        if len(best_val_score) > 1 and hasattr(self.model, "num_elites"):
            sorted_indices = np.argsort(best_val_score.tolist())
            elite_models = sorted_indices[: self.model.num_elites]
            self.model.set_elite(elite_models)


def make_model_trainer(model, optim_lr: float = 1e-4, weight_decay: float = 1e-5, optim_eps: float = 1e-8, logger=None, **kw):
    """The trainer's analogue of ``make_eval_fn``: ``hipets.ModelTrainer(model, ..., extended=True, **kw)`` where the model trains
    in HIP (one GaussianMLP, NLL or deterministic; a BasicEnsemble of one-member GaussianMLPs); for any other model
    ``mbrl.models.ModelTrainer(model, ...)`` with one warning that names the reason, or, where mbrl cannot be imported, the
    UnsupportedModelError itself."""
    try:
        return ModelTrainer(model, optim_lr=optim_lr, weight_decay=weight_decay, optim_eps=optim_eps, logger=logger, extended=True, **kw)
    except UnsupportedModelError as exc:
        try:
            import mbrl.models as stock
        except ImportError:
            raise exc from None
        warnings.warn(f"hipets.make_model_trainer: training with mbrl.models.ModelTrainer ({str(exc).replace(_KEEP_STOCK, '')})", stacklevel=2)
        return stock.ModelTrainer(model, optim_lr=optim_lr, weight_decay=weight_decay, optim_eps=optim_eps, logger=logger)
