"""What the dynamics ensemble predicts, and how much its members disagree, on the device: ``GaussianMLP.forward(x,
use_propagation=False)`` (mbrl/models/gaussian_mlp.py:140-154, 277-281; ``BasicEnsemble._default_forward``, basic_ensemble.py:94-99)
behind ``OneDTransitionRewardModel``'s model input (one_dim_tr_model.py:103-116), as one HIP launch over all members
(hipets_ensemble_predict), and the uncertainty penalty of pessimistic model rollouts built on its statistics (MOPO's ``r - lambda u``,
MOReL's halt):

    predictor = hipets.EnsemblePredictor(model_env)
    mean, logvar = predictor.forward(model_in)                 # [E, B, out] each: model.forward(x, use_propagation=False)
    stats = predictor.uncertainty(obs, act)                    # [B, 4]: max_std, disagreement, total_std, max_deviation
    hipets.rollout_model_and_populate_sac_buffer(..., uncertainty=hipets.UncertaintyPenalty("max_std", coef=1.0))
"""
from __future__ import annotations

import math
import types
from dataclasses import dataclass
from typing import Optional

import torch

from ._lib import ENSEMBLE_STATS
from ._pack import check_ensemble_shape
from .model import ModelSpec, ObsColumns, UnsupportedModelError, model_version, spec_from_model_env
from .sac import _SlotOwner


@dataclass(frozen=True)
class UncertaintyPenalty:
    """``reward -= coef * u`` with ``u`` one of the ensemble's statistics (``kind``: 'max_std' -- MOPO's largest predicted std over the
    members --, 'disagreement', 'total_std' or 'max_deviation'; hipets_ensemble_predict), over the elite members (``only_elite``) or
    all.  ``halt_threshold``: rows with ``u`` above it are done (MOReL's halt) and, with ``halt_reward``, get that reward instead."""

    kind: str = "max_std"
    coef: float = 1.0
    halt_threshold: Optional[float] = None
    halt_reward: Optional[float] = None
    only_elite: bool = True

    def __post_init__(self):
        if self.kind not in ENSEMBLE_STATS:
            raise ValueError(f"UncertaintyPenalty kind {self.kind!r} is not one of {ENSEMBLE_STATS}")
        for name in ("coef", "halt_threshold", "halt_reward"):
            v = getattr(self, name)
            if v is None and name != "coef":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or (name != "halt_reward" and math.isinf(v)):
                raise ValueError(f"UncertaintyPenalty {name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if self.halt_reward is not None and self.halt_threshold is None:
            raise ValueError("UncertaintyPenalty halt_reward needs a halt_threshold")
        object.__setattr__(self, "only_elite", bool(self.only_elite))

    @property
    def stat(self) -> int:
        """column of the statistics the penalty reads"""
        return ENSEMBLE_STATS.index(self.kind)


def _unused_fn(act, next_obs):  # stands where a bare dynamics model has no reward / termination function: the predictor reads neither
    raise NotImplementedError


def _as_model_env(dm):
    """A ``OneDTransitionRewardModel`` dressed as the ModelEnv ``spec_from_model_env`` reads: its widths come from the model itself."""
    mlp = dm.model
    first = mlp.members[0] if hasattr(mlp, "members") and not hasattr(mlp, "hidden_layers") else mlp
    out = int(first.mean_and_logvar.weight.shape[-1]) // (1 if getattr(first, "deterministic", False) else 2)
    in_dim = int((first.hidden_layers[0][0] if len(first.hidden_layers) else first.mean_and_logvar).weight.shape[-2])
    obs_dim = out - (1 if dm.learned_rewards else 0)
    fn = getattr(dm, "obs_process_fn", None)
    obs_in = len(fn.columns) if isinstance(fn, ObsColumns) else (obs_dim if fn is None else int(fn(torch.zeros(1, obs_dim)).shape[-1]))
    box = lambda n: types.SimpleNamespace(shape=(n,))  # noqa: E731
    return types.SimpleNamespace(dynamics_model=dm, reward_fn=_unused_fn, termination_fn=_unused_fn, observation_space=box(obs_dim),
                                 action_space=box(in_dim - obs_in), device=getattr(dm, "device", None))


class EnsemblePredictor(_SlotOwner):
    """All members' predictions for a batch, and their uncertainty statistics, on the ensemble kernel.  ``model``: what
    ``hipets.ModelEnv`` accepts -- a live ``mbrl.models.ModelEnv`` (or a ``hipets.ModelEnv`` over one), a ``ModelSpec`` -- or a bare
    ``OneDTransitionRewardModel``.  A model the kernel does not cover (bf16 precisions, more than 16 members, widths past the limits)
    raises UnsupportedModelError here.  The engine holds a SNAPSHOT: it is taken again when ``model_version`` says the live model was
    trained in between, or when another predictor's model sits in the engine."""
    slot = "ensemble"

    def __init__(self, model, engine=None, device=None):
        if hasattr(model, "_eval") and hasattr(model, "spec"):  # a hipets.ModelEnv: the model it was built from
            engine = engine if engine is not None else model.engine
            model = model._eval._live if model._eval._live is not None else model.spec
        self._live = self._version = None
        if isinstance(model, ModelSpec):
            self.spec = model
        else:
            self._live = model if hasattr(model, "dynamics_model") else _as_model_env(model)
            self.spec = self._read()
            self._version = model_version(self._live)
        self.spec.validate()
        check_ensemble_shape(self.spec)  # (before anything touches a device)
        if engine is None:
            from .engine import get_engine

            engine = get_engine(device if device is not None else (getattr(self._live, "device", None) or "cuda:0"))
        self.engine, self.device = engine, engine.device
        self._set()

    def _read(self) -> ModelSpec:
        return spec_from_model_env(self._live, allow_custom_fns=True, propagation="random_model")  # (a forward reads no propagation)

    def _set(self):
        self.engine.ensemble_set(self.spec)
        self.claim()

    def refresh(self, force: bool = False):
        """Re-take the snapshot if the live model changed (ModelTrainer.train, hipets.ModelTrainer) or another owner holds the slot."""
        moved = False
        if self._live is not None:
            v = model_version(self._live)
            if force or v != self._version:
                self.spec, self._version, moved = self._read(), v, True
                check_ensemble_shape(self.spec)
        if moved or force or not self.owns() or self.engine.ensemble_spec is not self.spec:
            self._set()

    def _dev(self, t) -> torch.Tensor:
        return torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous()

    def predict(self, obs, act, only_elite: bool = False):
        """(mean [n, B, out_dim], logvar [n, B, out_dim] or None for a deterministic model) of raw ``obs`` [B, obs_dim] / ``act`` [B,
        act_dim]: the model's own obs_process, concatenation and normaliser, then every member's forward."""
        self.refresh()
        mean, logvar, _ = self.engine.ensemble_predict(self._dev(obs), self._dev(act), only_elite=only_elite, logvar=not self.spec.deterministic)
        return mean, logvar

    def forward(self, model_in, only_elite: bool = False):
        """``model.forward(x, use_propagation=False)`` for a ready model input ``x`` [B, in_dim]: (mean, logvar | None), [n, B, out_dim]."""
        self.refresh()
        mean, logvar, _ = self.engine.ensemble_predict(model_in=self._dev(model_in), only_elite=only_elite, logvar=not self.spec.deterministic)
        return mean, logvar

    def uncertainty(self, obs, act, only_elite: bool = True) -> torch.Tensor:
        """stats f32 [B, 4] -- max_std, disagreement, total_std, max_deviation (hipets_ensemble_predict) -- of raw ``obs`` / ``act``,
        reduced over the members inside the launch: no [n, B, out_dim] tensor is written."""
        self.refresh()
        return self.engine.ensemble_predict(self._dev(obs), self._dev(act), only_elite=only_elite, mean=False, logvar=False, stats=True)[2]

    def geometry(self, batch: int):
        """(row tiles per workgroup, dynamic LDS bytes) of a launch over ``batch`` rows"""
        self.refresh()
        return self.engine.ensemble_geometry(batch)

    def penalise(self, penalty: UncertaintyPenalty, obs: torch.Tensor, act: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor):
        """One statistics launch on the step's (``obs``, ``act``) and one penalty launch on its ``rewards`` f32 [B] / ``dones`` (bool or
        uint8 [B]), both updated in place."""
        stats = self.uncertainty(obs, act, only_elite=penalty.only_elite)
        self.engine.uncertainty_penalty(stats, penalty.stat, penalty.coef, rewards, dones, halt_threshold=penalty.halt_threshold,
                                        halt_reward=penalty.halt_reward)
        return stats


def reference_statistics(mean: torch.Tensor, logvar: Optional[torch.Tensor]) -> torch.Tensor:
    """The four statistics of hipets_ensemble_predict from ``mean`` / ``logvar`` [n, B, out_dim] with torch ops (any device): what the
    reference loop's penalty uses where the kernel does not cover the model."""
    var_m = mean.var(dim=0, unbiased=False).sum(-1)
    ev = logvar.exp().sum(-1) if logvar is not None else torch.zeros_like(mean[..., 0])
    dev = (mean - mean[:1]).pow(2).sum(-1).sqrt()
    return torch.stack([ev.sqrt().max(dim=0).values, var_m.sqrt(), (var_m + ev.mean(dim=0)).sqrt(), dev.max(dim=0).values], dim=-1)


class ReferencePenalisedEnv:
    """A live ``mbrl.models.ModelEnv`` whose ``step`` applies ``penalty`` with the reference's own torch forward
    (``dynamics_model.model.forward(x, use_propagation=False)`` over ``_get_model_input``): the environment of the reference loop where
    the ensemble kernel does not cover the model.  reset / step as the reference's, numpy in and out."""

    def __init__(self, model_env, penalty: UncertaintyPenalty):
        self.env, self.penalty = model_env, penalty

    def reset(self, *args, **kwargs):
        return self.env.reset(*args, **kwargs)

    @torch.no_grad()
    def step(self, actions, model_state, sample: bool = False):
        import numpy as np

        dm, p = self.env.dynamics_model, self.penalty
        obs = model_state["obs"]
        act_t = torch.as_tensor(np.asarray(actions), dtype=torch.float32, device=obs.device)
        mean, logvar = dm.model.forward(dm._get_model_input(obs, act_t), use_propagation=False)
        elite = getattr(dm.model, "elite_models", None)
        if p.only_elite and elite is not None:
            mean, logvar = mean[list(elite)], (None if logvar is None else logvar[list(elite)])
        u = reference_statistics(mean.float(), None if logvar is None else logvar.float())[:, p.stat].cpu().numpy()
        nobs, rew, done, state = self.env.step(actions, model_state, sample=sample)
        rew = np.asarray(rew, dtype=np.float32).copy()
        done = np.asarray(done).copy()
        rew[:, 0] = rew[:, 0] - np.float32(p.coef) * u
        if p.halt_threshold is not None:
            halted = u > np.float32(p.halt_threshold)
            done[halted, 0] = True
            if p.halt_reward is not None:
                rew[halted, 0] = np.float32(p.halt_reward)
        return nobs, rew, done, state
