"""Policy-guided planning (LOOP, TD-MPC): the learned SAC policy rolled through the learned model, and its action sequences as
candidates of every planning iteration.

    rollout = hipets.PolicyRollout(model_env, sac_agent)
    actions = rollout.sequences(obs, n=24, horizon=10, mean_rows=1)        # [24, 10, A]: one launch (hipets_policy_rollout)
    agent.set_policy_prior(hipets.PolicyPrior(model_env, sac_agent, num=24))  # a TrajectoryOptimizerAgent: 24 rows of every population

A step of a row is ``GaussianPolicy`` on its state (``SACActor``'s kernel arithmetic), then the ensemble's expected next observation
(``ModelEnv.step(..., sample=False)`` under ``propagation_method="expectation"``: the mean over the members of their mean heads, the
delta rule of ``OneDTransitionRewardModel``).  No termination test: the objective that evaluates a sequence applies its own.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .ensemble import EnsemblePredictor
from .sac import SACActor


def _check_prior_args(num, mean_rows):
    if isinstance(num, bool) or not isinstance(num, (int, np.integer)) or num < 1:
        raise ValueError(f"num must be an integer >= 1, got {num!r}")
    if isinstance(mean_rows, bool) or not isinstance(mean_rows, (int, np.integer)) or not 0 <= mean_rows <= num:
        raise ValueError(f"mean_rows must be an integer in [0, {num}], got {mean_rows!r}")


class PolicyRollout:
    """The actor of ``agent`` (what :class:`hipets.SACActor` accepts) rolled through the dynamics ensemble of ``model`` (what
    :class:`hipets.EnsemblePredictor` accepts: a ModelEnv, a ``ModelSpec``, a bare ``OneDTransitionRewardModel``).  The engine holds
    SNAPSHOTS of both; before every call what went stale is taken again -- the agent's parameters moved, the engine ran a
    ``sac_update``, the model was trained, or another owner sits in a slot.  ``only_elite``: average the model's elite members (all
    where it has none)."""

    def __init__(self, model, agent, engine=None, only_elite: bool = True, seed: int = 0):
        self.predictor = EnsemblePredictor(model, engine=engine)
        self.engine = self.predictor.engine
        self.actor = SACActor(agent, engine=self.engine, seed=seed)
        self.device, self.only_elite, self.seed = self.engine.device, bool(only_elite), int(seed)
        obs, _, act = self.actor.dims
        spec = self.predictor.spec
        if (obs, act) != (spec.obs_dim, spec.act_dim):
            raise ValueError(f"the policy's (obs {obs}, act {act}) differs from the model's (obs_dim {spec.obs_dim}, act_dim {spec.act_dim})")
        self.obs_dim, self.act_dim = obs, act
        self.calls = 0

    def refresh(self):
        """Re-take the snapshots that went stale (``_Snapshot.stale`` for the actor, ``EnsemblePredictor.refresh`` for the model)."""
        if self.actor.stale():
            self.actor.refresh()
        self.predictor.refresh()

    def geometry(self, n: int):
        """(row tiles per workgroup, dynamic LDS bytes) of a launch over ``n`` rows"""
        self.refresh()
        return self.engine.policy_rollout_geometry(n)

    def sequences(self, obs, n: Optional[int] = None, horizon: int = 1, mean_rows: int = 0, eps: Optional[torch.Tensor] = None,
                  stream_id: Optional[int] = None, return_states: bool = False):
        """actions f32 [n, horizon, A] on the device (with ``return_states`` also the visited states [horizon + 1, n, obs_dim]) from
        ``obs`` -- [obs_dim], broadcast to ``n`` rows, or [n, obs_dim]; numpy or a tensor.  Rows below ``mean_rows`` take the mean
        action, the others sample: with ``eps`` [horizon, n, A], else drawn in-kernel under (seed, ``stream_id``; None: the number of
        calls so far).  Nothing here waits for the device."""
        s0 = torch.as_tensor(obs).to(device=self.device, dtype=torch.float32)
        if s0.ndim == 1:
            s0 = s0.unsqueeze(0).expand(1 if n is None else int(n), -1)
        if s0.ndim != 2 or int(s0.shape[1]) != self.obs_dim or (n is not None and int(s0.shape[0]) != int(n)):
            raise ValueError(f"obs must be [{self.obs_dim}] or [n, {self.obs_dim}], got {tuple(s0.shape)} with n = {n}")
        rows = int(s0.shape[0])
        if not 0 <= int(mean_rows) <= rows:
            raise ValueError(f"mean_rows must be in [0, {rows}], got {mean_rows}")
        self.calls += 1
        self.refresh()
        return self.engine.policy_rollout(s0.contiguous(), int(horizon), mean_rows=int(mean_rows), only_elite=self.only_elite, seed=self.seed,
                                          stream_id=self.calls if stream_id is None else int(stream_id), eps=eps, states=return_states)


class PolicyPrior:
    """The policy's share of a plan's population, for ``TrajectoryOptimizerAgent.set_policy_prior``: per plan ``num`` action
    sequences of :class:`PolicyRollout` from the plan's observation -- ``mean_rows`` of them the mean policy, the others sampled
    (``sample=False``: all of them the mean policy, i.e. ``num`` equal rows) -- drawn under (``seed``, the number of plans so far)."""

    def __init__(self, model_env, agent, num: int = 24, sample: bool = True, mean_rows: int = 1, only_elite: bool = True, seed: int = 0,
                 engine=None):
        _check_prior_args(num, mean_rows)
        self.num, self.sample, self.mean_rows = int(num), bool(sample), int(mean_rows)
        self.rollout = PolicyRollout(model_env, agent, engine=engine, only_elite=only_elite, seed=seed)
        self.plans = 0

    def sequences(self, obs, horizon: int) -> torch.Tensor:
        """[num, horizon, A] on the device for the plan that starts at ``obs``"""
        self.plans += 1
        return self.rollout.sequences(obs, n=self.num, horizon=horizon, mean_rows=self.mean_rows if self.sample else self.num,
                                      stream_id=self.plans)
