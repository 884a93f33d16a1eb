"""Value-bootstrapped planning: a candidate's worth as ``sum_t gamma^t r_t + gamma^H min(Q1, Q2)(s_H, pi(s_H))``, the SAC agent's
critic closing a short planning horizon (POLO / LOOP / TD-MPC style), on the device.

    critic = hipets.SACCritic(sac_agent)                                  # QNetwork.forward as one HIP launch
    q1, q2, qmin = critic.q(obs_t, act_t)
    fn = hipets.make_eval_fn(model_env, num_particles, terminal_value=sac_agent, discount=0.99)
    agent.set_trajectory_eval_fn(fn)                                      # any optimizer, through its per-iteration loop

One evaluation is one traced rollout, the rewards and terminations of :class:`CallableTrajectoryEvalFn`, one actor launch (the mean
action) on the last predicted states, one critic launch and one ``hipets_discounted_returns`` launch.  The engine holds SNAPSHOTS of
the actor and the critic; the objective re-takes them when the agent changed (see :class:`ValueTrajectoryEvalFn`).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._pack import check_discount
from .model import PlaNetSpec, is_planet_model
from .objectives import CallableTrajectoryEvalFn
from .sac import SACActor, SACCritic, _Snapshot, find_critic  # noqa: F401  (their home before hipets.sac)


class ValueTrajectoryEvalFn(CallableTrajectoryEvalFn):
    """``trajectory_eval_fn`` whose candidates are worth ``sum_t discount^t r_t + discount^H min(Q1, Q2)(s_H, pi(s_H))``: the
    undiscounted objective of ``ModelEnv.evaluate_action_sequences`` (model_env.py:145-191) with a discount and the SAC agent's critic
    at the mean action of its actor as the tail.  ``agent``: what :class:`SACCritic` and ``hipets.SACActor`` take (it needs both a
    Gaussian policy and a critic); ``None`` gives discounting alone.  ``target_critic``: bootstrap from ``critic_target``.

    Rewards and terminations are :class:`CallableTrajectoryEvalFn`'s: the callables where given (``reward_fn`` / ``termination_fn``, or
    the spec's custom ones; they must be row-wise), else the kernel's own reward and the closed-form termination restated over the
    traced states.  A row that terminated at any step gets no bootstrap.  ``mode``, seed, streams and ``particle_reduce`` as for every
    rollout objective; with ``discount=1`` and no agent the returns are :class:`HipTrajectoryEvalFn`'s bits.  Not a fused-plan target
    (``kernel_mode`` is None): the optimizers run their per-iteration loops and call it; the batched agents refuse it.  No host
    synchronisation in the in-kernel modes.

    The engine holds snapshots of the actor and the critic.  Before every call the objective re-takes one when a parameter's
    ``_version`` moved (a stock optimizer step; with ``target_critic`` the live critic's parameters count too, since the stock soft
    update writes the target through ``.data``), when the engine ran ``sac_update`` since (``SACUpdater``'s kernels write through raw
    pointers and move no version), or when another owner sits in the engine's slot; :meth:`refresh_agent` forces both."""

    _needs_callable = False

    def __init__(self, model, num_particles: int, agent=None, discount: float = 1.0, target_critic: bool = False, reward_fn=None,
                 termination_fn=None, engine=None, mode: str = "device", seed: int = 0, device=None, rng: Optional[torch.Generator] = None,
                 check_rowwise: bool = True, max_trajectory_bytes: int = 2 << 30, particle_reduce=None):
        self.discount = check_discount(discount)
        if isinstance(model, PlaNetSpec) or is_planet_model(getattr(model, "dynamics_model", model)):
            raise ValueError("value-bootstrapped objectives are not available for PlaNet latent models (no critic over latent states)")
        super().__init__(model, num_particles, reward_fn, termination_fn, engine, mode, seed, device, rng, check_rowwise, max_trajectory_bytes,
                         particle_reduce)
        self.actor = self.critic = None
        if agent is not None:
            self.actor = SACActor(agent, engine=self.engine)
            self.critic = SACCritic(agent, engine=self.engine, target=target_critic, obs_dim=self.spec.obs_dim)
            if self.actor.dims[0] != self.spec.obs_dim or self.actor.dims[2] != self.spec.act_dim or self.critic.split[1] != self.spec.act_dim:
                raise ValueError(f"the agent acts on (obs {self.actor.dims[0]}, act {self.actor.dims[2]}), its critic on (obs {self.critic.split[0]}, "
                                 f"act {self.critic.split[1]}); the model has (obs {self.spec.obs_dim}, act {self.spec.act_dim})")

    def refresh_agent(self, force: bool = True):
        """Re-snapshot the actor's and the critic's live weights; ``force=False``: only what may have changed (the class docstring)."""
        if self.actor is None:
            return
        for part in (self.actor, self.critic):
            if force or part.stale():
                part.refresh()

    def _terminal(self, next_obs: torch.Tensor):
        """(terminal_actions [B, act], terminal_values [B]) on the last predicted states, or (None, None) without an agent"""
        if self.actor is None:
            return None, None
        self.refresh_agent(force=False)
        last = next_obs[-1]
        actions = self.actor.act_device(last, sample=False)
        return actions, self.critic.q(last, actions, q1=False, q2=False)[2]

    def _trajectory(self, initial_state, action_sequences, details):
        a = self._prep(action_sequences)
        self.calls += 1
        pop, P = a.shape[0], self.num_particles
        next_obs, rewards, dones = self._rewards_and_dones(a, initial_state)
        actions, values = self._terminal(next_obs)
        if not details:
            return self.engine.discounted_returns(rewards, dones, pop, P, gamma=self.discount, terminal_values=values)
        returns, row_totals, first_done = self.engine.discounted_returns(rewards, dones, pop, P, gamma=self.discount, terminal_values=values,
                                                                         row_totals=True, first_done=True)
        return {"next_obs": next_obs, "rewards": rewards, "dones": dones, "first_done": first_done, "row_totals": row_totals, "returns": returns,
                "terminal_actions": actions, "terminal_values": values}

    def trajectories(self, initial_state: np.ndarray, action_sequences: torch.Tensor):
        """:meth:`_RolloutObjective.trajectories`' keys -- ``row_totals`` and ``returns`` discounted and bootstrapped -- plus
        ``terminal_actions`` [B, act] (the actor's mean action on ``next_obs[-1]``) and ``terminal_values`` [B] (min(Q1, Q2) there, before
        the discount and the termination select); both None without an agent."""
        return self._trajectory(initial_state, action_sequences, True)
