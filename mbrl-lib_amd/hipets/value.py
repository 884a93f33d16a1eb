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

import weakref
from typing import Optional

import numpy as np
import torch

from ._pack import check_critic_split, check_discount, pack_critic
from .mbpo import SACActor
from .model import PlaNetSpec, UnsupportedModelError, is_planet_model
from .objectives import CallableTrajectoryEvalFn


def find_critic(agent, target: bool = False):
    """The critic module of an ``mbrl.planning.SACAgent`` (``.sac_agent.critic``), a ``pytorch_sac_pranz24.SAC`` (``.critic``) -- their
    ``critic_target`` with ``target`` -- or a bare ``QNetwork``-shaped module."""
    inner = getattr(agent, "sac_agent", agent)
    name = "critic_target" if target else "critic"
    module = getattr(inner, name, None)
    if module is not None:
        return module
    if getattr(inner, "linear1", None) is not None:  # a bare module (it has no target of its own)
        return inner
    raise UnsupportedModelError(f"{type(agent).__name__} has no {name}: expected an mbrl SACAgent, a pytorch_sac_pranz24 SAC or a QNetwork-shaped module")


class _Snapshot:
    """When was a module's snapshot in an engine taken?  ``moved()``: a watched parameter's ``_version`` changed (a stock optimizer
    step, a ``load_state_dict``), or the engine ran ``sac_update`` since (its kernels write parameters through raw pointers: no version
    moves).  ``watch``: further modules whose parameters are watched too -- for a ``critic_target`` the live ``critic``: the stock
    agent writes its target as ``target_param.data.copy_(...)`` (pytorch_sac_pranz24/utils.py:28, 33), which moves no version of the
    target's, but every such write follows a ``critic_optim.step()``, which moves the critic's."""

    def __init__(self, module, engine, watch=()):
        self.modules, self.engine = (module,) + tuple(m for m in watch if m is not None and m is not module), engine
        self.mark()

    def _state(self):
        return tuple(int(p._version) for m in self.modules for p in m.parameters()), self.engine.sac_updates

    def mark(self):
        self.state = self._state()

    def moved(self) -> bool:
        return self.state != self._state()


class SACCritic:
    """``QNetwork.forward`` (pytorch_sac_pranz24/model.py:36-61) on the critic kernel (hipets_critic_q).  ``agent``: an
    ``mbrl.planning.SACAgent``, a ``pytorch_sac_pranz24.SAC`` or a bare ``QNetwork``-shaped module (linear1..3 = Q1, linear4..6 = Q2);
    ``target``: the agent's ``critic_target``.  Anything else raises UnsupportedModelError with the reason.  The engine holds a SNAPSHOT
    of the weights: ``refresh()`` after the critic changed (``stale()`` tells; for a target it also watches the agent's live
    ``critic``, whose optimizer step precedes every stock soft update).  ``obs_dim``: where the critic's input splits into state and
    action; by default read off the agent's policy, else fixed by the first ``q`` call."""

    def __init__(self, agent, engine=None, target: bool = False, obs_dim: Optional[int] = None):
        self.critic = find_critic(agent, target)
        (self.K, self.hidden), tensors = pack_critic(self.critic)
        if obs_dim is None:
            l1 = getattr(getattr(getattr(agent, "sac_agent", agent), "policy", None), "linear1", None)
            if getattr(l1, "weight", None) is not None and l1.weight.ndim == 2:
                obs_dim = int(l1.weight.shape[1])
        self.split = None
        if obs_dim is not None:
            check_critic_split(self.K, int(obs_dim), self.K - int(obs_dim))
            self.split = (int(obs_dim), self.K - int(obs_dim))
        if engine is None:
            from .engine import get_engine

            p = tensors[0]
            engine = get_engine(p.device if p.device.type == "cuda" else "cuda")
        self.engine, self.device = engine, engine.device
        live = getattr(getattr(agent, "sac_agent", agent), "critic", None) if target else None
        self._snapshot = _Snapshot(self.critic, engine, watch=(live,) if isinstance(live, torch.nn.Module) else ())
        if self.split is not None:
            self.refresh()

    @property
    def dims(self):
        """(obs_dim, act_dim, hidden); the first two are None until the split is known"""
        return (self.split or (None, None)) + (self.hidden,)

    def refresh(self):
        """Re-snapshot the critic's live weights (device to device where the critic is on the engine's GPU)."""
        if self.split is None:
            raise ValueError("the critic's state / action split is not known yet: pass obs_dim=, or call q(obs, actions) once")
        self.engine.critic_set(self.critic, *self.split)
        self.engine.critic_owner = weakref.ref(self)
        self._snapshot.mark()

    def owns_engine(self) -> bool:
        owner = self.engine.critic_owner
        return owner is not None and owner() is self

    def stale(self) -> bool:
        """Does the engine's snapshot differ from the live critic as far as can be told without reading it: a parameter's version
        moved, the engine ran a SAC update since, or another critic sits in the engine's slot?"""
        return not self.owns_engine() or self._snapshot.moved()

    def q(self, obs_t: torch.Tensor, act_t: torch.Tensor, q1: bool = True, q2: bool = True, qmin: bool = True):
        """``obs_t`` f32 [B, obs_dim], ``act_t`` f32 [B, act_dim] on the device -> (q1, q2, qmin) f32 [B] on the device (one not
        wanted is None); qmin = torch.min(q1, q2)."""
        if not isinstance(obs_t, torch.Tensor) or not isinstance(act_t, torch.Tensor) or obs_t.ndim != 2 or act_t.ndim != 2:
            raise ValueError("obs / actions must be [B, obs_dim] / [B, act_dim] tensors")
        split = (int(obs_t.shape[1]), int(act_t.shape[1]))
        if self.split is None:
            check_critic_split(self.K, *split)
            self.split = split
        if split != self.split:
            raise ValueError(f"obs / actions must be [B, {self.split[0]}] / [B, {self.split[1]}], got {tuple(obs_t.shape)} / {tuple(act_t.shape)}")
        if not self.owns_engine():  # (another critic's weights sit in the engine)
            self.refresh()
        return self.engine.critic_q(obs_t, act_t, q1=q1, q2=q2, qmin=qmin)


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
        self.actor = self.critic = self._actor_snapshot = None
        if agent is not None:
            self.actor = SACActor(agent, engine=self.engine)
            self.critic = SACCritic(agent, engine=self.engine, target=target_critic, obs_dim=self.spec.obs_dim)
            if self.actor.dims[0] != self.spec.obs_dim or self.actor.dims[2] != self.spec.act_dim or self.critic.split[1] != self.spec.act_dim:
                raise ValueError(f"the agent acts on (obs {self.actor.dims[0]}, act {self.actor.dims[2]}), its critic on (obs {self.critic.split[0]}, "
                                 f"act {self.critic.split[1]}); the model has (obs {self.spec.obs_dim}, act {self.spec.act_dim})")
            self._actor_snapshot = _Snapshot(self.actor.policy, self.engine)

    def refresh_agent(self, force: bool = True):
        """Re-snapshot the actor's and the critic's live weights; ``force=False``: only what may have changed (the class docstring)."""
        if self.actor is None:
            return
        owner = getattr(self.engine, "policy_owner", None)
        if force or owner is None or owner() is not self.actor or self._actor_snapshot.moved():
            self.actor.refresh()
            self._actor_snapshot.mark()
        if force or self.critic.stale():
            self.critic.refresh()

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
