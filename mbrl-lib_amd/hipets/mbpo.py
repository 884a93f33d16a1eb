"""MBPO's agent side on the device (mbrl/algorithms/mbpo.py): the model rollouts into the SAC buffer (:31-63) -- the SAC actor as one HIP
launch, the model step as the existing ``hipets_step`` launch, and a compaction of the step's live rows into a device staging area,
three plainly ordered pieces per rollout step, one device -> host copy per call -- and SAC's updates (:258-275), a fixed sequence of HIP
launches per update that works in place on the agent's live torch tensors.  With a ``hipets.DeviceReplayBuffer`` as the SAC buffer the
rows never leave the device: the populate compacts straight into its ring, the updates gather their batches from it in one launch.

    agent = hipets.SACActor(sac_agent)                    # drop-in for SACAgent.act, numpy in / numpy out
    hipets.rollout_model_and_populate_sac_buffer(model_env, replay_buffer, sac_agent, sac_buffer, True, rollout_length, batch_size)
    updater = hipets.make_sac_updater(sac_agent)          # drop-in for sac_agent.sac_agent.update_parameters
    updater.update_parameters(which_buffer, batch_size, updates_made, logger, reverse_mask=True)
    sac_buffer = hipets.maybe_replace_sac_buffer(sac_buffer, obs_shape, act_shape, capacity, seed)   # a hipets.DeviceReplayBuffer

``mbpo.train`` changes one name per piece.  A ``DeterministicPolicy`` runs the reference's code instead, with a warning.  (The actor and the
updater are ``hipets.sac``'s.)
"""
from __future__ import annotations

import warnings
import weakref

import numpy as np
import torch

from .model import UnsupportedModelError
from .replay import DeviceReplayBuffer
from .sac import LOG_KEYS, ReferenceSACUpdater, SACActor, SACUpdater, find_policy, make_sac_updater  # noqa: F401  (their home before hipets.sac)
from ._pack import pack_sac_batch, row_width, staging_views  # noqa: F401

_ENVS = weakref.WeakKeyDictionary()    # a live mbrl ModelEnv -> its hipets.ModelEnv
_ACTORS = weakref.WeakKeyDictionary()  # an agent -> its SACActor


def _hip_env(model_env):
    from .objectives import ModelEnv

    if isinstance(model_env, ModelEnv) or hasattr(model_env, "engine"):  # (or an object that behaves like one: it carries its engine)
        return model_env
    env = _ENVS.get(model_env)
    if env is None:
        env = _ENVS[model_env] = ModelEnv(model_env)
    return env


class PenalisedEnv:
    """A view of a ``hipets.ModelEnv`` whose ``step`` applies an :class:`hipets.UncertaintyPenalty` (one statistics launch of the
    ensemble kernel on the step's (obs, action), one penalty launch on its rewards and dones).  The environment itself is not changed:
    whoever else holds it steps it unpenalised, and its counters and streams advance whichever of the two is stepped."""

    def __init__(self, env, penalty):
        from .ensemble import EnsemblePredictor

        self.env, self.penalty = env, penalty
        self.predictor = EnsemblePredictor(env, engine=env.engine)  # (UnsupportedModelError for a model the kernel does not cover)
        self.engine, self.device = env.engine, env.device

    def reset(self, *args, **kwargs):
        return self.env.reset(*args, **kwargs)

    def step(self, actions, model_state, sample: bool = False):
        return self.env._step(actions, model_state, sample, self.predictor, self.penalty)


def _penalised(env, penalty):
    """the penalised view of ``env`` for ``penalty``, made once per pair and kept with the environment (its step is not touched); an
    environment that carries that very penalty is its own"""
    if getattr(env, "uncertainty", None) == penalty:
        return env
    if not hasattr(env, "_step"):
        raise UnsupportedModelError("the model environment has no step that takes an uncertainty penalty")
    views = env.__dict__.setdefault("_penalised_views", {})  # (a global weak map would keep every environment alive: a view holds its own)
    if penalty not in views:
        views[penalty] = PenalisedEnv(env, penalty)
    return views[penalty]


def _actor(agent, engine) -> SACActor:
    if isinstance(agent, SACActor):
        return agent
    try:
        actor = _ACTORS.get(agent)
    except TypeError:  # (an agent that cannot be weakly referenced gets a fresh actor per call)
        return SACActor(agent, engine=engine)
    if actor is None or actor.engine is not engine or actor.policy is not find_policy(agent):
        actor = _ACTORS[agent] = SACActor(agent, engine=engine)
    return actor


def reference_populate_loop(model_env, replay_buffer, agent, sac_buffer, sac_samples_action: bool, rollout_horizon: int, batch_size: int):
    """mbpo.py:40-63 as the reference runs them: numpy between ``agent.act`` and ``model_env.step``, one ``add_batch`` per step."""
    batch = replay_buffer.sample(batch_size)
    initial_obs, *_ = batch.astuple()
    model_state = model_env.reset(initial_obs_batch=initial_obs, return_as_np=True)
    accum_dones = np.zeros(initial_obs.shape[0], dtype=bool)
    obs = initial_obs
    for _ in range(rollout_horizon):
        action = agent.act(obs, sample=sac_samples_action, batched=True)
        pred_next_obs, pred_rewards, pred_dones, model_state = model_env.step(action, model_state, sample=True)
        truncateds = np.zeros_like(pred_dones, dtype=bool)
        keep = ~accum_dones
        sac_buffer.add_batch(obs[keep], action[keep], pred_next_obs[keep], pred_rewards[keep, 0], pred_dones[keep, 0], truncateds[keep, 0])
        obs = pred_next_obs
        accum_dones |= pred_dones.squeeze()


def add_staged_batches(sac_buffer, staged: np.ndarray, cap: int, counts, obs_dim: int, act_dim: int):
    """One ``sac_buffer.add_batch`` per rollout step over views of the staging area's host copy ``staged`` (``staging_views``), step i
    holding the next ``counts[i]`` rows: the reference's circular-buffer order and wrap-around; reward / terminated (n,), truncated all
    False; the buffer casts to its own dtypes."""
    obs, action, next_obs, reward, done = staging_views(staged, cap, obs_dim, act_dim)
    o = 0
    for n in (int(c) for c in counts):
        r = slice(o, o + n)
        o += n
        sac_buffer.add_batch(obs[r], action[r], next_obs[r], reward[r], done[r] != 0, np.zeros(n, dtype=bool))


def _host_copy(env, buf: torch.Tensor) -> np.ndarray:
    """``buf`` on the host, in ONE copy.  On a GPU the copy lands in a pinned buffer the environment keeps between calls (a pageable
    copy of a fresh array pays a page fault per 4 KiB on top of a slower transfer); the views handed to add_batch are copied out by it
    before the next call overwrites them."""
    if buf.device.type != "cuda":
        return buf.cpu().numpy()
    host = getattr(env, "_mbpo_host", None)
    if host is None or host.numel() < buf.numel():
        host = env._mbpo_host = torch.empty(buf.numel(), dtype=torch.float32, pin_memory=True)
    out = host[:buf.numel()]
    out.copy_(buf, non_blocking=True)
    torch.cuda.current_stream(buf.device).synchronize()
    return out.numpy()


def rollout_model_and_populate_sac_buffer(model_env, replay_buffer, agent, sac_buffer, sac_samples_action: bool, rollout_horizon: int,
                                          batch_size: int, *, uncertainty=None):
    """``mbrl.algorithms.mbpo.rollout_model_and_populate_sac_buffer`` (mbpo.py:31-63), same signature.  ``model_env``: a
    ``hipets.ModelEnv``, or a live ``mbrl.models.ModelEnv`` (wrapped once, cached); ``agent``: what :class:`SACActor` takes, or a
    SACActor.  ``replay_buffer.sample`` stays on the host (the buffer's RNG is consumed as the reference consumes it) and the initial
    observations go up once; every step then is the actor launch, the model step over ALL rows (done or not, as the reference steps
    them) and the compaction of the rows not done before, all on the device; ONE device -> host copy at the end (into a pinned buffer kept
    on the environment) feeds one
    ``add_batch`` per step.  ``model_env``'s reset / step counters advance as under the reference's loop.  An agent the actor kernel
    does not cover runs :func:`reference_populate_loop` over the same environment, with a warning.

    ``sac_buffer`` a :class:`hipets.DeviceReplayBuffer` on the environment's engine: every step's compaction goes straight into the
    buffer's ring (``Engine.ring_compact_transitions``) -- no staging area, no bulk copy, no ``add_batch``; the call ends in one copy
    of the buffer's cursor and the per-step counts (kept in ``sac_buffer.last_populate_counts``) and sets its ``cur_idx`` /
    ``num_stored``.  A batch larger than the buffer's capacity is a ValueError.

    ``uncertainty`` (keyword only; not in the reference): a :class:`hipets.UncertaintyPenalty`.  The rollout steps then run through a
    penalised view of the environment (:class:`PenalisedEnv`, made once per environment and penalty; the environment itself stays as
    it is): after every model step one statistics launch of the ensemble kernel on the step's (obs, action) and one penalty launch on
    its rewards and dones, so both the staging area and the ring store the penalised rewards and dones, and a halted row is stored
    once and dropped from the later steps.  The reference-loop fall-backs step the same penalised view; a model the ensemble kernel
    does not cover runs the reference's loop, with one warning, over the live model's own torch forward
    (:class:`hipets.ensemble.ReferencePenalisedEnv`)."""
    try:
        env = _hip_env(model_env)
        stepper = env if uncertainty is None else _penalised(env, uncertainty)
    except UnsupportedModelError as exc:
        if uncertainty is not None and not hasattr(model_env, "dynamics_model"):
            raise  # (no live model to run the reference's forward on)
        warnings.warn(f"hipets.rollout_model_and_populate_sac_buffer: running the reference's loop ({exc})", stacklevel=2)
        if uncertainty is not None:
            from .ensemble import ReferencePenalisedEnv

            model_env = ReferencePenalisedEnv(model_env, uncertainty)
        return reference_populate_loop(model_env, replay_buffer, agent, sac_buffer, sac_samples_action, rollout_horizon, batch_size)
    try:
        actor = _actor(agent, env.engine)
    except UnsupportedModelError as exc:
        warnings.warn(f"hipets.rollout_model_and_populate_sac_buffer: running the reference's loop over the model environment ({exc})", stacklevel=2)
        return reference_populate_loop(stepper, replay_buffer, agent, sac_buffer, sac_samples_action, rollout_horizon, batch_size)
    batch = replay_buffer.sample(batch_size)
    initial_obs, *_ = batch.astuple()
    L = int(rollout_horizon)
    state = env.reset(initial_obs_batch=np.asarray(initial_obs), return_as_np=False)
    try:
        if L < 1:
            return
        actor.refresh()  # SAC updates ran since the last call
        N, od = (int(v) for v in state["obs"].shape)
        ad = actor.dims[2]
        if isinstance(sac_buffer, DeviceReplayBuffer) and sac_buffer.engine is env.engine:
            return _populate_ring(stepper, actor, sac_buffer, state, sac_samples_action, L)
        head = (L + 3) // 4 * 4  # the per-step counts (int32) travel in front of the staging area: one buffer, one copy
        buf = torch.empty(head + N * L * row_width(od, ad), dtype=torch.float32, device=env.device)
        counts = buf[:head].view(torch.int32)
        counts.zero_()
        staging, cap = buf[head:], N * L
        offset = torch.zeros(1, dtype=torch.int64, device=env.device)
        _rollout_steps(stepper, actor, state, sac_samples_action, L,
                       lambda i, *rows: env.engine.compact_transitions(*rows, staging, cap, offset, counts[i:i + 1]))
        host = _host_copy(env, buf)
    finally:
        env._return_as_np = True  # (what the reference's reset(return_as_np=True) leaves behind)
    add_staged_batches(sac_buffer, host[head:], cap, host[:head].view(np.int32)[:L], od, ad)


def _rollout_steps(env, actor, state, sac_samples_action: bool, L: int, compact):
    """L rollout steps: the actor launch, the model step over ALL rows, ``compact(i, <a compaction's first six arguments>)``"""
    obs = state["obs"]
    accum = torch.zeros(int(obs.shape[0]), dtype=torch.uint8, device=env.device)
    for i in range(L):
        action = actor.act_device(obs, sample=sac_samples_action)
        nobs, rew, done, state = env.step(action, state, sample=True)
        compact(i, obs, action, nobs, rew.reshape(-1), done.reshape(-1), accum)
        obs = nobs


def _populate_ring(env, actor, sac_buffer, state, sac_samples_action: bool, L: int):
    """The rollout steps of :func:`rollout_model_and_populate_sac_buffer` into a DeviceReplayBuffer's ring"""
    N, od = (int(v) for v in state["obs"].shape)
    if (od, actor.dims[2]) != (sac_buffer.obs_dim, sac_buffer.act_dim):
        raise ValueError(f"the SAC buffer stores obs {sac_buffer.obs_dim} / act {sac_buffer.act_dim}, the rollout makes {od} / {actor.dims[2]}")
    if N > sac_buffer.capacity:
        raise ValueError(f"a rollout batch of {N} rows does not fit a SAC buffer of {sac_buffer.capacity}")
    counts = torch.zeros(L, dtype=torch.int32, device=env.device)
    _rollout_steps(env, actor, state, sac_samples_action, L,
                   lambda i, *rows: env.engine.ring_compact_transitions(*rows, sac_buffer.storage, sac_buffer.capacity, sac_buffer.cursor,
                                                                        counts[i:i + 1]))
    tail = torch.cat([sac_buffer.cursor, counts.to(torch.int64)]).cpu().tolist()  # the call's ONE device -> host copy
    sac_buffer.cur_idx, sac_buffer.num_stored = tail[0], tail[1]
    sac_buffer.last_populate_counts = tail[2:]
