"""MBPO's model rollouts on the device (mbrl/algorithms/mbpo.py:31-63): the SAC actor as one HIP launch, the model step as the
existing ``hipets_step`` launch, and a compaction of the step's live rows into a device staging area -- three plainly ordered pieces per
rollout step, one device -> host copy per call.

    agent = hipets.SACActor(sac_agent)                    # drop-in for SACAgent.act, numpy in / numpy out
    hipets.rollout_model_and_populate_sac_buffer(model_env, replay_buffer, sac_agent, sac_buffer, True, rollout_length, batch_size)

``mbpo.train`` changes one name.  Out of scope: SAC's updates, ``DeterministicPolicy`` (the reference's loop runs instead, with a warning).
"""
from __future__ import annotations

import warnings
import weakref
from typing import Optional

import numpy as np
import torch

from ._pack import pack_policy
from .model import UnsupportedModelError


def find_policy(agent):
    """The policy module of an ``mbrl.planning.SACAgent`` (``.sac_agent.policy``), a ``pytorch_sac_pranz24.SAC`` (``.policy``) or a
    bare policy module."""
    inner = getattr(agent, "sac_agent", agent)
    return getattr(inner, "policy", inner)


class SACActor:
    """``GaussianPolicy.forward / sample`` (pytorch_sac_pranz24/model.py:88-108) as ``SAC.select_action`` uses them, on the actor kernel
    (hipets_policy_act).  ``agent``: an ``mbrl.planning.SACAgent``, a ``pytorch_sac_pranz24.SAC`` or a bare ``GaussianPolicy``; anything
    else -- a ``DeterministicPolicy`` -- raises UnsupportedModelError.  The engine holds a SNAPSHOT of the weights: ``refresh()`` after
    SAC updates (``rollout_model_and_populate_sac_buffer`` does it at every call).

    Sampling draws eps in-kernel from (``seed``, the number of sampling calls so far): two actors with one seed and one call history
    draw the same actions; ``last_draw`` = the (seed, stream_id) of the latest one, for ``Engine.policy_normals``."""

    def __init__(self, agent, engine=None, seed: int = 0):
        self.policy = find_policy(agent)
        self.dims, _ = pack_policy(self.policy)  # (UnsupportedModelError for anything that is not a GaussianPolicy of the kernel's sizes)
        if engine is None:
            from .engine import get_engine

            p = self.policy.linear1.weight
            engine = get_engine(p.device if p.device.type == "cuda" else "cuda")
        self.engine, self.device, self.seed = engine, engine.device, int(seed)
        self.draws = 0
        self.last_draw = None
        self.refresh()

    def refresh(self):
        """Re-snapshot the policy's live weights (device to device where the policy is on the engine's GPU)."""
        self.dims = self.engine.policy_set(self.policy)
        self.engine.policy_owner = weakref.ref(self)

    def _own_engine(self):
        owner = getattr(self.engine, "policy_owner", None)
        if owner is None or owner() is not self:  # (another actor's policy sits in the engine)
            self.refresh()

    def act_device(self, obs_t: torch.Tensor, sample: bool = False, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``obs_t`` f32 [B, obs_dim] on the device -> actions f32 [B, act_dim] on the device.  ``eps`` [B, act_dim]: the sample's
        normals (torch's own, for the exact path) instead of the in-kernel draw."""
        if not isinstance(obs_t, torch.Tensor) or obs_t.ndim != 2 or int(obs_t.shape[1]) != self.dims[0]:
            raise ValueError(f"obs must be [B, {self.dims[0]}], got {tuple(getattr(obs_t, 'shape', ()))}")
        self._own_engine()
        stream = 0
        if sample and eps is None:
            self.draws += 1
            stream = self.draws
            self.last_draw = (self.seed, stream)
        return self.engine.policy_act(obs_t, sample=sample, seed=self.seed, stream_id=stream, eps=eps)

    def act(self, obs: np.ndarray, sample: bool = False, batched: bool = False, **_kwargs) -> np.ndarray:
        """``SACAgent.act`` (mbrl/planning/sac_wrapper.py:27-46): the mean action, or a sampled one; ``batched``: obs is [B, obs_dim]."""
        t = torch.as_tensor(np.asarray(obs, dtype=np.float32))
        if not batched:
            t = t.unsqueeze(0)
        out = self.act_device(t.to(self.device).contiguous(), sample=sample).cpu().numpy()
        return out if batched else out[0]


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


def staging_views(flat, cap: int, obs_dim: int, act_dim: int):
    """The five arrays of hipets_compact_transitions' staging area in ``flat`` (a tensor or a numpy array of at least cap * (2 obs_dim +
    act_dim + 2) float32): (obs [cap, obs_dim], action [cap, act_dim], next_obs [cap, obs_dim], reward [cap], done [cap] as 0.0 / 1.0)"""
    o1 = cap * obs_dim
    o2 = o1 + cap * act_dim
    o3 = o2 + cap * obs_dim
    return (flat[:o1].reshape(cap, obs_dim), flat[o1:o2].reshape(cap, act_dim), flat[o2:o3].reshape(cap, obs_dim), flat[o3:o3 + cap],
            flat[o3 + cap:o3 + 2 * cap])


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
                                          batch_size: int):
    """``mbrl.algorithms.mbpo.rollout_model_and_populate_sac_buffer`` (mbpo.py:31-63), same signature.  ``model_env``: a
    ``hipets.ModelEnv``, or a live ``mbrl.models.ModelEnv`` (wrapped once, cached); ``agent``: what :class:`SACActor` takes, or a
    SACActor.  ``replay_buffer.sample`` stays on the host (the buffer's RNG is consumed as the reference consumes it) and the initial
    observations go up once; every step then is the actor launch, the model step over ALL rows (done or not, as the reference steps
    them) and the compaction of the rows not done before, all on the device; ONE device -> host copy at the end (into a pinned buffer kept
    on the environment) feeds one
    ``add_batch`` per step.  ``model_env``'s reset / step counters advance as under the reference's loop.  An agent the actor kernel
    does not cover runs :func:`reference_populate_loop` over the same environment, with a warning."""
    try:
        env = _hip_env(model_env)
    except UnsupportedModelError as exc:
        warnings.warn(f"hipets.rollout_model_and_populate_sac_buffer: running the reference's loop ({exc})", stacklevel=2)
        return reference_populate_loop(model_env, replay_buffer, agent, sac_buffer, sac_samples_action, rollout_horizon, batch_size)
    try:
        actor = _actor(agent, env.engine)
    except UnsupportedModelError as exc:
        warnings.warn(f"hipets.rollout_model_and_populate_sac_buffer: running the reference's loop over the model environment ({exc})", stacklevel=2)
        return reference_populate_loop(env, replay_buffer, agent, sac_buffer, sac_samples_action, rollout_horizon, batch_size)
    batch = replay_buffer.sample(batch_size)
    initial_obs, *_ = batch.astuple()
    L = int(rollout_horizon)
    state = env.reset(initial_obs_batch=np.asarray(initial_obs), return_as_np=False)
    try:
        if L < 1:
            return
        actor.refresh()  # SAC updates ran since the last call
        eng, dev = env.engine, env.device
        obs = state["obs"]
        N, od = (int(v) for v in obs.shape)
        ad = actor.dims[2]
        width = 2 * od + ad + 2
        head = (L + 3) // 4 * 4  # the per-step counts (int32) travel in front of the staging area: one buffer, one copy
        buf = torch.empty(head + N * L * width, dtype=torch.float32, device=dev)
        counts = buf[:head].view(torch.int32)
        counts.zero_()
        staging, cap = buf[head:], N * L
        offset = torch.zeros(1, dtype=torch.int64, device=dev)
        accum = torch.zeros(N, dtype=torch.uint8, device=dev)
        for i in range(L):
            action = actor.act_device(obs, sample=sac_samples_action)
            nobs, rew, done, state = env.step(action, state, sample=True)
            eng.compact_transitions(obs, action, nobs, rew.reshape(-1), done.reshape(-1), accum, staging, cap, offset, counts[i:i + 1])
            obs = nobs
        host = _host_copy(env, buf)
    finally:
        env._return_as_np = True  # (what the reference's reset(return_as_np=True) leaves behind)
    add_staged_batches(sac_buffer, host[head:], cap, host[:head].view(np.int32)[:L], od, ad)
