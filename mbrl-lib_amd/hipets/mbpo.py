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

``mbpo.train`` changes one name per piece.  A ``DeterministicPolicy`` runs the reference's code instead, with a warning.
"""
from __future__ import annotations

import warnings
import weakref
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._pack import pack_policy
from .model import UnsupportedModelError
from .replay import DeviceReplayBuffer


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
    does not cover runs :func:`reference_populate_loop` over the same environment, with a warning.

    ``sac_buffer`` a :class:`hipets.DeviceReplayBuffer` on the environment's engine: every step's compaction goes straight into the
    buffer's ring (``Engine.ring_compact_transitions``) -- no staging area, no bulk copy, no ``add_batch``; the call ends in one copy
    of the buffer's cursor and the per-step counts (kept in ``sac_buffer.last_populate_counts``) and sets its ``cur_idx`` /
    ``num_stored``.  A batch larger than the buffer's capacity is a ValueError."""
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
        if isinstance(sac_buffer, DeviceReplayBuffer) and sac_buffer.engine is eng:
            return _populate_ring(env, actor, sac_buffer, state, sac_samples_action, L)
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


def _populate_ring(env, actor, sac_buffer, state, sac_samples_action: bool, L: int):
    """The rollout steps of :func:`rollout_model_and_populate_sac_buffer` into a DeviceReplayBuffer's ring"""
    eng, dev = env.engine, env.device
    obs = state["obs"]
    N, od = (int(v) for v in obs.shape)
    if (od, actor.dims[2]) != (sac_buffer.obs_dim, sac_buffer.act_dim):
        raise ValueError(f"the SAC buffer stores obs {sac_buffer.obs_dim} / act {sac_buffer.act_dim}, the rollout makes {od} / {actor.dims[2]}")
    if N > sac_buffer.capacity:
        raise ValueError(f"a rollout batch of {N} rows does not fit a SAC buffer of {sac_buffer.capacity}")
    counts = torch.zeros(L, dtype=torch.int32, device=dev)
    accum = torch.zeros(N, dtype=torch.uint8, device=dev)
    for i in range(L):
        action = actor.act_device(obs, sample=sac_samples_action)
        nobs, rew, done, state = env.step(action, state, sample=True)
        eng.ring_compact_transitions(obs, action, nobs, rew.reshape(-1), done.reshape(-1), accum, sac_buffer.storage, sac_buffer.capacity,
                                     sac_buffer.cursor, counts[i:i + 1])
        obs = nobs
    tail = torch.cat([sac_buffer.cursor, counts.to(torch.int64)]).cpu().tolist()  # the call's ONE device -> host copy
    sac_buffer.cur_idx, sac_buffer.num_stored = tail[0], tail[1]
    sac_buffer.last_populate_counts = tail[2:]


# ---- SAC's updates (third_party/pytorch_sac_pranz24/sac.py:76-173) ----------------------------------------------------------------
_POLICY_LAYERS = ("linear1", "linear2", "mean_linear", "log_std_linear")
_CRITIC_LAYERS = ("linear1", "linear2", "linear3", "linear4", "linear5", "linear6")
_SAC_ATTRS = ("policy", "critic", "critic_target", "critic_optim", "policy_optim", "gamma", "tau", "alpha", "target_update_interval",
              "automatic_entropy_tuning")
LOG_KEYS = ("train/batch_reward", "train_critic/loss", "train_actor/loss", "train_actor/target_entropy", "train_actor/entropy",
            "train_alpha/loss", "train_alpha/value")


def pack_sac_batch(transitions, reverse_mask: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
    """``memory.sample(batch_size).astuple()`` -> f32 [B, 2 obs + act + 2], a row = (state, action, next_state, reward, mask): what
    sac.py:80-95 uploads as five tensors.  mask = the terminated flag as a float, or ``1 - terminated`` under ``reverse_mask``
    (``mask_batch.logical_not()``).  The truncated flags are ignored, as there.  ``out``: a [B, width] array to fill."""
    state, action, next_state, reward, terminated = (np.asarray(v) for v in transitions[:5])
    B, obs = state.shape
    act = action.shape[1]
    if out is None:
        out = np.empty((B, 2 * obs + act + 2), dtype=np.float32)
    out[:, :obs] = state
    out[:, obs:obs + act] = action
    out[:, obs + act:2 * obs + act] = next_state
    out[:, 2 * obs + act] = np.reshape(reward, B)
    mask = np.reshape(terminated, B).astype(np.float32)
    out[:, 2 * obs + act + 1] = (mask == 0).astype(np.float32) if reverse_mask else mask
    return out


def _plain_adam(opt, name: str):
    """(lr, beta1, beta2, eps) of a torch.optim.Adam with the settings the update kernels implement, or UnsupportedModelError"""
    if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
        raise UnsupportedModelError(f"{name} is not a torch.optim.Adam with one parameter group")
    g = opt.param_groups[0]
    for key in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
        if g.get(key):
            raise UnsupportedModelError(f"{name}: Adam with {key}=True is not covered by the update kernels")
    if float(g.get("weight_decay", 0.0)) != 0.0:
        raise UnsupportedModelError(f"{name}: Adam with weight_decay != 0 is not covered by the update kernels")
    b1, b2 = (float(b) for b in g["betas"])
    return float(g["lr"]), b1, b2, float(g["eps"])


def _adam_state(opt, params):
    """The optimizer's (exp_avg list, exp_avg_sq list, step tensors) of ``params``; missing entries are created the way
    torch.optim.Adam._init_group creates them (step a float scalar on the host, moments zeros_like the parameter)."""
    try:
        from torch.optim.optimizer import _get_scalar_dtype
        step_dtype = _get_scalar_dtype()
    except ImportError:
        step_dtype = torch.float32
    ms, vs, steps = [], [], []
    for p in params:
        st = opt.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=step_dtype)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if not torch.is_tensor(st.get("step")):  # (a state_dict of an old torch: a Python number)
            st["step"] = torch.tensor(float(st["step"]), dtype=step_dtype)
        ms.append(st["exp_avg"])
        vs.append(st["exp_avg_sq"])
        steps.append(st["step"])
    return ms, vs, steps


class SACUpdater:
    """``SAC.update_parameters`` (pytorch_sac_pranz24/sac.py:76-173) on the update kernels (hipets_sac_update): same signature, same
    5-tuple.  ``agent``: an ``mbrl.planning.SACAgent``, a ``pytorch_sac_pranz24.SAC`` or an object shaped like one (policy, critic,
    critic_target, critic_optim, policy_optim, gamma, tau, alpha, target_update_interval, automatic_entropy_tuning; with tuning on
    also log_alpha, alpha_optim, target_entropy).

    The kernels work IN PLACE on the modules' parameters, ``log_alpha`` and the optimizers' ``exp_avg`` / ``exp_avg_sq``: no packed
    copy, nothing to write back -- ``SACAgent.act``, ``SACActor.refresh()``, ``save_checkpoint`` and a later stock
    ``update_parameters`` see current values.  ``state[p]["step"]`` counts the updates; ``agent.alpha`` holds exp(log_alpha) after a
    tuned update.  ``memory.sample`` stays on the host (the buffer's RNG is consumed as the reference consumes it); the two normal
    tables of an update are drawn by torch on the device as ``Normal.rsample`` draws them, next-state table first.

    Raises UnsupportedModelError for what the kernels do not cover (a DeterministicPolicy, modules off the engine's device, Adam
    settings other than the plain ones, sizes past the HIPETS_POLICY_MAX_* limits, a batch outside 1 .. 1024)."""

    def __init__(self, agent, engine=None, batch_size: Optional[int] = None):
        sac = getattr(agent, "sac_agent", agent)
        missing = [n for n in _SAC_ATTRS if not hasattr(sac, n)]
        if missing:
            raise UnsupportedModelError(f"{type(sac).__name__} is not shaped like a SAC agent (no {', '.join(missing)})")
        self.sac = sac
        self.tuning = bool(sac.automatic_entropy_tuning)
        if self.tuning and any(not hasattr(sac, n) for n in ("log_alpha", "alpha_optim", "target_entropy")):
            raise UnsupportedModelError("automatic_entropy_tuning without log_alpha / alpha_optim / target_entropy")
        (obs, hid, act), pol = pack_policy(sac.policy)  # (a DeterministicPolicy has no heads: UnsupportedModelError)
        self.dims = (obs, act, hid)
        self.check_batch(batch_size)
        for net, name in ((sac.critic, "critic"), (sac.critic_target, "critic_target")):
            layers = [getattr(net, n, None) for n in _CRITIC_LAYERS]
            if any(l is None or getattr(l, "weight", None) is None or getattr(l, "bias", None) is None for l in layers):
                raise UnsupportedModelError(f"{name} is not shaped like a QNetwork (linear1 .. linear6 with biases)")
            want = [(hid, obs + act), (hid, hid), (1, hid)] * 2
            if [tuple(l.weight.shape) for l in layers] != want:
                raise UnsupportedModelError(f"{name} layer shapes do not chain: expected [hid, obs + act], [hid, hid], [1, hid] twice")
        self._adam = [_plain_adam(sac.critic_optim, "critic_optim"), _plain_adam(sac.policy_optim, "policy_optim"),
                      _plain_adam(sac.alpha_optim, "alpha_optim") if self.tuning else (0.0, 0.9, 0.999, 1e-8)]
        pol_p = [t for l in _POLICY_LAYERS for t in (getattr(sac.policy, l).weight, getattr(sac.policy, l).bias)]
        crit_p = [t for l in _CRITIC_LAYERS for t in (getattr(sac.critic, l).weight, getattr(sac.critic, l).bias)]
        tgt_p = [t for l in _CRITIC_LAYERS for t in (getattr(sac.critic_target, l).weight, getattr(sac.critic_target, l).bias)]
        for opt, params, name in ((sac.policy_optim, pol_p, "policy_optim"), (sac.critic_optim, crit_p, "critic_optim")):
            owned = opt.param_groups[0]["params"]
            if len(owned) != len(params) or any(a is not b for a, b in zip(sorted(owned, key=id), sorted(params, key=id))):
                raise UnsupportedModelError(f"{name} does not optimize exactly its network's layers")
        every = pol_p + crit_p + tgt_p + ([sac.log_alpha] if self.tuning else [])
        dev = pol_p[0].device
        if engine is None:
            if dev.type != "cuda":
                raise UnsupportedModelError(f"the agent's modules are on {dev}: the update kernels need them on the GPU")
            from .engine import get_engine

            engine = get_engine(dev)
        if any(t.device != engine.device for t in every):
            raise UnsupportedModelError(f"the agent's modules are not all on the engine's device {engine.device}")
        if any(t.dtype != torch.float32 or not t.is_contiguous() for t in every):
            raise UnsupportedModelError("the agent's parameters must be contiguous float32 tensors")
        if self.tuning and (sac.log_alpha.numel() != 1 or sac.alpha_optim.param_groups[0]["params"][0] is not sac.log_alpha):
            raise UnsupportedModelError("alpha_optim does not optimize a one-element log_alpha")
        self.engine, self.device = engine, engine.device
        self._params = (pol_p, crit_p, tgt_p)
        self._scale = pol["action_scale"].to(self.device, torch.float32).contiguous()
        self._bias = pol["action_bias"].to(self.device, torch.float32).contiguous()
        self._alpha = torch.zeros(1, dtype=torch.float32, device=self.device)  # the coefficient the kernels read (and, tuned, write)
        self._alpha_seen = None
        self._bound = None
        self._host = None
        self._host_idx = None

    @staticmethod
    def check_batch(batch_size):
        if batch_size is not None and not 1 <= int(batch_size) <= _lib.SAC_MAX_BATCH:
            raise UnsupportedModelError(f"a SAC batch of {batch_size} is outside the update kernels' 1 .. {_lib.SAC_MAX_BATCH}")

    # ---- binding: the live tensors' addresses, re-read at every call (an optimizer.load_state_dict replaces the moment tensors) ----
    def _tensors(self):
        sac = self.sac
        pol_p, crit_p, tgt_p = self._params
        pm, pv, psteps = _adam_state(sac.policy_optim, pol_p)
        cm, cv, csteps = _adam_state(sac.critic_optim, crit_p)
        if self.tuning:
            am, av, asteps = _adam_state(sac.alpha_optim, [sac.log_alpha])
            alpha_t = [sac.log_alpha, am[0], av[0]]
        else:
            alpha_t, asteps = [None, None, None], []
        table = pol_p + pm + pv + crit_p + cm + cv + tgt_p + alpha_t + [self._alpha, self._scale, self._bias]
        return table, (csteps, psteps, asteps)

    def _bind(self):
        table, steps = self._tensors()
        for t in table:
            if t is not None and (t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous()):
                raise UnsupportedModelError("an optimizer's state is not contiguous float32 on the engine's device")
        ptrs = tuple(0 if t is None else t.data_ptr() for t in table)
        sac = self.sac
        hyper = (float(sac.gamma), float(sac.tau), float(sac.target_entropy) if self.tuning else 0.0, int(sac.target_update_interval),
                 tuple(a[1:] for a in self._current_adam()))
        owner = getattr(self.engine, "sac_owner", None)
        if self._bound != (ptrs, hyper) or owner is None or owner() is not self:
            self.engine.sac_bind(self.dims, self.tuning, hyper[0], hyper[1], hyper[2], hyper[3], [v for a in hyper[4] for v in a], ptrs)
            self.engine.sac_owner = weakref.ref(self)
            self._bound = (ptrs, hyper)
        return steps

    def _current_adam(self):
        sac = self.sac
        return [_plain_adam(sac.critic_optim, "critic_optim"), _plain_adam(sac.policy_optim, "policy_optim"),
                _plain_adam(sac.alpha_optim, "alpha_optim") if self.tuning else (0.0, 0.9, 0.999, 1e-8)]

    def _sync_alpha(self):
        alpha = self.sac.alpha
        if alpha is self._alpha or alpha is self._alpha_seen:
            return
        with torch.no_grad():
            if torch.is_tensor(alpha):
                self._alpha.copy_(alpha.detach().reshape(-1)[:1])
            else:
                self._alpha.fill_(float(alpha))
        self._alpha_seen = alpha

    def _staging(self, n: int, B: int):
        width = 2 * self.dims[0] + self.dims[1] + 2
        need = n * B * width
        if self._host is None or self._host[0].numel() < need or self._host[1].shape[0] < n:
            self._host = (torch.empty(need, dtype=torch.float32, pin_memory=True), torch.empty(max(n, 1), 8, dtype=torch.float32, pin_memory=True))
        return self._host[0][:need].view(n, B, width), self._host[1][:n]

    def _index_staging(self, need: int):
        if self._host_idx is None or self._host_idx.numel() < need:
            self._host_idx = torch.empty(need, dtype=torch.int64, pin_memory=True)
        return self._host_idx[:need]

    def update_many(self, memories, batch_size: int, first_update: int, logger=None, reverse_mask: bool = False, *, eps=None):
        """``len(memories)`` consecutive updates, update i sampling ``memories[i]`` (mbpo.py:259-260 picks a buffer per update) with
        index ``first_update + i``: all batches are sampled in order and go up in ONE pinned copy, the 2 n normal tables are drawn in
        order, the n updates are queued behind each other, ONE synchronisation, one small device -> host copy.  Returns the n
        5-tuples -- bit for bit those of n single :meth:`update_parameters` calls.  A memory that is a
        :class:`hipets.DeviceReplayBuffer` on this engine only draws its indices on the host (``sample_indices``: its generator is
        consumed as ``sample`` consumes it, in the memories' order); all indices go up in one copy and ONE gather launch per distinct
        buffer builds its batches on the device -- the floats ``sample`` + ``pack_sac_batch`` would have uploaded.  ``eps``: n pairs
        (next-state table, state table) of device tensors [B, act] to use instead of drawing them (a replay of recorded draws).  A
        batch outside 1 .. 1024 raises UnsupportedModelError."""
        self.check_batch(batch_size)
        n, B = len(memories), int(batch_size)
        if n == 0:
            return []
        obs, act, _ = self.dims
        host, host_res = self._staging(n, B)
        where = [None] * n  # update i reads (None, its slot of the pinned slab) or (a device buffer's group, its slot there)
        groups = {}         # id(device buffer) -> [the buffer, its updates' index draws]
        n_host = 0
        for i, memory in enumerate(memories):
            if isinstance(memory, DeviceReplayBuffer) and memory.engine is self.engine:
                if (memory.obs_dim, memory.act_dim) != (obs, act):
                    raise ValueError(f"the buffer stores obs {memory.obs_dim} / act {memory.act_dim}, expected {obs} / {act}")
                group = groups.setdefault(id(memory), [memory, []])
                where[i] = (group, len(group[1]))
                group[1].append(memory.sample_indices(B))
                continue
            tr = memory.sample(B).astuple()
            if np.shape(tr[0]) != (B, obs) or np.shape(tr[1]) != (B, act):
                raise ValueError(f"the buffer's sample is {np.shape(tr[0])} / {np.shape(tr[1])}, expected ({B}, {obs}) / ({B}, {act})")
            pack_sac_batch(tr, reverse_mask, out=host[n_host].numpy())
            where[i] = (None, n_host)
            n_host += 1
        steps = self._bind()
        self._sync_alpha()
        dev = self.device
        with torch.cuda.device(dev), torch.no_grad():
            batch = host[:n_host].to(dev, non_blocking=True) if n_host else None
            if groups:
                idx = self._index_staging((n - n_host) * B)
                o = 0
                for group in groups.values():
                    for draw in group[1]:
                        idx[o:o + B] = torch.from_numpy(np.asarray(draw, dtype=np.int64))
                        o += B
                idx_dev = idx.to(dev, non_blocking=True)  # ONE upload of every buffer's draws
                o = 0
                for group in groups.values():
                    m = len(group[1])
                    group.append(group[0].gather(idx_dev[o:o + m * B], reverse_mask).view(m, B, -1))
                    o += m * B
            results = torch.empty(n, 8, dtype=torch.float32, device=dev)
            adam = self._current_adam()
            lrs = [a[0] for a in adam]
            step0 = [int(s[0].item()) if s else 0 for s in steps]
            for i in range(n):
                if eps is not None:
                    eps_next, eps_cur = eps[i]
                else:
                    eps_next = torch.empty(B, act, dtype=torch.float32, device=dev).normal_()  # Normal.rsample's draw, next state first
                    eps_cur = torch.empty(B, act, dtype=torch.float32, device=dev).normal_()
                group, slot = where[i]
                self.engine.sac_update(batch[slot] if group is None else group[2][slot], eps_next, eps_cur, int(first_update) + i,
                                       [s + i for s in step0], lrs, results[i])
            host_res.copy_(results, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
        for group in steps:
            for s in group:
                s += n
        if self.tuning:
            self.sac.alpha = self._alpha
        res = host_res.numpy()
        out = []
        for i in range(n):
            q1, q2, pl, al, alpha, reward, entropy = (float(v) for v in res[i, :7])
            if logger is not None:
                u = int(first_update) + i
                logger.log("train/batch_reward", reward, u)
                logger.log("train_critic/loss", float(np.float32(res[i, 0]) + np.float32(res[i, 1])), u)
                logger.log("train_actor/loss", pl, u)
                logger.log("train_actor/target_entropy", self.sac.target_entropy if self.tuning else 0, u)
                logger.log("train_actor/entropy", entropy, u)
                logger.log("train_alpha/loss", al, u)
                logger.log("train_alpha/value", alpha, u)
            out.append((q1, q2, pl, al, alpha))
        return out

    def update_parameters(self, memory, batch_size, updates, logger=None, reverse_mask=False):
        """``SAC.update_parameters`` (sac.py:76-173): (qf1_loss, qf2_loss, policy_loss, alpha_loss, alpha) as floats"""
        return self.update_many([memory], batch_size, updates, logger, reverse_mask)[0]

    def forward_taps(self, batch_size: int):
        """Intermediates of the last update: ``Engine.sac_forward_taps``"""
        return self.engine.sac_forward_taps(batch_size)


class ReferenceSACUpdater:
    """What :func:`make_sac_updater` returns for an agent the update kernels do not cover: ``update_parameters`` IS the agent's own."""

    def __init__(self, agent):
        self.sac = getattr(agent, "sac_agent", agent)
        self.update_parameters = self.sac.update_parameters

    def update_many(self, memories, batch_size, first_update, logger=None, reverse_mask=False):
        return [self.update_parameters(m, batch_size, int(first_update) + i, logger, reverse_mask) for i, m in enumerate(memories)]


def make_sac_updater(agent, engine=None, batch_size: Optional[int] = None):
    """A :class:`SACUpdater` for ``agent`` where the update kernels cover it; otherwise -- with ONE warning that names the reason --
    an object whose ``update_parameters`` is the agent's own (and whose ``update_many`` loops over it)."""
    try:
        return SACUpdater(agent, engine=engine, batch_size=batch_size)
    except UnsupportedModelError as exc:
        warnings.warn(f"hipets.make_sac_updater: running the agent's own update_parameters ({exc})", stacklevel=2)
        return ReferenceSACUpdater(agent)
