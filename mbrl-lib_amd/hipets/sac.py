"""The SAC agent's modules on the engine (third_party/pytorch_sac_pranz24): the actor (``SACActor``, hipets_policy_act), the critic
(``SACCritic``, hipets_critic_q) and the updates (``SACUpdater``, hipets_sac_update; ``make_sac_updater``); each holds one slot of the
engine, the first two by the one rule of :class:`_Snapshot`."""
from __future__ import annotations

import warnings
import weakref
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._pack import CRITIC_LAYERS, POLICY_LAYERS, check_critic_split, pack_critic, pack_policy, pack_sac_batch, row_width
from .model import UnsupportedModelError
from .replay import DeviceReplayBuffer

def find_policy(agent):
    """The policy module of an ``mbrl.planning.SACAgent`` (``.sac_agent.policy``), a ``pytorch_sac_pranz24.SAC`` (``.policy``) or a
    bare policy module."""
    inner = getattr(agent, "sac_agent", agent)
    return getattr(inner, "policy", inner)


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


def _engine_of(tensor):
    from .engine import get_engine

    return get_engine(tensor.device if tensor.device.type == "cuda" else "cuda")


class _SlotOwner:
    """Holds the engine's ``slot`` ("policy" / "critic" / "sac") by a weak reference in ``Engine.<slot>_owner``.  The engine may be any
    object with the slot's methods: one without the owner attribute yet has an empty slot, one without ``sac_updates`` has run none."""

    def owns(self) -> bool:
        ref = getattr(self.engine, self.slot + "_owner", None)
        return ref is not None and ref() is self

    def claim(self):
        setattr(self.engine, self.slot + "_owner", weakref.ref(self))


class _Snapshot(_SlotOwner):
    """When was a module's snapshot in an engine taken?  ``moved()``: a watched parameter's ``_version`` changed (a stock optimizer
    step, a ``load_state_dict``), or the engine ran ``sac_update`` since (its kernels write parameters through raw pointers: no version
    moves).  ``watch``: further modules whose parameters are watched too -- for a ``critic_target`` the live ``critic``: the stock
    agent writes its target as ``target_param.data.copy_(...)`` (pytorch_sac_pranz24/utils.py:28, 33), which moves no version of the
    target's, but every such write follows a ``critic_optim.step()``, which moves the critic's.  ``_set()`` snapshots the module into
    the subclass's slot (``Engine.<slot>_set``), claims it and marks the moment."""

    def __init__(self, module, engine, watch=()):
        self.modules, self.engine = (module,) + tuple(m for m in watch if m is not None and m is not module), engine
        self.mark()

    def _state(self):
        return tuple(int(p._version) for m in self.modules for p in m.parameters()), getattr(self.engine, "sac_updates", 0)

    def mark(self):
        self.state = self._state()

    def moved(self) -> bool:
        return self.state != self._state()

    def stale(self) -> bool:
        """Does the engine's snapshot differ from the live module as far as can be told without reading it: a parameter's version
        moved, the engine ran a SAC update since, or another owner sits in the engine's slot?"""
        return not self.owns() or self.moved()

    def _set(self, *args):
        dims = getattr(self.engine, self.slot + "_set")(self.modules[0], *args)
        self.claim()
        self.mark()
        return dims


class SACActor(_Snapshot):
    """``GaussianPolicy.forward / sample`` (pytorch_sac_pranz24/model.py:88-108) as ``SAC.select_action`` uses them, on the actor kernel
    (hipets_policy_act).  ``agent``: an ``mbrl.planning.SACAgent``, a ``pytorch_sac_pranz24.SAC`` or a bare ``GaussianPolicy``; anything
    else -- a ``DeterministicPolicy`` -- raises UnsupportedModelError.  The engine holds a SNAPSHOT of the weights: ``refresh()`` after
    SAC updates (``rollout_model_and_populate_sac_buffer`` does it at every call).

    Sampling draws eps in-kernel from (``seed``, the number of sampling calls so far): two actors with one seed and one call history
    draw the same actions; ``last_draw`` = the (seed, stream_id) of the latest one, for ``Engine.policy_normals``."""
    slot = "policy"

    def __init__(self, agent, engine=None, seed: int = 0):
        self.policy = find_policy(agent)
        self.dims, _ = pack_policy(self.policy)  # (UnsupportedModelError for anything that is not a GaussianPolicy of the kernel's sizes)
        super().__init__(self.policy, engine if engine is not None else _engine_of(self.policy.linear1.weight))
        self.device, self.seed = self.engine.device, int(seed)
        self.draws = 0
        self.last_draw = None
        self.refresh()

    def refresh(self):
        """Re-snapshot the policy's live weights (device to device where the policy is on the engine's GPU)."""
        self.dims = self._set()

    def act_device(self, obs_t: torch.Tensor, sample: bool = False, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``obs_t`` f32 [B, obs_dim] on the device -> actions f32 [B, act_dim] on the device.  ``eps`` [B, act_dim]: the sample's
        normals (torch's own, for the exact path) instead of the in-kernel draw."""
        if not isinstance(obs_t, torch.Tensor) or obs_t.ndim != 2 or int(obs_t.shape[1]) != self.dims[0]:
            raise ValueError(f"obs must be [B, {self.dims[0]}], got {tuple(getattr(obs_t, 'shape', ()))}")
        if not self.owns():  # (another actor's policy sits in the engine)
            self.refresh()
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


class SACCritic(_Snapshot):
    """``QNetwork.forward`` (pytorch_sac_pranz24/model.py:36-61) on the critic kernel (hipets_critic_q).  ``agent``: an
    ``mbrl.planning.SACAgent``, a ``pytorch_sac_pranz24.SAC`` or a bare ``QNetwork``-shaped module (linear1..3 = Q1, linear4..6 = Q2);
    ``target``: the agent's ``critic_target``.  Anything else raises UnsupportedModelError with the reason.  The engine holds a SNAPSHOT
    of the weights: ``refresh()`` after the critic changed (``stale()`` tells; for a target it also watches the agent's live
    ``critic``, whose optimizer step precedes every stock soft update).  ``obs_dim``: where the critic's input splits into state and
    action; by default read off the agent's policy, else fixed by the first ``q`` call."""
    slot = "critic"

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
        live = getattr(getattr(agent, "sac_agent", agent), "critic", None) if target else None
        super().__init__(self.critic, engine if engine is not None else _engine_of(tensors[0]), watch=(live,) if isinstance(live, torch.nn.Module) else ())
        self.device = self.engine.device
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
        self._set(*self.split)

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
        if not self.owns():  # (another critic's weights sit in the engine)
            self.refresh()
        return self.engine.critic_q(obs_t, act_t, q1=q1, q2=q2, qmin=qmin)


# ---- SAC's updates (third_party/pytorch_sac_pranz24/sac.py:76-173) ----------------------------------------------------------------
_SAC_ATTRS = ("policy", "critic", "critic_target", "critic_optim", "policy_optim", "gamma", "tau", "alpha", "target_update_interval",
              "automatic_entropy_tuning")
LOG_KEYS = ("train/batch_reward", "train_critic/loss", "train_actor/loss", "train_actor/target_entropy", "train_actor/entropy",
            "train_alpha/loss", "train_alpha/value")


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


class SACUpdater(_SlotOwner):
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
    slot = "sac"

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
            try:
                sizes, _ = pack_critic(net, obs)
            except UnsupportedModelError as exc:
                raise UnsupportedModelError(f"{name}: {exc}") from None
            if sizes != (obs + act, hid):
                raise UnsupportedModelError(f"{name} layer shapes do not chain: expected [hid, obs + act], [hid, hid], [1, hid] twice")
        self._current_adam()  # (UnsupportedModelError for optimizers the kernels do not implement)
        pol_p = [t for l in POLICY_LAYERS for t in (getattr(sac.policy, l).weight, getattr(sac.policy, l).bias)]
        crit_p = [t for l in CRITIC_LAYERS for t in (getattr(sac.critic, l).weight, getattr(sac.critic, l).bias)]
        tgt_p = [t for l in CRITIC_LAYERS for t in (getattr(sac.critic_target, l).weight, getattr(sac.critic_target, l).bias)]
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
        if self._bound != (ptrs, hyper) or not self.owns():
            self.engine.sac_bind(self.dims, self.tuning, hyper[0], hyper[1], hyper[2], hyper[3], [v for a in hyper[4] for v in a], ptrs)
            self.claim()
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
        width = row_width(self.dims[0], self.dims[1])
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
                for key, value in zip(LOG_KEYS, (reward, float(np.float32(res[i, 0]) + np.float32(res[i, 1])), pl,
                                                 self.sac.target_entropy if self.tuning else 0, entropy, al, alpha)):
                    logger.log(key, value, u)
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
