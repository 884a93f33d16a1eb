"""Engine: thin Python owner of one ``hipets_engine`` (one per GPU).  PyTorch is used only for
device memory and streams; every computation is a libhipets call."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import CemParams, HipetsError
from ._pack import (_check_dev, check_critic_split, check_discount, check_ensemble_shape, member_slots, pack_critic, pack_model_desc, pack_plan_trace,  # noqa: F401
                    pack_planet_desc, pack_reward_terms, pack_policy, pack_rollout_opts, pack_train_desc, row_width)
from .model import ModelSpec
from .reduce import ParticleReduce


def _address(v):
    """A void* argument that is neither a plain tensor nor None: a numpy array's or tensor subclass's data pointer; a ctypes object or
    an address goes as it is"""
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def _marshaller(params):
    """[(parameter name, ctype), ...] of one symbol -> a function of keyword arguments named as those parameters that returns the
    positional arguments in header order, built once per symbol.  Python's own argument binding refuses a missing or unknown name;
    ``e`` and ``stream`` are accepted for every symbol and dropped where the header has none.  Of the pointer parameters a tensor (or
    numpy array) goes as its data pointer and a bound struct by reference; None (NULL), a ctypes object or an address as it is.
    Scalars are not touched: ctypes wraps a Python int into a uint64_t."""
    def convert(n, t):
        if t is C.c_void_p and n not in ("e", "stream"):
            return f"{n}.data_ptr() if type({n}) is Tensor else {n} if {n} is None else address({n})"
        return f"byref({n}) if type({n}) in STRUCTS else {n}" if issubclass(t, C._Pointer) and t._type_ in _STRUCTS else n
    names = ["e", "stream"] + [n for n, _ in params if n not in ("e", "stream")]
    source = "lambda *, {}: ({})".format(", ".join(names), "".join(convert(n, t) + ", " for n, t in params))
    return eval(source, {"Tensor": torch.Tensor, "address": _address, "byref": C.byref, "STRUCTS": _STRUCTS})


_STRUCTS = frozenset(cls for cls in vars(_lib).values() if isinstance(cls, type) and issubclass(cls, C.Structure))
_MARSHAL = {name: _marshaller(params) for name, (_, params) in _lib.SYMBOLS.items()}


class Engine:
    """One fused planning engine bound to ``device`` (a gfx950 GPU).  Not thread-safe."""

    # the three slots of a SAC agent (hipets.sac), empty -- sizes and owner (a weakref) of the actor's snapshot, the critic's and the bound
    # agent -- and the SAC updates run so far.  (Class level: an Engine made without __init__ answers "has not been called" too.)
    policy_dims = policy_owner = critic_dims = critic_owner = sac_dims = sac_owner = None
    sac_updates = 0
    # the ensemble slot (hipets.ensemble): the spec whose snapshot hipets_ensemble_set took, and its owner (a weakref)
    ensemble_spec = ensemble_owner = None

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HipetsError("hipets.Engine needs a GPU device (libhipets has no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _lib.load()
        self._h = h = C.c_void_p()
        self._query("hipets_create", device=self.device.index, out=C.byref(h))
        self.spec: Optional[ModelSpec] = None
        self.planet_spec = None
        self.comm_world, self.comm_rank = 1, 0
        self.comm_group = None  # torch.distributed group of the communicator's ranks (hipets.dist.init_engine_comm)
        self.plan_mode = "fast"  # (the library's initial value; every fused plan sets its objective's mode: optimizers._prepare_fused)
        self.reduce = ParticleReduce()  # (the library's initial value, the mean; every objective sets its own: _Objective.bind_model)
        self._trace = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hipets_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the one call path ------------------------------------------------------------------------
    def _call(self, symbol: str, _enqueue: bool = True, **kw):
        """``symbol(**kw)`` with the keywords named as the parameters of include/hipets.h (``_lib.SYMBOLS``; ``e``, the handle, and
        ``stream``, the current stream of the engine's device, are filled in here), inside the engine's device scope.  The function is
        looked up on ``self._lib`` at every call and called positionally in header order (``_marshaller``; ``kw`` keeps a staged numpy
        array alive for the call).  A non-zero return code raises HipetsError."""
        args = _MARSHAL[symbol](e=self._h, stream=torch.cuda.current_stream(self.device).cuda_stream if _enqueue else None, **kw)
        fn = getattr(self._lib, symbol)
        if _enqueue:
            with torch.cuda.device(self.device):
                rc = fn(*args)
        else:
            rc = fn(*args)
        _lib.check(rc)

    def _query(self, symbol: str, **kw):
        """``_call`` for a host-only query or switch: no device scope"""
        self._call(symbol, False, **kw)

    # ---- model ------------------------------------------------------------------------------
    def set_model(self, spec: ModelSpec):
        spec.validate()
        ws = [w.detach().to(device=self.device, dtype=torch.float32).contiguous() for w in spec.weights]
        bs = [b.detach().to(device=self.device, dtype=torch.float32).contiguous() for b in spec.biases]
        d, cols, keep = pack_model_desc(spec, ws, bs)
        if cols is not None:
            self._call("hipets_set_model_columns", desc=d, cols=cols, n_cols=len(cols))
        else:
            self._call("hipets_set_model", desc=d)
        del keep
        self.spec = spec

    # ---- ModelEnv.evaluate_action_sequences ------------------------------------------------------
    def rollout(self, actions: torch.Tensor, s0: np.ndarray, num_particles: int, *, mode: str = "fast",
                perms: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None, seed: int = 0,
                stream_id: int = 0, member_schedule: Optional[torch.Tensor] = None,
                trace_next_obs: Optional[torch.Tensor] = None, trace_rewards: Optional[torch.Tensor] = None,
                rows_per_group: int = 0, out: Optional[torch.Tensor] = None,
                phase_cycles: Optional[torch.Tensor] = None, n_env: int = 1,
                members: Optional[torch.Tensor] = None, generic_kernel=False) -> torch.Tensor:
        """``members`` (EXACT mode): int64 [H, B] (random_model) or [B] (fixed_model) active-member slot of every row: the
        reference's ``torch.randint`` draws for BasicEnsemble models (basic_ensemble.py:122-129, 255-260), or any
        ``propagate_from_indices``-style assignment (util/math.py:180-196) for GaussianMLP models (no batch % members rule)."""
        if self.spec is None:
            raise HipetsError("Engine.set_model() has not been called")
        dev = self.device
        if actions.ndim != 3:
            raise ValueError("action_sequences must be [B, H, A]")
        _check_dev(actions, torch.float32, dev, "action_sequences")
        pop, H, A = actions.shape
        if A != self.spec.act_dim:
            raise ValueError(f"action dim {A} != model act_dim {self.spec.act_dim}")
        s0 = np.ascontiguousarray(np.asarray(s0, dtype=np.float32).reshape(-1))
        if s0.shape[0] != self.spec.obs_dim * max(1, n_env):
            raise ValueError(f"initial_state has {s0.shape[0]} values, expected n_env x obs_dim = {max(1, n_env)} x {self.spec.obs_dim}")
        if n_env > 1 and (mode not in ("fast", "device") or pop % n_env):
            raise ValueError("batched rollouts (n_env > 1) need mode='fast' or 'device' and a population divisible by n_env")
        o, keep = pack_rollout_opts(self.spec, dev, mode, pop * num_particles, H, perms, members, eps, seed, stream_id, member_schedule,
                                    rows_per_group, generic_kernel, n_env=n_env, trace_next_obs=trace_next_obs, trace_rewards=trace_rewards,
                                    phase_cycles=phase_cycles, n_workgroups=lambda: self.fast_geometry(pop, num_particles, H, rows_per_group)[0])
        if out is None:
            out = torch.empty(pop, dtype=torch.float32, device=dev)
        else:
            _check_dev(out, torch.float32, dev, "out", (pop,))
        self._call("hipets_rollout", actions=actions, s0=s0, pop=pop, horizon=H, num_particles=num_particles, opts=o, returns=out)
        del keep
        return out

    def step(self, obs: torch.Tensor, actions: torch.Tensor, *, mode: str = "fast", sample: bool = True,
             perm: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None, seed: int = 0, stream_id: int = 0,
             member_schedule: Optional[torch.Tensor] = None, rows_per_group: int = 0,
             members: Optional[torch.Tensor] = None, perm_stream_id: int = 0, generic_kernel=False):
        """One model transition for B independent rows (ModelEnv.step, mbrl/models/model_env.py:87-140).
        Returns (next_obs [B,obs], rewards [B,1], dones [B,1] bool) on the device.  ``members`` int64 [B]: EXACT-mode
        member of every row for BasicEnsemble models (GaussianMLP models take ``perm``).  ``perm_stream_id`` (DEVICE mode,
        fixed_model propagation): the stream whose TS-infinity permutation the step uses -- the rollout's reset -- while
        ``stream_id`` keys this step's eps; 0 = ``stream_id``.  ``generic_kernel`` as for :meth:`rollout`."""
        if self.spec is None:
            raise HipetsError("Engine.set_model() has not been called")
        dev = self.device
        B = int(obs.shape[0])
        _check_dev(obs, torch.float32, dev, "obs", (B, self.spec.obs_dim))
        _check_dev(actions, torch.float32, dev, "actions", (B, self.spec.act_dim))
        o, keep = pack_rollout_opts(self.spec, dev, mode, B, None, perm, members, eps, seed, stream_id, member_schedule, rows_per_group,
                                    generic_kernel, sample=sample, perm_stream_id=perm_stream_id)
        next_obs = torch.empty_like(obs)
        rewards = torch.empty(B, dtype=torch.float32, device=dev)
        dones = torch.empty(B, dtype=torch.uint8, device=dev)
        self._call("hipets_step", obs=obs, actions=actions, batch=B, opts=o, next_obs=next_obs, rewards=rewards, dones=dones)
        del keep
        return next_obs, rewards.view(B, 1), dones.view(B, 1).bool()

    def trajectory_returns(self, rewards: torch.Tensor, dones: torch.Tensor, pop: int, num_particles: int, *, row_totals: bool = False,
                           first_done: bool = False):
        """model_env.py:186-191 over a finished trajectory (hipets_trajectory_returns): ``rewards`` f32 [H, B] and ``dones`` bool or
        uint8 [H, B] (B = pop * num_particles, row c * P + p) -> ``returns`` f32 [pop]: per row the rewards up to and including the
        first step whose ``dones`` is set, summed in step order, then the particle mean of ``Engine.rollout``'s own returns.  With
        ``row_totals`` / ``first_done`` the result is the tuple (returns, row totals f32 [B] or None, first terminating step int32 [B]
        -- H where a row never terminates -- or None)."""
        dev = self.device
        if not isinstance(rewards, torch.Tensor) or rewards.ndim != 2:
            raise ValueError("rewards must be a [H, B] tensor")
        H, B = (int(v) for v in rewards.shape)
        if pop < 1 or num_particles < 1 or pop * num_particles != B:
            raise ValueError(f"rewards holds {B} rows per step, pop x num_particles = {pop} x {num_particles}")
        _check_dev(rewards, torch.float32, dev, "rewards")
        if isinstance(dones, torch.Tensor) and dones.dtype == torch.bool:
            dones = dones.view(torch.uint8)  # (one byte per element, 0 / 1)
        _check_dev(dones, torch.uint8, dev, "dones", (H, B))
        out = torch.empty(pop, dtype=torch.float32, device=dev)
        tot = torch.empty(B, dtype=torch.float32, device=dev) if row_totals else None
        first = torch.empty(B, dtype=torch.int32, device=dev) if first_done else None
        self._call("hipets_trajectory_returns", rewards=rewards, dones=dones, pop=int(pop), horizon=H, num_particles=int(num_particles),
                   returns=out, row_totals=tot, first_done=first)
        return (out, tot, first) if (row_totals or first_done) else out

    def fast_geometry(self, pop: int, num_particles: int, horizon: int, rows_per_group: int = 0):
        nwg, r = C.c_int32(), C.c_int32()
        self._query("hipets_fast_geometry", pop=pop, num_particles=num_particles, horizon=horizon, rows_per_group=rows_per_group,
                    n_workgroups=C.byref(nwg), row_tiles=C.byref(r))
        return nwg.value, r.value

    def kernel_class(self, pop: int, num_particles: int, horizon: int, mode: str = "device", rows_per_group: int = 0):
        """(class name, row tiles per workgroup) of the rollout-kernel instance a default rollout / fused plan of this size runs on
        the engine's model: "generic", "hidden_static", "fused", "wide" or "bf16" (the instances of precision="bf16") (include/hipets.h,
        hipets_kernel_class); ``rows_per_group``
        > 0: the answer for a call that forces that row-tile count.  Diagnostic."""
        cls, r = C.c_int32(), C.c_int32()
        self._query("hipets_kernel_class", pop=pop, num_particles=num_particles, horizon=horizon, mode=_lib.MODES[mode],
                    rows_per_group=int(rows_per_group), kernel_class=C.byref(cls), row_tiles=C.byref(r))
        return _lib.KERNEL_CLASSES[cls.value], r.value

    def _replay(self, symbol: str, out_name: str, shape, dtype, horizon: int, seed: int, stream_id: int, **size):
        """The randomness a rollout with (seed, stream_id) uses, exported into a fresh tensor (hipets_fast_schedule / _fast_normals /
        _device_perms: the horizon, one size, the keys, the output)"""
        out = torch.empty(shape, dtype=dtype, device=self.device)
        self._call(symbol, horizon=horizon, seed=int(seed), stream_id=int(stream_id), **size, **{out_name: out})
        return out

    def fast_schedule(self, horizon: int, n_workgroups: int, seed: int = 0, stream_id: int = 0) -> torch.Tensor:
        """The member schedule a FAST rollout with (seed, stream_id) uses: int32 [H, n_workgroups]."""
        return self._replay("hipets_fast_schedule", "schedule", (horizon, n_workgroups), torch.int32, horizon, seed, stream_id, n_workgroups=n_workgroups)

    def fast_normals(self, horizon: int, batch: int, seed: int = 0, stream_id: int = 0) -> torch.Tensor:
        """The eps a FAST rollout with (seed, stream_id) draws: f32 [H, B, out_dim]."""
        return self._replay("hipets_fast_normals", "normals", (horizon, batch, self.spec.out_dim), torch.float32, horizon, seed, stream_id, batch=batch)

    def device_perms(self, horizon: int, batch: int, seed: int = 0, stream_id: int = 0) -> torch.Tensor:
        """The permutations a DEVICE-mode rollout with (seed, stream_id) uses, in the reference's convention
        (``model_shuffle_indices``): int64 [H, B] for random_model, [B] for fixed_model."""
        fixed = self.spec.propagation == "fixed_model"
        out = self._replay("hipets_device_perms", "perms", (1 if fixed else horizon, batch), torch.int64, horizon, seed, stream_id, batch=batch)
        return out[0] if fixed else out

    def set_plan_mode(self, mode: str):
        """Randomness mode of the rollouts inside the fused plans: 'fast' or 'device'."""
        if mode not in ("fast", "device"):
            raise ValueError("plan mode must be 'fast' or 'device'")
        self._query("hipets_set_plan_mode", mode=_lib.MODES[mode])
        self.plan_mode = mode

    def set_particle_reduce(self, reduce: ParticleReduce):
        """How every call that reduces a candidate's particles forms its value from now on (hipets_set_particle_reduce): rollouts,
        ``trajectory_returns``, ``particle_reduce`` and every fused plan.  ``reduce``: a resolved reduction (``ParticleReduce.resolve``)."""
        self._query("hipets_set_particle_reduce", **reduce.abi_args())
        self.reduce = reduce

    def particle_reduce(self, totals: torch.Tensor, pop: int, num_particles: int) -> torch.Tensor:
        """``totals`` f32 [pop * num_particles] (row c * P + p) -> f32 [pop] under the engine's reduction (hipets_particle_reduce)."""
        _check_dev(totals, torch.float32, self.device, "totals", numel=int(pop) * int(num_particles))
        out = torch.empty(int(pop), dtype=torch.float32, device=self.device)
        self._call("hipets_particle_reduce", totals=totals, pop=int(pop), num_particles=int(num_particles), returns=out)
        return out

    def set_persistent(self, on: bool = True):
        """Allow (default) or forbid the persistent one-launch form of DEVICE-mode rollouts (hipets_set_persistent)."""
        self._query("hipets_set_persistent", on=int(bool(on)))

    def synchronize(self):
        """Wait for everything enqueued on this engine's device (torch.cuda.synchronize)."""
        torch.cuda.synchronize(self.device)

    def set_handover_timeout(self, seconds: float = 0.2):
        """Bound of every hand-over poll of the persistent DEVICE-mode form (hipets_set_handover_timeout)."""
        self._query("hipets_set_handover_timeout", seconds=float(seconds))

    def check_async_error(self) -> bool:
        """True if a persistent DEVICE-mode rollout enqueued on this engine gave up waiting for another workgroup's rows
        (hipets_check_async_error): call after the results reached the host; on True they are invalid, the engine has
        switched to per-step launches and the call must be re-run (``TrajectoryOptimizer.optimize`` does)."""
        flag = C.c_int32(0)
        self._query("hipets_check_async_error", timed_out=C.byref(flag))
        return bool(flag.value)

    def set_plan_trace(self, iters: int = 0, max_rows: int = 0, horizon: int = 0, act_dim: int = 0, elite_num: int = 0, n_env: int = 1):
        """Record the following fused plans iteration by iteration (hipets_set_plan_trace); returns the dict of device
        tensors the library writes into.  ``iters=0`` switches recording off.  ``max_rows`` counts the candidates of ALL
        environments of a batched plan."""
        if iters <= 0:
            self._query("hipets_set_plan_trace", trace=None)
            self._trace = None
            return None
        dev = self.device
        env = (iters,) if n_env == 1 else (iters, n_env)
        tr = {"populations": torch.zeros(iters, max_rows, horizon, act_dim, device=dev), "values": torch.zeros(iters, max_rows, device=dev),
              "mus": torch.zeros(*env, horizon, act_dim, device=dev), "dispersions": torch.zeros(*env, horizon, act_dim, device=dev),
              "elite_idx": torch.zeros(*env, max(1, elite_num), dtype=torch.int32, device=dev)}
        self._query("hipets_set_plan_trace", trace=pack_plan_trace(tr, max_rows)[0])
        self._trace = tr  # keeps the buffers alive while the library holds their addresses
        return tr

    # ---- optimizer pieces ---------------------------------------------------------------------------
    @staticmethod
    def cem_params(population_size, horizon, act_dim, num_iterations, elite_num, alpha, return_mean_elites=False,
                   clipped_normal=False, unbiased_var=True) -> CemParams:
        p = CemParams()
        p.population_size, p.horizon, p.act_dim = int(population_size), int(horizon), int(act_dim)
        p.num_iterations, p.elite_num, p.alpha = int(num_iterations), int(elite_num), float(alpha)
        p.return_mean_elites, p.clipped_normal, p.unbiased_var = int(return_mean_elites), int(clipped_normal), int(unbiased_var)
        return p

    def cem_sample(self, p: CemParams, mu, dispersion, lower, upper, population, z=None, seed=0, stream_id=0):
        dev = self.device
        D = p.horizon * p.act_dim
        for n_, t in (("mu", mu), ("dispersion", dispersion), ("lower", lower), ("upper", upper)):
            _check_dev(t, torch.float32, dev, n_, numel=D)
        _check_dev(population, torch.float32, dev, "population", numel=p.population_size * D)
        if z is not None:
            _check_dev(z, torch.float32, dev, "z", numel=p.population_size * D)
        self._call("hipets_cem_sample", p=p, mu=mu, dispersion=dispersion, lower=lower, upper=upper, z=z, seed=int(seed),
                   stream_id=int(stream_id), population=population)
        return population

    def cem_refit(self, p: CemParams, values, population, mu, dispersion, best_value, best_solution, elite_idx=None, elites=None):
        """``elites`` int32 [elite_num] (device): refit on THESE candidates, best first, instead of the kernel's own top-k
        (hipets_cem_refit_elites: the reference-order parity mode passes torch.topk's indices, ties and all)."""
        dev = self.device
        D = p.horizon * p.act_dim
        _check_dev(values, torch.float32, dev, "values", (p.population_size,))
        _check_dev(population, torch.float32, dev, "population", numel=p.population_size * D)
        for n_, t in (("mu", mu), ("dispersion", dispersion), ("best_solution", best_solution)):
            _check_dev(t, torch.float32, dev, n_, numel=D)
        _check_dev(best_value, torch.float32, dev, "best_value", (1,))
        if elite_idx is not None:
            _check_dev(elite_idx, torch.int32, dev, "elite_idx", (p.elite_num,))
        state = dict(p=p, values=values, population=population, mu=mu, dispersion=dispersion, best_value=best_value, best_solution=best_solution)
        if elites is None:
            self._call("hipets_cem_refit", elite_idx=elite_idx, **state)
            return
        _check_dev(elites, torch.int32, dev, "elites", (p.elite_num,))
        # (this path follows a host-side torch.topk, i.e. it has synchronised with the host already: the range check is free)
        lo, hi = int(elites.min()), int(elites.max())
        if lo < 0 or hi >= p.population_size:
            raise ValueError(f"elites must index the population [0, {p.population_size}): got {lo} .. {hi}")
        self._call("hipets_cem_refit_elites", elites=elites, **state)
        if elite_idx is not None:
            elite_idx.copy_(elites)

    def gather_rows(self, src: torch.Tensor, index: torch.Tensor, out: torch.Tensor):
        dev = self.device
        rows, dim = int(index.numel()), int(out.numel() // max(1, index.numel()))
        _check_dev(src, torch.float32, dev, "src")
        _check_dev(index, torch.int32, dev, "index")
        _check_dev(out, torch.float32, dev, "out", numel=rows * dim)
        self._call("hipets_gather_rows", rows=rows, dim=dim, src=src, index=index, dst=out)
        return out

    def mppi_sample(self, pop, H, A, beta, mean, past_action, lower, upper, population, z=None, seed=0, stream_id=0):
        dev = self.device
        for n_, t in (("mean", mean), ("lower", lower), ("upper", upper)):
            _check_dev(t, torch.float32, dev, n_, numel=H * A)
        _check_dev(past_action, torch.float32, dev, "past_action", numel=A)
        _check_dev(population, torch.float32, dev, "population", numel=pop * H * A)
        if z is not None:
            _check_dev(z, torch.float32, dev, "z", numel=pop * H * A)
        self._call("hipets_mppi_sample", pop=pop, horizon=H, act_dim=A, beta=float(beta), mean=mean, past_action=past_action, lower=lower,
                   upper=upper, z=z, seed=int(seed), stream_id=int(stream_id), population=population)
        return population

    def mppi_update(self, pop, H, A, gamma, values, population, mean):
        dev = self.device
        _check_dev(values, torch.float32, dev, "values", (pop,))
        _check_dev(population, torch.float32, dev, "population", numel=pop * H * A)
        _check_dev(mean, torch.float32, dev, "mean", numel=H * A)
        self._call("hipets_mppi_update", pop=pop, horizon=H, act_dim=A, gamma=float(gamma), values=values, population=population, mean=mean)
        return mean

    def icem_sample(self, n, H, A, exponent, mu, var, lower, upper, population, normals=None, seed=0, stream_id=0):
        dev = self.device
        for n_, t in (("mu", mu), ("var", var), ("lower", lower), ("upper", upper)):
            _check_dev(t, torch.float32, dev, n_, numel=H * A)
        _check_dev(population, torch.float32, dev, "population")
        if population.numel() < n * H * A:
            raise ValueError("population buffer too small")
        if normals is not None:
            _check_dev(normals, torch.float32, dev, "normals", (2, n, A, H // 2 + 1))
        self._call("hipets_icem_sample", n=n, horizon=H, act_dim=A, exponent=float(exponent), mu=mu, var=var, lower=lower, upper=upper,
                   normals=normals, seed=int(seed), stream_id=int(stream_id), population=population)
        return population

    def icem_shift(self, keep, H, A, kept, mu, var, out, end_noise=None, seed=0, stream_id=0):
        dev = self.device
        _check_dev(kept, torch.float32, dev, "kept", numel=keep * H * A)
        _check_dev(out, torch.float32, dev, "out", numel=keep * H * A)
        for n_, t in (("mu", mu), ("var", var)):
            _check_dev(t, torch.float32, dev, n_, numel=H * A)
        if end_noise is not None:
            _check_dev(end_noise, torch.float32, dev, "end_noise", numel=keep * A)
        self._call("hipets_icem_shift", keep=keep, horizon=H, act_dim=A, kept=kept, mu=mu, var=var, end_noise=end_noise, seed=int(seed),
                   stream_id=int(stream_id), out=out)
        return out

    # ---- fused plans: one body per optimizer; the public methods choose the symbol and the start state -----------------------------
    def _plan_args(self, symbol: str, tensors, n_env: int, seed: int, plan_id: int, s0=None, latent0=None, belief0=None) -> dict:
        """The checks every plan shares, in this order: the bound model (the ensemble for ``s0``, the PlaNet model for ``latent0``
        / ``belief0``); ``tensors``, (name, tensor, shape tuple or element count) on the device, float32 (keep_idx: int32; None: not
        passed); the start state, host s0 of n_env x obs_dim values or device latent0 [n_env, latent] / belief0 [n_env, belief].
        Returns the arguments the plans of all optimizers share: the start state, seed and plan id, n_env for a ``_batched`` symbol."""
        planet = s0 is None
        spec = self.planet_spec if planet else self.spec
        if spec is None:
            raise HipetsError("Engine.planet_set_model() has not been called" if planet else "Engine.set_model() has not been called")
        for name, t, size in tensors:
            if t is not None:
                dtype = torch.int32 if name == "keep_idx" else torch.float32
                _check_dev(t, dtype, self.device, name, **({"shape": size} if isinstance(size, tuple) else {"numel": size}))
        args = {"seed": int(seed), "plan_id": int(plan_id)}
        if symbol.endswith("_batched"):
            args["n_env"] = int(n_env)
        if planet:
            _check_dev(latent0, torch.float32, self.device, "latent0", numel=n_env * spec.latent_size)
            _check_dev(belief0, torch.float32, self.device, "belief0", numel=n_env * spec.belief_size)
            args["latent0"], args["belief0"] = latent0, belief0
            return args
        s0 = np.ascontiguousarray(np.asarray(s0, dtype=np.float32).reshape(-1))
        if s0.shape[0] != spec.obs_dim * n_env:
            expected = spec.obs_dim if symbol.endswith("_sharded") else f"{n_env} x {spec.obs_dim}"
            raise ValueError(f"initial_state has {s0.shape[0]} values, expected {expected}")
        args["s0"] = s0
        return args

    def _plan_cem(self, symbol: str, p, x0, lower, upper, num_particles, seed, plan_id, out, n_env: int = 1, **start):
        """A sharded plan takes x0 exactly [H, A] and returns [H, A]; the others x0 of n_env x H x A elements and return its shape"""
        shp, sharded = (p.horizon, p.act_dim), symbol.endswith("_sharded")
        args = self._plan_args(symbol, [("x0", x0, shp if sharded else n_env * p.horizon * p.act_dim), ("lower", lower, shp), ("upper", upper, shp)],
                               n_env, seed, plan_id, **start)
        if out is None:
            out = torch.empty(shp if sharded else tuple(x0.shape), dtype=torch.float32, device=self.device)  # [H, A] or [n_env, H, A]
        self._call(symbol, p=p, x0=x0, lower=lower, upper=upper, num_particles=num_particles, out=out, **args)
        return out

    def _plan_mppi(self, symbol: str, pop, H, A, num_iterations, gamma, beta, mean, lower, upper, num_particles, seed, plan_id, n_env: int = 1,
                   **start):
        args = self._plan_args(symbol, [("mean", mean, (H, A) if symbol.endswith("_sharded") else n_env * H * A), ("lower", lower, (H, A)),
                                        ("upper", upper, (H, A))], n_env, seed, plan_id, **start)
        self._call(symbol, population_size=pop, horizon=H, act_dim=A, num_iterations=num_iterations, gamma=float(gamma), beta=float(beta),
                   mean=mean, lower=lower, upper=upper, num_particles=num_particles, **args)
        return mean

    def _plan_icem(self, symbol: str, p, x0, lower, upper, elite, has_elite, num_particles, seed, plan_id, keep_idx, out, n_env: int = 1, **start):
        shp, nd, sharded = (p.horizon, p.act_dim), p.horizon * p.act_dim, symbol.endswith("_sharded")
        args = self._plan_args(symbol, [("x0", x0, shp if sharded else n_env * nd), ("lower", lower, shp), ("upper", upper, shp),
                                        ("elite", elite, n_env * p.elite_num * nd), ("keep_idx", keep_idx, p.num_iterations * n_env * p.keep_elite_size)],
                               n_env, seed, plan_id, **start)
        if out is None:
            out = torch.empty(shp if sharded else tuple(x0.shape), dtype=torch.float32, device=self.device)
        self._call(symbol, p=p, x0=x0, lower=lower, upper=upper, elite=elite, has_elite=int(bool(has_elite)), keep_idx=keep_idx,
                   num_particles=num_particles, out=out, **args)
        return out

    def plan_cem(self, p: CemParams, x0, lower, upper, s0: np.ndarray, num_particles: int, seed: int = 0,
                 plan_id: int = 0, out: Optional[torch.Tensor] = None, n_env: int = 1) -> torch.Tensor:
        """Whole CEM plan on the device.  n_env > 1: x0 / out are [n_env, H, A], s0 is [n_env, obs_dim]; p.population_size is
        per environment (hipets_plan_cem_batched)."""
        return self._plan_cem("hipets_plan_cem_batched", p, x0, lower, upper, num_particles, seed, plan_id, out, n_env, s0=s0)

    def plan_mppi(self, pop: int, H: int, A: int, num_iterations: int, gamma: float, beta: float, mean: torch.Tensor, lower,
                  upper, s0: np.ndarray, num_particles: int, seed: int = 0, plan_id: int = 0, n_env: int = 1) -> torch.Tensor:
        """Whole MPPI plan on the device (hipets_plan_mppi[_batched]).  ``mean`` [H, A] ([n_env, H, A] for a batch of
        environments, ``s0`` then [n_env, obs_dim]) is the optimizer's persistent mean: shifted and refined IN PLACE."""
        return self._plan_mppi("hipets_plan_mppi_batched", pop, H, A, num_iterations, gamma, beta, mean, lower, upper, num_particles, seed, plan_id,
                               n_env, s0=s0)

    def plan_icem(self, p: "_lib.IcemParams", x0, lower, upper, elite: torch.Tensor, has_elite: bool, s0: np.ndarray,
                  num_particles: int, seed: int = 0, plan_id: int = 0, keep_idx: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, n_env: int = 1) -> torch.Tensor:
        """Whole iCEM plan on the device (hipets_plan_icem[_batched]).  ``elite`` [elite_num, H, A] is the optimizer's
        persistent elite set (read when ``has_elite``, always overwritten); ``keep_idx`` int32 [num_iterations, keep]
        optionally injects the kept-elite draws.  n_env > 1: x0 / out [n_env, H, A], elite [n_env, elite_num, H, A],
        keep_idx [num_iterations, n_env, keep], s0 [n_env, obs_dim]."""
        return self._plan_icem("hipets_plan_icem_batched", p, x0, lower, upper, elite, has_elite, num_particles, seed, plan_id, keep_idx, out,
                               n_env, s0=s0)

    # ---- in-library RCCL communicator (population-sharded fused plans) -----------------------------
    def comm_unique_id(self) -> bytes:
        """A fresh communicator id (rank 0 makes it, the host broadcasts the bytes to the other ranks)."""
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        self._query("hipets_comm_unique_id", id_out=buf)
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world_size: int):
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {_lib.COMM_ID_BYTES} bytes")
        self._call("hipets_comm_init", unique_id=C.c_char_p(unique_id), rank=int(rank), world_size=int(world_size))
        self.comm_world, self.comm_rank = int(world_size), int(rank)

    def comm_destroy(self):
        self._query("hipets_comm_destroy")
        self.comm_world, self.comm_rank, self.comm_group = 1, 0, None

    def comm_info(self) -> tuple:
        """(rank, world size) as the communicator itself reports them (hipets_comm_info)."""
        r, w = C.c_int32(0), C.c_int32(1)
        self._query("hipets_comm_info", rank=C.byref(r), world_size=C.byref(w))
        return r.value, w.value

    def plan_cem_sharded(self, p: CemParams, x0, lower, upper, s0: np.ndarray, num_particles: int, seed: int = 0, plan_id: int = 0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """hipets_plan_cem over all ranks of the communicator (identical arguments on every rank)."""
        return self._plan_cem("hipets_plan_cem_sharded", p, x0, lower, upper, num_particles, seed, plan_id, out, s0=s0)

    def plan_mppi_sharded(self, pop: int, H: int, A: int, num_iterations: int, gamma: float, beta: float, mean: torch.Tensor, lower,
                          upper, s0: np.ndarray, num_particles: int, seed: int = 0, plan_id: int = 0) -> torch.Tensor:
        """hipets_plan_mppi over all ranks of the communicator (identical arguments on every rank; ``mean`` in place)."""
        return self._plan_mppi("hipets_plan_mppi_sharded", pop, H, A, num_iterations, gamma, beta, mean, lower, upper, num_particles, seed, plan_id,
                               s0=s0)

    def plan_icem_sharded(self, p: "_lib.IcemParams", x0, lower, upper, elite: torch.Tensor, has_elite: bool, s0: np.ndarray,
                          num_particles: int, seed: int = 0, plan_id: int = 0, keep_idx: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """hipets_plan_icem over all ranks of the communicator (identical arguments on every rank; ``elite`` in place)."""
        return self._plan_icem("hipets_plan_icem_sharded", p, x0, lower, upper, elite, has_elite, num_particles, seed, plan_id, keep_idx, out, s0=s0)

    # ---- PlaNet latent planner -----------------------------------------------
    def planet_set_model(self, spec):
        """Pack the planning heads of a PlaNet model (``hipets.PlaNetSpec``)."""
        spec.validate()
        d, keep = pack_planet_desc(spec, [getattr(spec, n).detach().to(device=self.device, dtype=torch.float32).contiguous()
                                          for n in _lib._PLANET_TENSORS])
        self._call("hipets_planet_set_model", d=d)
        del keep
        self.planet_spec = spec

    def planet_rollout(self, actions: torch.Tensor, latent0: torch.Tensor, belief0: torch.Tensor, num_particles: int, *,
                       eps: Optional[torch.Tensor] = None, sample: bool = True, seed: int = 0, stream_id: int = 0,
                       trace_latent: Optional[torch.Tensor] = None, trace_belief: Optional[torch.Tensor] = None,
                       trace_rewards: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       phase_cycles: Optional[torch.Tensor] = None, n_env: int = 1) -> torch.Tensor:
        """ModelEnv.evaluate_action_sequences on the PlaNet model (model_env.py:145-191): actions [pop, H, A]; latent0 /
        belief0 = the saved posterior sample / belief ([latent] / [belief], any leading 1s) on the device.  ``n_env > 1``: the
        pop candidates are n_env groups of pop / n_env, group g starts from latent0[g] / belief0[g] ([n_env, latent] /
        [n_env, belief]); eps and the traces stay indexed by the launch-global row."""
        spec = self.planet_spec
        if spec is None:
            raise HipetsError("Engine.planet_set_model() has not been called")
        dev = self.device
        if actions.ndim != 3:
            raise ValueError("action_sequences must be [B, H, A]")
        _check_dev(actions, torch.float32, dev, "action_sequences")
        pop, H, A = actions.shape
        if A != spec.action_size:
            raise ValueError(f"action dim {A} != model action_size {spec.action_size}")
        _check_dev(latent0, torch.float32, dev, "latent0", numel=n_env * spec.latent_size)
        _check_dev(belief0, torch.float32, dev, "belief0", numel=n_env * spec.belief_size)
        B = pop * num_particles
        o = _lib.PlanetOpts(seed=int(seed), stream_id=int(stream_id), no_sample=int(not sample), n_env=int(n_env))
        # (phase_cycles is filled by -DHIPETS_LEAN_PROF=1 builds only: profiles/one_tile_phase_profile.py)
        for name, t, dtype, shape in (("eps", eps, torch.float32, (H, B, spec.latent_size)), ("trace_latent", trace_latent, torch.float32, (H, B, spec.latent_size)),
                                      ("trace_belief", trace_belief, torch.float32, (H, B, spec.belief_size)),
                                      ("trace_rewards", trace_rewards, torch.float32, (H, B)), ("phase_cycles", phase_cycles, torch.int64, (8, 16))):
            if t is not None:
                _check_dev(t, dtype, dev, name, shape)
                setattr(o, name, t.data_ptr())
        if out is None:
            out = torch.empty(pop, dtype=torch.float32, device=dev)
        else:
            _check_dev(out, torch.float32, dev, "out", (pop,))
        self._call("hipets_planet_rollout", actions=actions, latent0=latent0, belief0=belief0, pop=pop, horizon=H, num_particles=num_particles,
                   opts=o, returns=out)
        return out

    def planet_kernel_class(self) -> str:
        """Which instance of the PlaNet rollout kernel the next launch runs for the model set last: "static" (specialised for the tile
        counts of conf/dynamics_model/planet.yaml) or "generic" (every other model, and every model under HIPETS_PLANET_GENERIC=1)."""
        is_static = C.c_int32(-1)
        self._query("hipets_planet_kernel_class", is_static=C.byref(is_static))
        return "static" if is_static.value else "generic"

    def plan_planet_cem(self, p: CemParams, x0, lower, upper, latent0: torch.Tensor, belief0: torch.Tensor, num_particles: int,
                        seed: int = 0, plan_id: int = 0, out: Optional[torch.Tensor] = None, n_env: int = 1) -> torch.Tensor:
        """Whole CEM plan over the PlaNet latent model on the device.  x0 [H, A] with n_env = 1: hipets_plan_planet_cem; else
        hipets_plan_planet_cem_batched with x0 / out [n_env, H, A], latent0 [n_env, latent], belief0 [n_env, belief] and
        p.population_size per environment."""
        symbol = "hipets_plan_planet_cem" if n_env == 1 and getattr(x0, "ndim", 0) == 2 else "hipets_plan_planet_cem_batched"
        return self._plan_cem(symbol, p, x0, lower, upper, num_particles, seed, plan_id, out, n_env, latent0=latent0, belief0=belief0)

    def plan_planet_mppi(self, pop: int, H: int, A: int, num_iterations: int, gamma: float, beta: float, mean: torch.Tensor, lower, upper,
                         latent0: torch.Tensor, belief0: torch.Tensor, num_particles: int, seed: int = 0, plan_id: int = 0,
                         n_env: int = 1) -> torch.Tensor:
        """Whole MPPI plan over the PlaNet latent model (hipets_plan_planet_mppi_batched): ``mean`` [n_env, H, A] is the persistent
        mean of every environment, shifted and refined IN PLACE; latent0 [n_env, latent], belief0 [n_env, belief]."""
        return self._plan_mppi("hipets_plan_planet_mppi_batched", pop, H, A, num_iterations, gamma, beta, mean, lower, upper, num_particles, seed,
                               plan_id, n_env, latent0=latent0, belief0=belief0)

    def plan_planet_icem(self, p: "_lib.IcemParams", x0, lower, upper, elite: torch.Tensor, has_elite: bool, latent0: torch.Tensor,
                         belief0: torch.Tensor, num_particles: int, seed: int = 0, plan_id: int = 0, keep_idx: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None, n_env: int = 1) -> torch.Tensor:
        """Whole iCEM plan over the PlaNet latent model (hipets_plan_planet_icem_batched); arguments as :meth:`plan_icem` with
        latent0 [n_env, latent] / belief0 [n_env, belief] in place of s0."""
        return self._plan_icem("hipets_plan_planet_icem_batched", p, x0, lower, upper, elite, has_elite, num_particles, seed, plan_id, keep_idx, out,
                               n_env, latent0=latent0, belief0=belief0)

    # ---- GaussianMLP ensemble training (hipets_train_steps / hipets_train_eval) ------------------------------------------
    def train_steps(self, weights, biases, exp_avg, exp_avg_sq, min_logvar, max_logvar, x: torch.Tensor, y: torch.Tensor,
                    idx: torch.Tensor, rows: torch.Tensor, step0: int, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                    weight_decay: float = 0.0, activation: str = "silu", leaky_slope: float = 0.01, steps_per_launch: int = 0,
                    loss: str = "nll", grad_scale: float = 1.0, bounds_per_member: bool = False):
        """``n_steps = idx.shape[0]`` minibatch steps of Model.update + torch.optim.Adam on every member, in place on the DEVICE
        tensors ``weights`` / ``biases`` and the Adam state ``exp_avg`` / ``exp_avg_sq`` (pairs of per-layer lists (w, b)).
        x [N, in] / y [N, out] f32 = the dataset's model inputs and targets; idx int32 [n_steps, E, max_batch] its rows per
        (step, member); rows int32 [n_steps] the rows of each step; step0 = Adam steps taken before.  Returns (loss, grad_sq)
        DEVICE f32 [n_steps, E] (hipets.h: hipets_train_steps).  Asynchronous on the current stream.
        ``loss`` "mse": a deterministic model (last layer out wide, bounds None, loss = the member's sum of squared errors);
        ``bounds_per_member``: min_logvar / max_logvar are [E, out]; ``grad_scale`` multiplies the loss gradient (1 / E for a
        BasicEnsemble).  Any of them off its default goes through hipets_train_steps_loss."""
        dev = self.device
        out_dim = int(y.shape[-1]) if y.dim() == 2 else -1
        _check_dev(x, torch.float32, dev, "x")
        _check_dev(y, torch.float32, dev, "y")
        if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0]:
            raise ValueError("x / y must be [N, in] / [N, out] with the same N")
        _check_dev(idx, torch.int32, dev, "idx")
        if idx.dim() != 3:
            raise ValueError("idx must be [n_steps, E, max_batch]")
        n_steps, E, max_batch = (int(v) for v in idx.shape)
        if E != int(weights[0].shape[0]):
            raise ValueError(f"idx has {E} members, the model {int(weights[0].shape[0])}")
        _check_dev(rows, torch.int32, dev, "rows", numel=n_steps)
        d, keep = pack_train_desc(dev, weights, biases, activation, leaky_slope, out_dim, max_batch,
                                  adam=(exp_avg[0], exp_avg[1], exp_avg_sq[0], exp_avg_sq[1], min_logvar, max_logvar, lr, betas[0], betas[1],
                                        eps, weight_decay, steps_per_launch), loss=loss, bounds_per_member=bounds_per_member)
        losses = torch.empty(n_steps, E, dtype=torch.float32, device=dev)
        gsq = torch.empty(n_steps, E, dtype=torch.float32, device=dev)
        kw = dict(d=d, x=x, y=y, n_rows=int(x.shape[0]), idx=idx, rows=rows, n_steps=n_steps, step0=int(step0), loss=losses, grad_sq=gsq)
        if loss == "nll" and not bounds_per_member and float(grad_scale) == 1.0:
            self._call("hipets_train_steps", **kw)
        else:
            self._call("hipets_train_steps_loss", loss_kind=_lib.TRAIN_LOSS[loss], bounds_per_member=int(bool(bounds_per_member)),
                       grad_scale=float(grad_scale), **kw)
        del keep
        return losses, gsq

    def train_eval(self, weights, biases, x: torch.Tensor, y: torch.Tensor, order: Optional[torch.Tensor] = None, *,
                   activation: str = "silu", leaky_slope: float = 0.01, row_scores: bool = False, loss: str = "nll"):
        """GaussianMLP.eval_score averaged over rows and dims, per member: DEVICE f32 [E] (and, with ``row_scores``, the
        [E, N] per-row squared-error sums in pass order).  Asynchronous on the current stream.  ``loss`` "mse": the last layer is
        out wide (a deterministic model), through hipets_train_eval_loss."""
        dev = self.device
        _check_dev(x, torch.float32, dev, "x")
        _check_dev(y, torch.float32, dev, "y")
        if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0]:
            raise ValueError("x / y must be [N, in] / [N, out] with the same N")
        N = int(x.shape[0])
        if order is not None:
            _check_dev(order, torch.int32, dev, "order", numel=N)
        d, keep = pack_train_desc(dev, weights, biases, activation, leaky_slope, int(y.shape[1]), 1, loss=loss)
        E = int(weights[0].shape[0])
        score = torch.empty(E, dtype=torch.float32, device=dev)
        rs = torch.empty(E, N, dtype=torch.float32, device=dev) if row_scores else None
        if loss == "nll":
            self._call("hipets_train_eval", d=d, x=x, y=y, n_rows=N, order=order, score=score, row_score=rs)
        else:
            self._call("hipets_train_eval_loss", d=d, x=x, y=y, n_rows=N, order=order, score=score, row_score=rs, loss_kind=_lib.TRAIN_LOSS[loss])
        del keep
        return (score, rs) if row_scores else score

    # ---- MBPO model rollouts: the SAC Gaussian actor and the compacting populate step (hipets_policy_* / hipets_compact_transitions) ----
    def policy_set(self, policy):
        """Snapshot a ``GaussianPolicy``-shaped module's live weights into the engine (hipets_policy_set; ``_pack.pack_policy`` reads
        the module or raises UnsupportedModelError).  Device to device where the policy is on this GPU.  Asynchronous."""
        dims, tensors = pack_policy(policy)
        on_dev = {n: t.to(device=self.device, dtype=torch.float32).contiguous() for n, t in tensors.items()}
        self._call("hipets_policy_set", obs_dim=dims[0], hidden=dims[1], act_dim=dims[2], **on_dev)
        self.policy_dims = dims
        return dims

    def _slot_dims(self, slot: str, setter: str):
        dims = getattr(self, slot + "_dims")
        if dims is None:
            raise HipetsError(f"Engine.{setter}() has not been called")
        return dims

    def policy_act(self, obs: torch.Tensor, *, sample: bool = False, seed: int = 0, stream_id: int = 0, eps: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, taps: bool = False):
        """The actor's forward for ``obs`` f32 [B, obs_dim] on the device -> actions f32 [B, act_dim] (hipets_policy_act): the
        policy's mean action, or with ``sample`` a draw with ``eps`` f32 [B, act_dim] (None: drawn in-kernel from (seed, stream_id),
        see :meth:`policy_normals`).  ``taps``: returns (actions, mean, log_std), the heads before tanh."""
        obs_dim, _, act_dim = self._slot_dims("policy", "policy_set")
        dev = self.device
        if not isinstance(obs, torch.Tensor) or obs.ndim != 2 or int(obs.shape[0]) < 1:
            raise ValueError("obs must be a [B, obs_dim] tensor with B >= 1")
        B = int(obs.shape[0])
        _check_dev(obs, torch.float32, dev, "obs", (B, obs_dim))
        if eps is not None:
            _check_dev(eps, torch.float32, dev, "eps", (B, act_dim))
        if out is None:
            out = torch.empty(B, act_dim, dtype=torch.float32, device=dev)
        else:
            _check_dev(out, torch.float32, dev, "out", (B, act_dim))
        mean = torch.empty_like(out) if taps else None
        log_std = torch.empty_like(out) if taps else None
        self._call("hipets_policy_act", obs=obs, batch=B, sample=int(bool(sample)), seed=int(seed), stream_id=int(stream_id), eps=eps,
                   actions=out, mean_out=mean, log_std_out=log_std)
        return (out, mean, log_std) if taps else out

    def policy_normals(self, batch: int, act_dim: int, seed: int = 0, stream_id: int = 0) -> torch.Tensor:
        """The eps a sampling :meth:`policy_act` of ``batch`` rows draws in-kernel for (seed, stream_id): f32 [batch, act_dim]."""
        out = torch.empty(int(batch), int(act_dim), dtype=torch.float32, device=self.device)
        self._call("hipets_policy_normals", batch=int(batch), act_dim=int(act_dim), seed=int(seed), stream_id=int(stream_id), out=out)
        return out

    def policy_geometry(self, batch: int):
        """(row tiles per workgroup -- a workgroup owns 16 of them rows --, dynamic LDS bytes) of a :meth:`policy_act` of ``batch`` rows."""
        self._slot_dims("policy", "policy_set")
        return self._geometry("hipets_policy_geometry", batch)

    def _geometry(self, symbol: str, batch: int):
        r, lds = C.c_int32(), C.c_int32()
        self._query(symbol, batch=int(batch), row_tiles=C.byref(r), lds_bytes=C.byref(lds))
        return r.value, lds.value

    def compact_transitions(self, obs, action, next_obs, rewards, dones, accum_dones, staging, cap, offset, count_out):
        """mbpo.py:53-63 for one rollout step (hipets_compact_transitions): the rows whose ``accum_dones`` (uint8 [N], updated in
        place: ``|= dones``) is 0 are appended in row order to ``staging``, a flat f32 buffer of at least ``cap * (2 obs_dim + act_dim +
        2)`` elements holding five arrays one behind the other -- obs [cap, obs_dim], action [cap, act_dim], next_obs [cap, obs_dim],
        reward [cap], done [cap] (``hipets._pack.staging_views`` splits it) -- at row ``offset`` (int64 [1], advanced); ``count_out``
        int32 [1] = the rows kept.  All tensors on the device; ``rewards`` f32 and ``dones`` bool / uint8 of N elements."""
        N, od, ad, dones, cap = self._check_step_rows(obs, action, next_obs, rewards, dones, accum_dones, staging, cap, "staging", "cap")
        _check_dev(offset, torch.int64, self.device, "offset", numel=1)
        _check_dev(count_out, torch.int32, self.device, "count_out", numel=1)
        self._call("hipets_compact_transitions", obs=obs, action=action, next_obs=next_obs, rewards=rewards, dones=dones, accum_dones=accum_dones,
                   n=N, obs_dim=od, act_dim=ad, staging=staging, cap=cap, offset=offset, count_out=count_out)

    def _check_step_rows(self, obs, action, next_obs, rewards, dones, accum_dones, area, cap, area_name, cap_name):
        """The argument checks the two compactions share: (N, obs_dim, act_dim, dones as uint8, cap)"""
        dev = self.device
        if not isinstance(obs, torch.Tensor) or obs.ndim != 2 or not isinstance(action, torch.Tensor) or action.ndim != 2:
            raise ValueError("obs / action must be [N, obs_dim] / [N, act_dim] tensors")
        N, od = (int(v) for v in obs.shape)
        ad = int(action.shape[1])
        if N < 1:
            raise ValueError("no rows")
        _check_dev(obs, torch.float32, dev, "obs")
        _check_dev(action, torch.float32, dev, "action", (N, ad))
        _check_dev(next_obs, torch.float32, dev, "next_obs", (N, od))
        _check_dev(rewards, torch.float32, dev, "rewards", numel=N)
        if isinstance(dones, torch.Tensor) and dones.dtype == torch.bool:
            dones = dones.view(torch.uint8)
        _check_dev(dones, torch.uint8, dev, "dones", numel=N)
        _check_dev(accum_dones, torch.uint8, dev, "accum_dones", (N,))
        _check_dev(area, torch.float32, dev, area_name)
        cap = int(cap)
        if cap < 0 or area.numel() < cap * row_width(od, ad):
            raise ValueError(f"{area_name} must hold {cap_name} * (2 obs_dim + act_dim + 2) = {cap} * {row_width(od, ad)} floats, got {area.numel()}")
        return N, od, ad, dones, cap

    # ---- a device-resident SAC replay buffer (hipets_ring_compact_transitions / hipets_replay_gather; hipets.DeviceReplayBuffer) ----
    def ring_compact_transitions(self, obs, action, next_obs, rewards, dones, accum_dones, ring, capacity, cursor, count_out):
        """:meth:`compact_transitions` followed by ``ReplayBuffer.add_batch`` for one rollout step (hipets_ring_compact_transitions):
        the k-th row whose ``accum_dones`` is 0 lands at row ``(cur_idx + k) % capacity`` of ``ring``, a flat f32 buffer of at least
        ``capacity * (2 obs_dim + act_dim + 2)`` elements in the staging area's five-array layout over ``capacity`` rows; ``cursor``
        int64 [2] = (cur_idx, num_stored), advanced as ``add_batch`` advances them; ``count_out`` int32 [1] = the rows kept;
        ``accum_dones |= dones``.  All tensors on the device.  N > capacity is refused by the library (ERR_INVALID_ARGUMENT)."""
        N, od, ad, dones, capacity = self._check_step_rows(obs, action, next_obs, rewards, dones, accum_dones, ring, capacity, "ring", "capacity")
        _check_dev(cursor, torch.int64, self.device, "cursor", numel=2)
        _check_dev(count_out, torch.int32, self.device, "count_out", numel=1)
        self._call("hipets_ring_compact_transitions", obs=obs, action=action, next_obs=next_obs, rewards=rewards, dones=dones,
                   accum_dones=accum_dones, n=N, obs_dim=od, act_dim=ad, ring=ring, capacity=capacity, cursor=cursor, count_out=count_out)

    def replay_gather(self, ring, capacity, obs_dim, act_dim, indices, reverse_mask: bool = False, out: Optional[torch.Tensor] = None):
        """Rows of ``ring`` (the layout of :meth:`ring_compact_transitions`) by index -> f32 [n, 2 obs_dim + act_dim + 2] on the device,
        row j = (obs[i], action[i], next_obs[i], reward[i], mask) of row i = indices[j], the batch layout :meth:`sac_update` reads
        (hipets_replay_gather, one launch); mask = done, or ``1 - done`` under ``reverse_mask``.  ``indices``: an int64 device tensor of
        n elements -- an index outside [0, capacity) then gives a row of NaN, no error --, or host integers (a numpy array, a list),
        which are range-checked here (ValueError) and uploaded."""
        dev = self.device
        capacity, od, ad = int(capacity), int(obs_dim), int(act_dim)
        W = row_width(od, ad)
        _check_dev(ring, torch.float32, dev, "ring")
        if capacity < 1 or od < 1 or ad < 1 or ring.numel() < capacity * W:
            raise ValueError(f"ring must hold capacity * (2 obs_dim + act_dim + 2) = {capacity} * {W} floats, got {ring.numel()}")
        if not isinstance(indices, torch.Tensor):
            host = np.ascontiguousarray(np.asarray(indices).reshape(-1))
            if host.size and (not np.issubdtype(host.dtype, np.integer) or host.min() < 0 or host.max() >= capacity):
                raise ValueError(f"indices must be integers in [0, {capacity})")
            indices = torch.from_numpy(host.astype(np.int64, copy=False)).to(dev)
        n = int(indices.numel())
        _check_dev(indices, torch.int64, dev, "indices", numel=n)
        if out is None:
            out = torch.empty(n, W, dtype=torch.float32, device=dev)
        else:
            _check_dev(out, torch.float32, dev, "out", (n, W))
        if n:
            self._call("hipets_replay_gather", ring=ring, capacity=capacity, obs_dim=od, act_dim=ad, indices=indices, n_rows=n,
                       reverse_mask=int(bool(reverse_mask)), out=out)
        return out

    # ---- SAC updates (hipets_sac_bind / hipets_sac_update / hipets_sac_forward_taps) -----------------------------------------
    def sac_bind(self, dims, tuning: bool, gamma: float, tau: float, target_entropy: float, target_update_interval: int, adam, ptrs):
        """Tell the engine where a SAC agent's tensors live (hipets_sac_bind): ``dims`` = (obs_dim, act_dim, hidden); ``adam`` the
        three optimizers' (beta1, beta2, eps), critic / policy / alpha; ``ptrs`` the ``_lib.SAC_N_PTRS`` device addresses in the
        header's order (0 = absent).  The tensors are updated in place by :meth:`sac_update`; the caller keeps them alive."""
        adam = np.ascontiguousarray(np.asarray(adam, dtype=np.float64).reshape(-1))
        ptrs = np.ascontiguousarray(np.asarray(ptrs, dtype=np.uint64).reshape(-1))
        if adam.size != 9:
            raise ValueError("adam must hold (beta1, beta2, eps) of three optimizers")
        self.sac_owner = self.sac_dims = None  # (a refused bind leaves no agent in the engine)
        with torch.cuda.device(self.device):
            self._query("hipets_sac_bind", obs_dim=int(dims[0]), act_dim=int(dims[1]), hidden=int(dims[2]), tuning=int(bool(tuning)),
                        gamma=float(gamma), tau=float(tau), target_entropy=float(target_entropy), target_update_interval=int(target_update_interval),
                        adam=adam.ctypes.data_as(C.POINTER(C.c_double)), ptrs=ptrs, n_ptrs=int(ptrs.size))
        self.sac_dims = tuple(int(v) for v in dims)

    def sac_update(self, batch: torch.Tensor, eps_next: torch.Tensor, eps_cur: torch.Tensor, update_index: int, steps, lrs, result: torch.Tensor):
        """One SAC update on the bound agent (hipets_sac_update), asynchronous on the current stream.  ``batch`` f32 [B, 2 obs + act + 2]
        (state, action, next_state, reward, mask), ``eps_next`` / ``eps_cur`` f32 [B, act], ``steps`` / ``lrs`` = the Adam steps taken
        before and the learning rates of (critic, policy, alpha), ``result`` f32 [8] -- all device tensors but the scalars."""
        obs, act, _ = self._slot_dims("sac", "sac_bind")
        if not isinstance(batch, torch.Tensor) or batch.ndim != 2:
            raise ValueError("batch must be a [B, 2 obs + act + 2] tensor")
        B = int(batch.shape[0])
        _check_dev(batch, torch.float32, self.device, "batch", (B, row_width(obs, act)))
        _check_dev(eps_next, torch.float32, self.device, "eps_next", (B, act))
        _check_dev(eps_cur, torch.float32, self.device, "eps_cur", (B, act))
        _check_dev(result, torch.float32, self.device, "result", numel=8)
        self._call("hipets_sac_update", batch=batch, batch_size=B, eps_next=eps_next, eps_cur=eps_cur, update_index=int(update_index),
                   step_critic=int(steps[0]), step_policy=int(steps[1]), step_alpha=int(steps[2]), lr_critic=float(lrs[0]),
                   lr_policy=float(lrs[1]), lr_alpha=float(lrs[2]), result=result)
        # the update kernels write the agent's parameters through raw pointers (no tensor's _version moves): snapshots of the actor or
        # the critic compare this counter (hipets.sac)
        self.sac_updates += 1

    def sac_forward_taps(self, batch_size: int) -> Dict[str, torch.Tensor]:
        """Intermediates of the last :meth:`sac_update` (of ``batch_size`` rows): q1, q2, y, log_pi_next, log_pi, f32 [B] each."""
        names = ("q1", "q2", "y", "log_pi_next", "log_pi")
        out = {n: torch.empty(int(batch_size), dtype=torch.float32, device=self.device) for n in names}
        self._call("hipets_sac_forward_taps", batch_size=int(batch_size), **out)
        return out

    # ---- value-bootstrapped planning (hipets_critic_* / hipets_discounted_returns) ----------------------------------------------
    def critic_set(self, critic, obs_dim: int, act_dim: int):
        """Snapshot a ``QNetwork``-shaped module's live weights into the engine (hipets_critic_set; ``_pack.pack_critic`` reads the
        module or raises UnsupportedModelError).  Device to device where the critic is on this GPU.  Asynchronous.  Returns
        (obs_dim, act_dim, hidden)."""
        (K, hidden), tensors = pack_critic(critic)
        check_critic_split(K, int(obs_dim), int(act_dim))
        on_dev = [t.to(device=self.device, dtype=torch.float32).contiguous() for t in tensors]
        table = np.array([t.data_ptr() for t in on_dev], dtype=np.uint64)
        self.critic_dims = self.critic_owner = None  # (a refused set leaves no critic in the engine; a SACCritic that sets one claims the slot)
        self._call("hipets_critic_set", obs_dim=int(obs_dim), act_dim=int(act_dim), hidden=hidden, ptrs=table, n_ptrs=int(table.size))
        del on_dev  # (the copies are enqueued: torch's allocator frees in stream order)
        self.critic_dims = (int(obs_dim), int(act_dim), hidden)
        return self.critic_dims

    def critic_q(self, obs: torch.Tensor, actions: torch.Tensor, *, q1: bool = True, q2: bool = True, qmin: bool = True):
        """The critic's forward for ``obs`` f32 [B, obs_dim] and ``actions`` f32 [B, act_dim] on the device -> (q1, q2, qmin), f32 [B]
        each (hipets_critic_q, one launch; an output not wanted is None).  qmin = torch.min(q1, q2)."""
        obs_dim, act_dim, _ = self._slot_dims("critic", "critic_set")
        dev = self.device
        if not isinstance(obs, torch.Tensor) or obs.ndim != 2 or int(obs.shape[0]) < 1:
            raise ValueError("obs must be a [B, obs_dim] tensor with B >= 1")
        B = int(obs.shape[0])
        _check_dev(obs, torch.float32, dev, "obs", (B, obs_dim))
        _check_dev(actions, torch.float32, dev, "actions", (B, act_dim))
        out = [torch.empty(B, dtype=torch.float32, device=dev) if want else None for want in (q1, q2, qmin)]
        self._call("hipets_critic_q", obs=obs, actions=actions, batch=B, q1=out[0], q2=out[1], qmin=out[2])
        return tuple(out)

    def critic_geometry(self, batch: int):
        """(row tiles per workgroup -- a workgroup owns 16 of them rows --, dynamic LDS bytes) of a :meth:`critic_q` of ``batch`` rows."""
        self._slot_dims("critic", "critic_set")
        return self._geometry("hipets_critic_geometry", batch)

    def discounted_returns(self, rewards: torch.Tensor, dones: torch.Tensor, pop: int, num_particles: int, *, gamma: float = 1.0,
                           terminal_values: Optional[torch.Tensor] = None, row_totals: bool = False, first_done: bool = False):
        """:meth:`trajectory_returns` with a discount and an optional bootstrap (hipets_discounted_returns): per row
        ``sum_t gamma^t r_t`` up to and including the first terminating step, plus ``gamma^H terminal_values[row]`` (f32 [B]) for a
        row that never terminated; then the engine's particle reduction.  Arguments and results as there."""
        dev = self.device
        if not isinstance(rewards, torch.Tensor) or rewards.ndim != 2:
            raise ValueError("rewards must be a [H, B] tensor")
        H, B = (int(v) for v in rewards.shape)
        if pop < 1 or num_particles < 1 or pop * num_particles != B:
            raise ValueError(f"rewards holds {B} rows per step, pop x num_particles = {pop} x {num_particles}")
        gamma = check_discount(gamma)
        _check_dev(rewards, torch.float32, dev, "rewards")
        if isinstance(dones, torch.Tensor) and dones.dtype == torch.bool:
            dones = dones.view(torch.uint8)  # (one byte per element, 0 / 1)
        _check_dev(dones, torch.uint8, dev, "dones", (H, B))
        if terminal_values is not None:
            _check_dev(terminal_values, torch.float32, dev, "terminal_values", numel=B)
        out = torch.empty(pop, dtype=torch.float32, device=dev)
        tot = torch.empty(B, dtype=torch.float32, device=dev) if row_totals else None
        first = torch.empty(B, dtype=torch.int32, device=dev) if first_done else None
        self._call("hipets_discounted_returns", rewards=rewards, dones=dones, terminal_values=terminal_values, gamma=gamma, pop=int(pop), horizon=H,
                   num_particles=int(num_particles), returns=out, row_totals=tot, first_done=first)
        return (out, tot, first) if (row_totals or first_done) else out

    # ---- ensemble predictions and uncertainty (hipets_ensemble_* / hipets_uncertainty_penalty) ------------------------------------
    def ensemble_set(self, spec: ModelSpec):
        """Snapshot ``spec`` -- every member, the normaliser, the bounds, the elite list -- into the engine's ensemble slot
        (hipets_ensemble_set), apart from the rollout model of :meth:`set_model`.  A shape the kernel does not cover raises
        UnsupportedModelError before anything is called; a refused set leaves the slot empty."""
        spec.validate()
        check_ensemble_shape(spec)
        ws = [w.detach().to(device=self.device, dtype=torch.float32).contiguous() for w in spec.weights]
        bs = [b.detach().to(device=self.device, dtype=torch.float32).contiguous() for b in spec.biases]
        d, cols, keep = pack_model_desc(spec, ws, bs)
        self.ensemble_spec = self.ensemble_owner = None
        self._call("hipets_ensemble_set", desc=d, cols=cols, n_cols=0 if cols is None else len(cols))
        del keep
        self.ensemble_spec = spec

    def _ensemble_spec(self) -> ModelSpec:
        if self.ensemble_spec is None:
            raise HipetsError("Engine.ensemble_set() has not been called")
        return self.ensemble_spec

    def ensemble_predict(self, obs: Optional[torch.Tensor] = None, actions: Optional[torch.Tensor] = None, *,
                         model_in: Optional[torch.Tensor] = None, only_elite: bool = False, mean: bool = True, logvar: bool = True,
                         stats: bool = False):
        """Every requested member's forward of the same rows in one launch (hipets_ensemble_predict): from ``obs`` f32 [B, obs_dim] and
        ``actions`` f32 [B, act_dim], or from a ready ``model_in`` f32 [B, in_dim].  Returns (mean [n, B, out_dim], logvar [n, B,
        out_dim], stats [B, 4]) on the device, None for an output not wanted; n = all members, or with ``only_elite`` the spec's
        member list.  The columns of ``stats``: ``_lib.ENSEMBLE_STATS``."""
        spec, dev = self._ensemble_spec(), self.device
        raw = obs is not None or actions is not None
        if raw == (model_in is not None) or (raw and (obs is None or actions is None)):
            raise ValueError("give either obs and actions, or model_in")
        first = model_in if model_in is not None else obs
        if not isinstance(first, torch.Tensor) or first.ndim != 2 or int(first.shape[0]) < 1:
            raise ValueError("the input must be a [B, width] tensor with B >= 1")
        B = int(first.shape[0])
        if model_in is not None:
            _check_dev(model_in, torch.float32, dev, "model_in", (B, spec.in_dim))
        else:
            _check_dev(obs, torch.float32, dev, "obs", (B, spec.obs_dim))
            _check_dev(actions, torch.float32, dev, "actions", (B, spec.act_dim))
        if logvar and spec.deterministic:
            raise ValueError("a deterministic model has no log-variance head")
        n = len(spec.members) if only_elite else spec.ensemble_size
        out = [torch.empty(shape, dtype=torch.float32, device=dev) if want else None
               for want, shape in ((mean, (n, B, spec.out_dim)), (logvar, (n, B, spec.out_dim)), (stats, (B, 4)))]
        self._call("hipets_ensemble_predict", obs=obs, actions=actions, model_in=model_in, batch=B, only_elite=int(bool(only_elite)),
                   mean=out[0], logvar=out[1], stats=out[2])
        return tuple(out)

    def ensemble_geometry(self, batch: int):
        """(row tiles per workgroup -- a workgroup owns 16 of them rows --, dynamic LDS bytes) of an :meth:`ensemble_predict` of ``batch`` rows."""
        self._ensemble_spec()
        return self._geometry("hipets_ensemble_geometry", batch)

    def uncertainty_penalty(self, stats: torch.Tensor, stat: int, coef: float, rewards: torch.Tensor, dones: Optional[torch.Tensor] = None, *,
                            halt_threshold: Optional[float] = None, halt_reward: Optional[float] = None):
        """``rewards`` f32 [B] -= coef * stats[:, stat], in place; with ``halt_threshold`` the rows above it get ``dones`` (uint8 or bool
        [B], in place) = 1 and, with ``halt_reward``, that reward (hipets_uncertainty_penalty; one launch, bit for bit
        tests/ensemble_restatement.penalty_np)."""
        dev = self.device
        B = int(rewards.numel())
        _check_dev(stats, torch.float32, dev, "stats", (B, 4))
        _check_dev(rewards, torch.float32, dev, "rewards", numel=B)
        if dones is not None:
            if dones.dtype == torch.bool:
                dones = dones.view(torch.uint8)  # (one byte per element, 0 / 1)
            _check_dev(dones, torch.uint8, dev, "dones", numel=B)
        elif halt_threshold is not None:
            raise ValueError("a halt threshold needs dones")
        self._call("hipets_uncertainty_penalty", stats=stats, stat=int(stat), coef=float(coef),
                   halt_threshold=float("nan") if halt_threshold is None else float(halt_threshold),
                   halt_reward=0.0 if halt_reward is None else float(halt_reward), use_halt_reward=int(halt_reward is not None), batch=B,
                   rewards=rewards, dones=dones)

    # ---- policy rollouts: the actor rolled through the ensemble (hipets_policy_rollout) ---------------------------------------------
    def policy_rollout(self, s0: torch.Tensor, horizon: int, *, mean_rows: int = 0, only_elite: bool = True, seed: int = 0, stream_id: int = 0,
                       eps: Optional[torch.Tensor] = None, states: bool = False):
        """The snapshot actor (:meth:`policy_set`) rolled ``horizon`` steps through the snapshot ensemble's expected next observation
        (:meth:`ensemble_set`) from ``s0`` f32 [n, obs_dim] on the device, one launch (hipets_policy_rollout).  Rows below ``mean_rows``
        take the mean action, the others sample with ``eps`` f32 [horizon, n, act_dim] (None: drawn in-kernel from (seed, stream_id);
        ``policy_normals(horizon * n, act_dim, seed, stream_id)`` is that table).  Returns actions f32 [n, horizon, act_dim], and with
        ``states`` also the visited states f32 [horizon + 1, n, obs_dim]."""
        obs_dim, _, act_dim = self._slot_dims("policy", "policy_set")
        self._ensemble_spec()
        dev, H = self.device, int(horizon)
        if not isinstance(s0, torch.Tensor) or s0.ndim != 2 or int(s0.shape[0]) < 1:
            raise ValueError("s0 must be a [n, obs_dim] tensor with n >= 1")
        n = int(s0.shape[0])
        _check_dev(s0, torch.float32, dev, "s0", (n, obs_dim))
        if H < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        if eps is not None:
            _check_dev(eps, torch.float32, dev, "eps", (H, n, act_dim))
        actions = torch.empty(n, H, act_dim, dtype=torch.float32, device=dev)
        visited = torch.empty(H + 1, n, obs_dim, dtype=torch.float32, device=dev) if states else None
        self._call("hipets_policy_rollout", s0=s0, n=n, horizon=H, mean_rows=int(mean_rows), only_elite=int(bool(only_elite)), seed=int(seed),
                   stream_id=int(stream_id), eps=eps, actions=actions, states=visited)
        return (actions, visited) if states else actions

    def policy_rollout_geometry(self, n: int):
        """(row tiles per workgroup -- a workgroup owns 16 of them rows --, dynamic LDS bytes) of a :meth:`policy_rollout` of ``n`` rows."""
        r, lds = C.c_int32(), C.c_int32()
        self._query("hipets_policy_rollout_geometry", n=int(n), row_tiles=C.byref(r), lds_bytes=C.byref(lds))
        return r.value, lds.value

    def timing_enable(self, on=True):
        """True / 1: time every rollout-kernel launch; k > 1: every k-th launch; False / 0: off."""
        self._query("hipets_timing_enable", on=int(on))

    def timing_read(self, reset: bool = True):
        n, ms = C.c_int64(), C.c_double()
        self._query("hipets_timing_read", launches=C.byref(n), total_ms=C.byref(ms), reset=int(reset))
        return n.value, ms.value


_ENGINES: Dict[int, Engine] = {}


def get_engine(device) -> Engine:
    """One Engine per GPU (the reference is single-device, single-threaded)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise HipetsError(f"hipets needs a GPU device, got {device} (there is no CPU fallback)")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _ENGINES:
        _ENGINES[idx] = Engine(torch.device("cuda", idx))
    return _ENGINES[idx]
