"""The planning objectives: ``make_eval_fn`` / ``HipTrajectoryEvalFn`` <- the closure at mbrl/planning/trajectory_opt.py:743-748
around ``ModelEnv.evaluate_action_sequences`` (mbrl/models/model_env.py:145-191), the model-as-environment ``ModelEnv``
(model_env.py:15-191), the unfused and the PlaNet objectives, all on libhipets' fused kernels.

There is no CPU fallback anywhere in this module: every objective needs a gfx950 device.
"""
from __future__ import annotations

import weakref
from typing import Dict, Optional

import numpy as np
import torch

from . import reference_draws as rd
from .engine import Engine, get_engine
from .model import (BoxTermination, ModelSpec, PlaNetSpec, UnsupportedModelError, is_planet_model, model_version, planet_version,
                    spec_from_model_env, spec_from_planet_model)
from .reduce import ParticleReduce


def _has_device_mode(spec: ModelSpec) -> bool:
    """Does the library's DEVICE mode (in-kernel balanced member shuffle) exist for ``spec``?  For GaussianMLP ensembles and for any
    model under expectation propagation; BasicEnsemble models draw iid members, which the library's DEVICE mode has no variant for."""
    return spec.ensemble_kind != "basic_ensemble" or spec.propagation == "expectation"


def _device_f32(t: torch.Tensor, device) -> torch.Tensor:
    """``t`` as a contiguous float32 tensor on ``device`` (itself when it already is one)."""
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    return t


# ---------------------------------------------------------------------------------------------
# objective: ModelEnv.evaluate_action_sequences on the fused kernel
# ---------------------------------------------------------------------------------------------
class _Objective:
    """What every objective shares: the spec, device and version token of a live model or of a spec (``_spec_type``) handed in
    as it is, re-packing when the live model changed, binding the spec to the engine shared per GPU, and the seed and call
    counter of its counter-based streams, and its reduction over the particles (``particle_reduce``: a :class:`ParticleReduce` or
    'mean' / 'min' / 'max').  A kind of objective supplies three hooks: ``_read_spec(live)``, ``_read_version(live)`` and
    ``_set_engine_model(only_if_other)``."""

    def __init__(self, model, num_particles: int, engine: Optional[Engine], seed: int, device, particle_reduce=None):
        self.particle_reduce = ParticleReduce.coerce(particle_reduce)  # (a bad one raises before anything touches the engine)
        self.num_particles, self.seed, self.calls = int(num_particles), int(seed), 0
        self._live, self._version = None, None
        if isinstance(model, self._spec_type):
            self.spec = model
            dev = device if device is not None else "cuda:0"
        else:
            self._live = model
            self.spec = self._read_spec(model)
            dev = device if device is not None else getattr(model, "device", "cuda:0")
            self._version = self._read_version(model)
        self.engine = engine if engine is not None else get_engine(dev)
        self.device = self.engine.device
        self._set_engine_model()

    def refresh(self, force: bool = False):
        """Re-pack weights if the live model changed (mbrl/models/model_trainer.py:288-296)."""
        if self._live is None:
            return
        v = self._read_version(self._live)
        if force or v != self._version:
            self.spec = self._read_spec(self._live)
            self._set_engine_model()
            self._version = v

    def bind_model(self):
        """Re-pack changed weights and make them the engine's model, and this objective's reduction over the particles the engine's
        (engines are shared per GPU: a default objective that follows a risk-aware one sets the mean back)."""
        self.refresh()
        self._set_engine_model(only_if_other=True)
        reduce = self.particle_reduce.resolve(self.num_particles)
        if getattr(self.engine, "reduce", ParticleReduce()) != reduce:  # (an engine that mirrors none is at the library's initial mean)
            self.engine.set_particle_reduce(reduce)


class _EnsembleObjective(_Objective):
    """The two ensemble objectives: built from a live ``mbrl.models.ModelEnv`` or a ``ModelSpec``; the reference's batch-size
    check."""

    _spec_type = ModelSpec
    _allow_custom_fns = False  # keep unrecognised reward / termination callables in the spec (the unfused objective)
    _read_version = staticmethod(model_version)

    def _read_spec(self, model_env) -> ModelSpec:
        return spec_from_model_env(model_env, allow_custom_fns=self._allow_custom_fns)

    def _set_engine_model(self, only_if_other: bool = False):
        if not (only_if_other and self.engine.spec is self.spec):
            self.engine.set_model(self.spec)

    def check_batch(self, pop: int):
        """The reference's ValueError (gaussian_mlp.py:195-200), raised for every propagation method and kept in
        FAST mode too so that switching engines never changes which configurations are accepted."""
        B, M = pop * self.num_particles, len(self.spec.members)
        if self.spec.ensemble_kind == "basic_ensemble":  # BasicEnsemble.forward has no such rule (basic_ensemble.py:142-196)
            return
        if B % M != 0:
            raise ValueError(
                f"GaussianMLP ensemble requires batch size to be a multiple of the "
                f"number of models. Current batch size is {B} for "
                f"{M} models."
            )


def closed_form_dones(spec: ModelSpec, states: torch.Tensor) -> torch.Tensor:
    """The spec's closed-form termination over ``states`` [N, obs] -> bool [N]: the torch restatement of the kernels' ``term_eval``
    (csrc/closed_forms.hpp; mbrl/env/termination_fns.py).  Comparisons of the same float32 values against the same float32
    constants, so the flags are the kernel's own."""
    s, term = states, spec.termination
    finite = lambda: torch.isfinite(s).all(dim=1)  # noqa: E731
    if isinstance(term, BoxTermination):
        ok = finite() if term.require_finite else torch.ones(s.shape[0], dtype=torch.bool, device=s.device)
        for iv in term.intervals:
            x = s[:, iv.dim]
            ok = ok & ((x > iv.lo) if iv.lo_open else (x >= iv.lo)) & ((x < iv.hi) if iv.hi_open else (x <= iv.hi))
        return ~ok
    if term == "cartpole":
        thr = 12.0 * 2.0 * 3.14159265358979323846 / 360.0
        return ~((s[:, 0] > -2.4) & (s[:, 0] < 2.4) & (s[:, 2] > -thr) & (s[:, 2] < thr))
    if term == "inverted_pendulum":
        return ~(finite() & (s[:, 1].abs() <= 0.2))
    if term == "hopper":
        return ~(finite() & (s[:, 1:].abs() < 100.0).all(dim=1) & (s[:, 0] > 0.7) & (s[:, 1].abs() < 0.2))
    if term == "walker2d":
        return ~((s[:, 0] > 0.8) & (s[:, 0] < 2.0) & (s[:, 1] > -1.0) & (s[:, 1] < 1.0))
    if term == "ant":
        return ~(finite() & (s[:, 0] >= 0.2) & (s[:, 0] <= 1.0))
    if term == "humanoid":
        return (s[:, 0] < 1.0) | (s[:, 0] > 2.0)
    if term == "no_termination":
        return torch.zeros(s.shape[0], dtype=torch.bool, device=s.device)
    raise UnsupportedModelError(f"no restatement of termination {term!r}")


class _RolloutObjective(_EnsembleObjective):
    """What the objectives that run a whole horizon per ``hipets_rollout`` call share: the randomness modes and their draws
    (``_rollout``), and the predicted trajectory of one call read off the rollout kernel's taps (``_traced_rollout``, ``_trajectory``)."""

    max_trajectory_bytes = 2 << 30

    def __init__(self, model, num_particles: int, engine: Optional[Engine] = None, mode: str = "device",
                 seed: int = 0, device=None, rng: Optional[torch.Generator] = None, particle_reduce=None):
        if mode not in ("fast", "device", "exact", "exact_device"):
            raise ValueError("mode must be 'fast', 'device', 'exact' or 'exact_device'")
        self.mode = mode
        self.rollout_kw = {}  # extra Engine.rollout arguments of every call (tests pin rows_per_group / generic_kernel)
        self._taps = None
        super().__init__(model, num_particles, engine, seed, device, particle_reduce)
        if rng is None and self._live is not None:
            rng = getattr(model, "_rng", None)
        self._rng = rng

    def _prep(self, action_sequences: torch.Tensor) -> torch.Tensor:
        self.bind_model()
        a = _device_f32(action_sequences, self.device)
        self.check_batch(a.shape[0])
        return a

    @property
    def _rollout_mode(self) -> Optional[str]:
        """'fast' / 'device' when the rollouts draw their randomness in-kernel from (seed, stream_id), else None."""
        if self.mode == "fast":
            return "fast"
        if self.mode in ("device", "exact_device") and _has_device_mode(self.spec):
            return "device"
        return None

    def _rollout(self, a: torch.Tensor, initial_state: np.ndarray, **kw) -> torch.Tensor:
        """One ``Engine.rollout`` of this call's stream (``self.calls``) in the objective's mode; ``kw``: the taps."""
        kw = {**self.rollout_kw, **kw}
        if self._rollout_mode is not None:
            return self.engine.rollout(a, initial_state, self.num_particles, mode=self._rollout_mode, seed=self.seed, stream_id=self.calls, **kw)
        pop, H, _ = a.shape
        B = pop * self.num_particles
        if self.mode in ("device", "exact_device"):  # BasicEnsemble models only: torch's device generator, not reference order
            members, eps = rd.device_generator_draws(self.spec, B, H, self._device_rng())
            return self.engine.rollout(a, initial_state, self.num_particles, mode="exact", members=members, eps=eps, **kw)
        perms, members, eps = rd.rollout_draws(self.spec, B, H, self._cpu_rng())
        if perms is not None:
            perms = perms.to(self.device)
        if eps is not None:
            eps = eps.to(self.device)
        return self.engine.rollout(a, initial_state, self.num_particles, mode="exact", perms=perms, members=members, eps=eps, **kw)

    def _device_rng(self):
        if not hasattr(self, "_dev_rng"):
            self._dev_rng = torch.Generator(device=self.device).manual_seed(self.seed)
        return self._dev_rng

    def _cpu_rng(self):
        if self._rng is not None and self._rng.device.type == "cpu":
            return self._rng
        if not hasattr(self, "_own_rng"):
            self._own_rng = torch.Generator().manual_seed(self.seed)
        return self._own_rng

    # ---- the predicted trajectory of one call ----
    def _traced_rollout(self, a: torch.Tensor, initial_state: np.ndarray):
        """This call's rollout with both taps set: (next_obs [H, B, obs], rewards [H, B]) -- every row's predicted states and the
        kernel's own reward (learned or closed form) before termination masking --, in buffers the objective owns and reuses
        across calls of the same (H, B)."""
        pop, H, _ = a.shape
        B, obs = pop * self.num_particles, self.spec.obs_dim
        nbytes = H * B * (obs + 1) * 4
        if nbytes > self.max_trajectory_bytes:
            raise ValueError(f"the trajectory of this call -- horizon {H} x {B} rows x ({obs} + 1) floats = {nbytes} bytes -- exceeds "
                             f"max_trajectory_bytes = {self.max_trajectory_bytes}")
        if self._taps is None or tuple(self._taps[0].shape) != (H, B, obs) or self._taps[0].device != self.device:
            self._taps = (torch.empty(H, B, obs, dtype=torch.float32, device=self.device),
                          torch.empty(H, B, dtype=torch.float32, device=self.device))
        next_obs, rewards = self._taps
        self._rollout(a, initial_state, trace_next_obs=next_obs, trace_rewards=rewards)
        return next_obs, rewards

    def _trajectory(self, initial_state: np.ndarray, action_sequences: torch.Tensor, details: bool):
        """One evaluation through the taps (the hook of a kind of objective: rewards / dones of the traced states)."""
        raise NotImplementedError

    def trajectories(self, initial_state: np.ndarray, action_sequences: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The predicted trajectories of ONE evaluation (the model side of ``mbrl.util.common.rollout_model_env``): ``next_obs``
        [H, B, obs], ``rewards`` [H, B] (before termination masking), ``dones`` bool [H, B], ``first_done`` int32 [B] (the first
        terminating step, H if none), ``row_totals`` [B], ``returns`` [pop] (the objective's reduction of ``row_totals`` over the
        particles); B = pop * num_particles, row c * P + p.  Counts as
        a call (it consumes the next stream, and returns what ``__call__`` would have); the views are valid until the next call."""
        return self._trajectory(initial_state, action_sequences, True)


class HipTrajectoryEvalFn(_RolloutObjective):
    """``trajectory_eval_fn(initial_state, action_sequences) -> Tensor[B]`` (mbrl/types.py:15).

    Built from a live ``mbrl.models.ModelEnv`` (weights are re-snapshotted whenever
    ``ModelTrainer.train`` changed them) or from a ``ModelSpec``.  Randomness modes:

    * ``'device'`` (THE DEFAULT since round 6): the reference's propagation semantics -- ONE balanced random permutation of all
      ``pop * particles`` rows per step (gaussian_mlp.py:203-205), iid eps per row and dim -- with both drawn
      in-kernel from ``(seed, call counter)`` (a keyed bijection + Philox).  ONE persistent launch for the horizon (rows
      change workgroups through an in-kernel hand-over table); one launch per step where that form does not apply
      (``Engine.set_persistent(False)``, batches beyond two workgroups per CU) -- same bits either way.
    * ``'fast'`` (opt-in; ~8 % faster at cfg2): one launch for the whole horizon; each workgroup (particle p of 16-48 consecutive
      candidates) draws one member per step from a balanced schedule: same marginals, block-wise common random numbers --
      NOT the reference's per-row shuffle (held to the statistical tests only; with fewer than 16-48 candidates several particles
      of one candidate share a member at every step, include/hipets.h hipets_fast_schedule).
    * ``'exact'``: replays the reference's own draws from torch's RNGs in the reference's order (one
      ``randperm(B)`` per step from the global generator, one ``normal_`` per step from ``rng``): seed-identical
      to ``ModelEnv.evaluate_action_sequences`` (a parity aid: it synchronises with the host).
    * ``'exact_device'``: alias of ``'device'`` (kept for round-1 callers; BasicEnsemble models draw their iid
      member maps with torch's device generator).

    ``particle_reduce``: how a candidate's ``num_particles`` totals become its value -- the mean (default, model_env.py:190-191), or
    a :class:`ParticleReduce` (worst case, mean - kappa * std, the mean of the worst k / CVaR, best case) for planning under the
    model's own uncertainty; the fused plans reduce the same way, inside their launches.
    """

    @property
    def kernel_mode(self) -> Optional[str]:
        """'fast' / 'device' when the objective draws its randomness in-kernel from (seed, stream_id) -- the modes the
        fused plans can run --, else None."""
        return self._rollout_mode

    def evaluate_seeded(self, initial_state: np.ndarray, action_sequences: torch.Tensor, seed: int, stream_id: int) -> torch.Tensor:
        """One objective evaluation with explicit counter-based randomness: what iteration ``stream_id`` of a fused plan
        runs, callable from the per-iteration optimizer paths so that both produce the same numbers bit for bit."""
        a = self._prep(action_sequences)
        return self.engine.rollout(a, initial_state, self.num_particles, mode=self.kernel_mode, seed=seed, stream_id=stream_id)

    def __call__(self, initial_state: np.ndarray, action_sequences: torch.Tensor) -> torch.Tensor:
        a = self._prep(action_sequences)
        self.calls += 1
        return self._rollout(a, initial_state)

    def _trajectory(self, initial_state, action_sequences, details):
        """The kernel's own rewards off the tap, the spec's closed-form termination restated over the traced states, reduced by
        hipets_trajectory_returns: ``returns`` are the bits of the untapped call of the same stream."""
        a = self._prep(action_sequences)
        self.calls += 1
        pop, H, _ = a.shape
        next_obs, rewards = self._traced_rollout(a, initial_state)
        dones = closed_form_dones(self.spec, next_obs.view(-1, self.spec.obs_dim)).view(H, -1)
        returns, row_totals, first_done = self.engine.trajectory_returns(rewards, dones, pop, self.num_particles, row_totals=True, first_done=True)
        return {"next_obs": next_obs, "rewards": rewards, "dones": dones, "first_done": first_done, "row_totals": row_totals, "returns": returns}


class ModelEnv:
    """The model-as-environment interface of mbrl/models/model_env.py:15-191 on the fused kernels:
    ``reset`` / ``step`` (one transition for a batch of independent rows: what MBPO-style model rollouts and the
    visualisers call) and ``evaluate_action_sequences``.  Built from a ``ModelSpec`` or a live mbrl ``ModelEnv``.

    TS-infinity (``fixed_model``) member maps travel in the model state, as the reference's ``propagation_indices`` do
    (gaussian_mlp.py:207-212, basic_ensemble.py:182-187): a step is a function of its state and the env's model and seed.
    Every ``reset`` draws a fresh map and returns it as ``propagation_indices`` -- a [B] permutation of the rows for GaussianMLP
    models in 'device' / 'exact' mode, [B] int64 member slots for BasicEnsemble models and for every model in 'fast' mode
    (``schedule[row // (16 r)]``) -- and, in the in-kernel modes, the stream that keys it, under ``MAP_STREAM_KEY`` (an int64
    scalar tensor).  A step whose state still holds the very tensor that reset returned re-derives that map in-kernel from
    (seed, stream); any other ``propagation_indices`` tensor is used as given (the EXACT kernel, eps still drawn from the step's own
    stream); a ``fixed_model`` state without one raises the reference's ValueError."""

    MAP_STREAM_KEY = "hipets_map_stream"

    def __init__(self, model, engine: Optional[Engine] = None, mode: str = "device", seed: int = 0, device=None,
                 generator: Optional[torch.Generator] = None, uncertainty=None):
        """``mode`` as for :class:`HipTrajectoryEvalFn`: 'device' (default; the reference's per-row balanced member shuffle and iid
        eps, drawn in-kernel), 'fast' (one member per workgroup of 16-48 consecutive rows), 'exact' (the reference's own torch draws).
        ``uncertainty``: a :class:`hipets.UncertaintyPenalty` -- every ``step`` then runs, after its model step, one statistics launch
        of the ensemble kernel on the step's (obs, action) and one penalty launch on its rewards and dones (``hipets.ensemble``); a
        model that kernel does not cover raises UnsupportedModelError here.  None: nothing is added."""
        self._eval = HipTrajectoryEvalFn(model, 1, engine=engine, mode=mode, seed=seed, device=device, rng=generator)
        self.engine, self.device, self.mode, self.seed = self._eval.engine, self._eval.device, mode, int(seed)
        self.uncertainty, self._predictor = uncertainty, None
        if uncertainty is not None:
            from .ensemble import EnsemblePredictor, UncertaintyPenalty

            if not isinstance(uncertainty, UncertaintyPenalty):
                raise TypeError("uncertainty must be a hipets.UncertaintyPenalty")
            self._predictor = EnsemblePredictor(self, engine=self.engine)
        self._return_as_np = True
        self._steps = 0
        self._resets = 0
        self._exported = weakref.WeakValueDictionary()  # reset stream -> the propagation_indices tensor that reset returned

    def _step_mode(self) -> str:
        """Kernel mode of ``step`` for the in-kernel randomness modes: 'device' where the library has it (GaussianMLP ensembles; any
        model under expectation propagation), else 'fast' (BasicEnsemble: iid member draws per workgroup)."""
        return self._eval.kernel_mode or "fast"

    @property
    def spec(self) -> ModelSpec:
        return self._eval.spec

    def reset(self, initial_obs_batch: np.ndarray, return_as_np: bool = True) -> Dict[str, torch.Tensor]:
        """model_env.py:62-85: returns the model state {"obs", "propagation_indices"} (+ ``MAP_STREAM_KEY``, see the class)."""
        assert len(initial_obs_batch.shape) == 2  # batch, obs_dim
        self._eval.bind_model()  # the maps below are exported for THIS model
        obs = torch.as_tensor(np.asarray(initial_obs_batch, dtype=np.float32)).to(self.device).contiguous()
        self._return_as_np = return_as_np
        B = obs.shape[0]
        self._eval.num_particles = 1
        self._eval.check_batch(B)
        state = {"obs": obs, "propagation_indices": None}
        if self.spec.propagation != "fixed_model":
            return state
        # model.py:404-407 -> gaussian_mlp.py:363-375 / basic_ensemble.py:255-260: one fresh map per reset
        if self.mode == "exact":
            idx = rd.reset_draws(self.spec, B, self._eval._cpu_rng())  # (BasicEnsemble member slots stay on the host)
            state["propagation_indices"] = idx if self.spec.ensemble_kind == "basic_ensemble" else idx.to(self.device)
            return state
        self._resets += 1
        stream = self._resets  # (0 would mean "none" to hipets_rollout_opts.perm_stream_id)
        if self._step_mode() == "device":
            # the TS-infinity permutation of (seed, stream), evaluated in-kernel at every step (hipets_rollout_opts.perm_stream_id)
            idx = self.engine.device_perms(1, B, self.seed, stream)
        else:
            idx = self._fast_map(B, stream)[1]
        self._exported[stream] = idx
        state["propagation_indices"] = idx
        state[self.MAP_STREAM_KEY] = torch.tensor(stream, dtype=torch.int64)
        return state

    def _fast_map(self, B: int, stream: int):
        """(member schedule, per-row member slots) of the FAST-mode TS-infinity map of (seed, stream): hipets_step runs the general
        kernel layout, workgroup w owns rows [16 r w, 16 r (w + 1))."""
        nwg, r = self.engine.fast_geometry(B, 1, 1, -1)
        sched = self.engine.fast_schedule(1, nwg, self.seed, stream).contiguous()
        return sched, sched[0].long()[torch.arange(B, device=self.device) // (16 * r)]

    def _explicit_map(self, indices, B: int):
        """A caller's ``propagation_indices``, checked on the host before a kernel reads them as row / member indices: member slots in
        [0, M) for BasicEnsemble models and in 'fast' mode, else a permutation of [0, B).  Returns (perm, members) for Engine.step."""
        m = torch.as_tensor(indices).detach().to("cpu", torch.int64).reshape(-1)
        if m.numel() != B:
            raise ValueError(f"propagation_indices holds {m.numel()} entries for a batch of {B} rows")
        if self.spec.ensemble_kind == "basic_ensemble" or self.mode == "fast":
            M = len(self.spec.members)
            if int(m.min()) < 0 or int(m.max()) >= M:
                raise ValueError(f"propagation_indices must hold member slots in [0, {M})")
            return None, m
        if not torch.equal(m.sort().values, torch.arange(B)):
            raise ValueError("propagation_indices of a GaussianMLP model must be a permutation of the batch rows")
        return m.to(self.device), None

    def step(self, actions, model_state: Dict[str, torch.Tensor], sample: bool = False):
        """model_env.py:87-140: (next_observs, rewards, dones, next_model_state)."""
        return self._step(actions, model_state, sample, self._predictor, self.uncertainty)

    def _step(self, actions, model_state, sample, predictor, penalty):
        """``step`` with the uncertainty penalty as an argument (``predictor`` None: none): what a penalised view of this environment
        calls (hipets.mbpo), so that the environment's own counters and streams advance whoever steps it"""
        assert len(actions.shape) == 2  # batch, action_dim
        self._eval.bind_model()
        if isinstance(actions, np.ndarray):
            actions = torch.from_numpy(actions)
        actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        obs = model_state["obs"].to(device=self.device, dtype=torch.float32).contiguous()
        B = obs.shape[0]
        fixed = self.spec.propagation == "fixed_model"
        indices = model_state.get("propagation_indices")
        if fixed and indices is None:  # gaussian_mlp.py:207-211, basic_ensemble.py:182-186
            raise ValueError("When using propagation='fixed_model', `propagation_indices` must be provided.")
        self._steps += 1
        keyed = 0  # the stream of the reset whose own map this state carries (in-kernel modes)
        if fixed and self.mode != "exact":
            s = model_state.get(self.MAP_STREAM_KEY)
            if s is not None and self._exported.get(int(s)) is indices:
                keyed = int(s)
        draws = sample and not self.spec.deterministic
        if self.mode == "exact":
            perm, members = self._explicit_map(indices, B) if fixed else (None, None)
            drawn, eps = rd.step_draws(self.spec, B, self._eval._cpu_rng(), sample)
            if drawn is not None:  # random_model: basic_ensemble.py:122-129 (the generator) / gaussian_mlp.py:205 (global RNG)
                perm, members = (None, drawn) if self.spec.ensemble_kind == "basic_ensemble" else (drawn.to(self.device), None)
            if eps is not None:
                eps = eps.to(self.device)
            nobs, rew, done = self.engine.step(obs, actions, mode="exact", sample=sample, perm=perm, eps=eps, members=members)
        elif fixed and not keyed:
            # a map the caller supplied: exactly that map, with the eps the in-kernel modes draw for this step's stream
            perm, members = self._explicit_map(indices, B)
            eps = self.engine.fast_normals(1, B, self.seed, self._steps)[0] if draws else None
            nobs, rew, done = self.engine.step(obs, actions, mode="exact", sample=sample, perm=perm, eps=eps, members=members)
        elif self._step_mode() == "device":
            nobs, rew, done = self.engine.step(obs, actions, mode="device", sample=sample, seed=self.seed, stream_id=self._steps,
                                               perm_stream_id=keyed)
        else:
            sched = self._fast_map(B, keyed)[0] if keyed else None
            nobs, rew, done = self.engine.step(obs, actions, mode="fast", sample=sample, seed=self.seed, stream_id=self._steps,
                                               member_schedule=sched)
        if predictor is not None:  # (rew [B, 1] and done [B, 1] are this step's own tensors: penalised in place)
            predictor.penalise(penalty, obs, actions, rew.view(-1), done.view(-1))
        next_state = {**model_state, "obs": nobs}
        if self._return_as_np:
            return nobs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), next_state
        return nobs, rew, done, next_state

    def evaluate_action_sequences(self, action_sequences: torch.Tensor, initial_state: np.ndarray, num_particles: int,
                                  particle_reduce=None) -> torch.Tensor:
        """model_env.py:145-191.  ``particle_reduce`` (this call only): a :class:`ParticleReduce` or 'mean' / 'min' / 'max' in place
        of the mean over the particles."""
        assert len(action_sequences.shape) == 3
        self._eval.num_particles = int(num_particles)
        self._eval.particle_reduce = ParticleReduce.coerce(particle_reduce)
        try:
            return self._eval(initial_state, action_sequences)
        finally:
            self._eval.particle_reduce = ParticleReduce()  # (reset / step bind the model too: they leave the engine at the mean)


class UnfusedTrajectoryEvalFn(_EnsembleObjective):
    """``trajectory_eval_fn`` for models whose ``reward_fn`` / ``termination_fn`` are arbitrary Python callables
    (SURVEY.md section 2.1 row 6 "documented unfused fallback"): the horizon loop of
    ``ModelEnv.evaluate_action_sequences`` (model_env.py:178-191) runs on the host, every model transition is ONE fused
    ``hipets_step`` launch (input build, ensemble MLP, sampling, delta), and the user's callables run as torch ops on
    the returned device tensors.  ``step_mode='device'`` (default): every step draws the reference's balanced per-row member
    shuffle and iid eps in-kernel; ``'fast'``: one member per workgroup of 16-48 consecutive rows (also what BasicEnsemble
    models run: the library's DEVICE mode has no iid-member variant)."""

    mode = "unfused"
    _allow_custom_fns = True

    def __init__(self, model, num_particles: int, reward_fn=None, termination_fn=None, engine: Optional[Engine] = None,
                 seed: int = 0, device=None, step_mode: str = "device", particle_reduce=None):
        if step_mode not in ("device", "fast"):
            raise ValueError("step_mode must be 'device' or 'fast'")
        self.step_mode = step_mode
        super().__init__(model, num_particles, engine, seed, device, particle_reduce)
        self.reward_fn = reward_fn if reward_fn is not None else self.spec.custom_reward_fn
        self.termination_fn = termination_fn if termination_fn is not None else self.spec.custom_termination_fn

    def __call__(self, initial_state: np.ndarray, action_sequences: torch.Tensor) -> torch.Tensor:
        self.bind_model()
        a_seq = action_sequences.to(device=self.device, dtype=torch.float32)
        pop, H, _ = a_seq.shape
        P = self.num_particles
        self.check_batch(pop)
        self.calls += 1
        obs = torch.as_tensor(np.asarray(initial_state, np.float32), device=self.device).repeat(pop * P, 1).contiguous()
        total = torch.zeros(pop * P, 1, device=self.device)
        terminated = torch.zeros(pop * P, 1, dtype=torch.bool, device=self.device)
        schedule = None
        device_mode = self.step_mode == "device" and _has_device_mode(self.spec)
        fixed = self.spec.propagation == "fixed_model"  # TS-infinity: one member map for the whole horizon (model.py:404-407)
        if fixed and not device_mode:
            nwg, _ = self.engine.fast_geometry(pop * P, 1, 1, -1)  # hipets_step runs the general kernel layout
            schedule = self.engine.fast_schedule(1, nwg, self.seed, self.calls * 4096).contiguous()
        for t in range(H):
            act = torch.repeat_interleave(a_seq[:, t, :], P, dim=0).contiguous()  # model_env.py:179-182
            if device_mode:  # (stream ids of a call start at calls * 4096 + 1: 0 means "none" for perm_stream_id)
                nobs, rew, done = self.engine.step(obs, act, mode="device", sample=True, seed=self.seed, stream_id=self.calls * 4096 + 1 + t,
                                                   perm_stream_id=self.calls * 4096 + 1 if fixed else 0)
            else:
                nobs, rew, done = self.engine.step(obs, act, mode="fast", sample=True, seed=self.seed, stream_id=self.calls * 4096 + t,
                                                   member_schedule=schedule)
            if self.reward_fn is not None:
                rew = self.reward_fn(act, nobs)
            if self.termination_fn is not None:
                done = self.termination_fn(act, nobs)
            rew = rew.clone()
            rew[terminated] = 0  # :186
            terminated |= done  # :187
            total += rew  # :188
            obs = nobs
        if self.particle_reduce.kind == "mean":
            return total.reshape(-1, P).mean(dim=1)
        return self.engine.particle_reduce(total.reshape(-1).contiguous(), pop, P)  # (bind_model made the reduction the engine's)


def _rowwise_output(out, n_rows: int, what: str, boolean: bool) -> torch.Tensor:
    """A callable's result over ``n_rows`` rows as a flat [n_rows] tensor: [N] or [N, 1], floats for a reward, bool for a termination."""
    if not isinstance(out, torch.Tensor) or tuple(out.shape) not in ((n_rows,), (n_rows, 1)):
        got = tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__
        raise ValueError(f"{what} must return a tensor of shape [{n_rows}] or [{n_rows}, 1] for {n_rows} rows, got {got}")
    if boolean and out.dtype != torch.bool:
        raise ValueError(f"{what} must return a bool tensor, got {out.dtype}")
    if not boolean and not out.dtype.is_floating_point:
        raise ValueError(f"{what} must return a floating-point tensor, got {out.dtype}")
    return out.reshape(n_rows)


def _same_values(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal with NaNs at equal positions counting as equal."""
    if a.dtype == torch.bool:
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


class CallableTrajectoryEvalFn(_RolloutObjective):
    """``trajectory_eval_fn`` for models whose ``reward_fn`` / ``termination_fn`` are arbitrary Python callables, in ONE rollout
    launch per evaluation.  In ``ModelEnv.evaluate_action_sequences`` (model_env.py:178-191) the dynamics never read the reward or
    the ``terminated`` mask -- terminated rows keep rolling, only their rewards are zeroed -- so the horizon runs as one
    ``hipets_rollout`` that writes every row's predicted states (the kernel's taps), the callables run ONCE over all ``H * B`` rows,
    and ``hipets_trajectory_returns`` applies lines 186-191.  :class:`UnfusedTrajectoryEvalFn` runs the same evaluation as ``H``
    ``hipets_step`` launches with the callables in between.

    THE CALLABLES MUST BE ROW-WISE: ``fn(act [N, A], next_obs [N, obs])`` returns, for every row, a value that depends on that row
    only, for any N.  They are called once per evaluation with ``N = H * B`` rows, time-major -- row ``t * B + c * P + p`` is step t
    of particle p of candidate c, its action ``action_sequences[c, t]`` -- not ``H`` times with ``B`` rows.  A reward returns ``[N]``
    or ``[N, 1]`` floats, a termination ``[N]`` or ``[N, 1]`` bool.  ``check_rowwise`` (default): the objective's FIRST call also
    evaluates both callables on step 0's ``B`` rows alone and compares with the first ``B`` rows of the batched result (that one
    call synchronises with the host); a callable that fails it -- one that normalises over the batch, say -- belongs to
    :class:`UnfusedTrajectoryEvalFn`.  Otherwise a call never synchronises in the in-kernel modes.

    ``reward_fn`` / ``termination_fn``: the arguments, else the spec's ``custom_reward_fn`` / ``custom_termination_fn`` (what
    ``spec_from_model_env(allow_custom_fns=True)`` kept).  Without a reward callable the rewards are the kernel's own (a learned
    reward, or the spec's closed form); without a termination callable the spec's closed-form termination is restated over the
    traced states (:func:`closed_form_dones`).  ``mode``, seed and streams as for :class:`HipTrajectoryEvalFn` (call k runs stream
    k of ``seed``).  The trajectory of a call takes ``H * B * (obs + 1) * 4`` bytes; a call beyond ``max_trajectory_bytes`` raises."""

    _allow_custom_fns = True
    _needs_callable = True  # (a subclass that adds something else to the evaluation runs without one: hipets.value)
    kernel_mode = None  # not a fused-plan target: the optimizers run their per-iteration loops and call it; batched agents refuse it

    def __init__(self, model, num_particles: int, reward_fn=None, termination_fn=None, engine: Optional[Engine] = None,
                 mode: str = "device", seed: int = 0, device=None, rng: Optional[torch.Generator] = None, check_rowwise: bool = True,
                 max_trajectory_bytes: int = 2 << 30, particle_reduce=None):
        super().__init__(model, num_particles, engine, mode, seed, device, rng, particle_reduce)
        self.reward_fn = reward_fn if reward_fn is not None else self.spec.custom_reward_fn
        self.termination_fn = termination_fn if termination_fn is not None else self.spec.custom_termination_fn
        if self._needs_callable and self.reward_fn is None and self.termination_fn is None:
            raise ValueError("neither a reward nor a termination callable: this model's objective is fully fused, use HipTrajectoryEvalFn")
        self.check_rowwise, self.max_trajectory_bytes = bool(check_rowwise), int(max_trajectory_bytes)
        self._rowwise_checked = False

    def _evaluate_callables(self, act_rows: torch.Tensor, obs_rows: torch.Tensor):
        """(rewards [N] or None, dones bool [N] or None) of the callables that are set, shapes and dtypes checked."""
        n = act_rows.shape[0]
        rew = done = None
        if self.reward_fn is not None:
            rew = _rowwise_output(self.reward_fn(act_rows, obs_rows), n, "reward_fn", boolean=False)
        if self.termination_fn is not None:
            done = _rowwise_output(self.termination_fn(act_rows, obs_rows), n, "termination_fn", boolean=True)
        return rew, done

    def _rewards_and_dones(self, a: torch.Tensor, initial_state):
        """One traced rollout of this call's stream and what the evaluation reduces: (next_obs [H, B, obs], rewards f32 [H, B], dones
        bool [H, B]) -- the callables' results where they are set, else the kernel's own rewards / the restated closed-form termination."""
        pop, H, A = a.shape
        P = self.num_particles
        B = pop * P
        next_obs, rewards = self._traced_rollout(a, initial_state)
        obs_rows = next_obs.view(H * B, self.spec.obs_dim)
        if self.reward_fn is None and self.termination_fn is None:
            return next_obs, rewards, closed_form_dones(self.spec, obs_rows).reshape(H, B).contiguous()
        act_rows = a.transpose(0, 1).unsqueeze(2).expand(H, pop, P, A).reshape(H * B, A)  # model_env.py:179-182, all steps at once
        rew, done = self._evaluate_callables(act_rows, obs_rows)
        if self.check_rowwise and not self._rowwise_checked:
            for name, batched, alone in zip(("reward_fn", "termination_fn"), (rew, done), self._evaluate_callables(act_rows[:B], obs_rows[:B])):
                if batched is not None and not _same_values(batched[:B], alone):
                    raise ValueError(f"{name} is not row-wise: evaluated on step 0's {B} rows alone it returns other values than for the "
                                     f"same rows inside the batch of {H * B}.  CallableTrajectoryEvalFn calls it once per evaluation over "
                                     "all steps; use UnfusedTrajectoryEvalFn (one call per step) for such a callable")
            self._rowwise_checked = True
        rewards = rewards if rew is None else rew.to(torch.float32).reshape(H, B).contiguous()
        dones = (closed_form_dones(self.spec, obs_rows) if done is None else done).reshape(H, B).contiguous()
        return next_obs, rewards, dones

    def _trajectory(self, initial_state, action_sequences, details):
        a = self._prep(action_sequences)
        self.calls += 1
        pop, P = a.shape[0], self.num_particles
        next_obs, rewards, dones = self._rewards_and_dones(a, initial_state)
        if not details:
            return self.engine.trajectory_returns(rewards, dones, pop, P)
        returns, row_totals, first_done = self.engine.trajectory_returns(rewards, dones, pop, P, row_totals=True, first_done=True)
        return {"next_obs": next_obs, "rewards": rewards, "dones": dones, "first_done": first_done, "row_totals": row_totals, "returns": returns}

    def __call__(self, initial_state: np.ndarray, action_sequences: torch.Tensor) -> torch.Tensor:
        return self._trajectory(initial_state, action_sequences, False)


class PlaNetTrajectoryEvalFn(_Objective):
    """``trajectory_eval_fn`` for a PlaNet latent model: ``ModelEnv.evaluate_action_sequences`` with
    ``PlaNetModel.sample`` as the transition (mbrl/models/planet.py:531-581, mbrl/algorithms/planet.py), the whole horizon in
    one kernel launch.  Like the reference, the observation argument only fixes the batch size: rollouts start from the
    model's saved posterior sample and belief (``update_posterior``, planet.py:600-640), read from the live model at every
    call, or set with :meth:`set_state` when built from a ``PlaNetSpec``.

    ``mode='device'`` (default; ``'fast'`` is the same thing here): iid standard normals per (row, step, latent dim) drawn
    in-kernel from Philox counters -- a PlaNet model has no ensemble, so there is no member shuffle to approximate and the two
    in-kernel modes of the PETS objective coincide with the reference's semantics; ``mode='exact'``: the reference's draws (one
    ``randn([B, latent])`` per step from the generator) made on the host and injected."""

    _spec_type = PlaNetSpec
    _read_spec = staticmethod(spec_from_planet_model)
    _read_version = staticmethod(planet_version)

    def __init__(self, model, num_particles: int = 1, engine: Optional[Engine] = None, mode: str = "device", seed: int = 0,
                 device=None, rng: Optional[torch.Generator] = None, particle_reduce=None):
        if mode not in ("device", "fast", "exact"):
            raise ValueError("mode must be 'device' (= 'fast': in-kernel draws) or 'exact'")
        self.mode, self._state = mode, None
        if not isinstance(model, PlaNetSpec):
            if rng is None:
                rng = getattr(model, "_rng", None)
            model = getattr(model, "dynamics_model", model)  # a ModelEnv or the PlaNetModel itself
        super().__init__(model, num_particles, engine, seed, device, particle_reduce)
        self._rng = rng

    def _set_engine_model(self, only_if_other: bool = False):
        if not (only_if_other and self.engine.planet_spec is self.spec):
            self.engine.planet_set_model(self.spec)

    def set_state(self, latent: torch.Tensor, belief: torch.Tensor):
        """The posterior sample s_t and belief h_t rollouts start from ([1, latent] / [1, belief])."""
        self._state = (latent.detach().to(self.device, torch.float32).reshape(-1).contiguous(),
                       belief.detach().to(self.device, torch.float32).reshape(-1).contiguous())

    @property
    def kernel_mode(self) -> Optional[str]:
        """'fast' / 'device' when the rollouts draw their eps in-kernel (what the batched agents' fused plans run), None for
        'exact'.  The single-environment optimizers do not route on it."""
        return self.mode if self.mode in ("fast", "device") else None

    def prepare(self):
        """What a call does before its rollout: re-pack changed weights, make them the engine's PlaNet model, fetch the live
        model's saved posterior sample / belief.  Returns (latent0, belief0)."""
        self.bind_model()
        if self._live is not None:  # planet.py:669-672
            if self._live._current_posterior_sample is None or self._live._current_belief is None:
                raise RuntimeError("PlaNetModel has no saved posterior: call update_posterior() before planning")
            self.set_state(self._live._current_posterior_sample, self._live._current_belief)
        if self._state is None:
            raise RuntimeError("no latent state: call set_state(latent, belief) first")
        return self._state

    def evaluate_seeded(self, initial_state, action_sequences: torch.Tensor, seed: int, stream_id: int) -> torch.Tensor:
        """One evaluation with explicit counter-based randomness (what iteration ``stream_id`` of the fused plan runs)."""
        latent0, belief0 = self.prepare()
        a = _device_f32(action_sequences, self.device)
        return self.engine.planet_rollout(a, latent0, belief0, self.num_particles, seed=seed, stream_id=stream_id)

    def __call__(self, initial_state, action_sequences: torch.Tensor) -> torch.Tensor:
        latent0, belief0 = self.prepare()
        a = _device_f32(action_sequences, self.device)
        self.calls += 1
        if self.mode in ("fast", "device"):
            return self.engine.planet_rollout(a, latent0, belief0, self.num_particles, seed=self.seed, stream_id=self.calls)
        pop, H, _ = a.shape
        if self._rng is None:
            self._rng = torch.Generator().manual_seed(self.seed)
        eps = rd.planet_rollout_draws(self.spec.latent_size, pop * self.num_particles, H, self._rng).to(self.device)
        return self.engine.planet_rollout(a, latent0, belief0, self.num_particles, eps=eps.contiguous())


def make_eval_fn(model, num_particles: int, callables: str = "steps", **kw):
    """``agent.set_trajectory_eval_fn(hipets.make_eval_fn(model_env, num_particles))`` on a stock or a
    hipets agent (seam 3 of SURVEY.md section 8b).  Returns the fully fused objective when reward / termination are
    mbrl.env closed forms; when they are arbitrary callables, ``callables='steps'`` (default) returns the unfused objective (one fused
    model step per launch, the callables between the steps) and ``callables='trajectory'`` the one-launch
    :class:`CallableTrajectoryEvalFn` (the callables must be row-wise: they run once over all steps' rows).
    Without a ``mode=`` argument the objective runs ``mode='device'``: the reference's TS1 semantics (one balanced permutation
    of all rows per step, gaussian_mlp.py:201-211), every draw made in-kernel; ``mode='fast'`` is the opt-in block-balanced variant.
    ``particle_reduce=`` (every objective): a :class:`ParticleReduce` or 'mean' / 'min' / 'max', the reduction over the particles.
    ``discount=`` / ``terminal_value=agent`` / ``target_critic=``: any of them returns a :class:`hipets.ValueTrajectoryEvalFn` --
    discounted returns, with an agent ``discount^H min(Q1, Q2)`` of its critic at its actor's mean action as the tail -- for closed-form
    and row-wise callable rewards / terminations alike (``callables`` is not read then)."""
    if callables not in ("steps", "trajectory"):
        raise ValueError(f"callables must be 'steps' or 'trajectory', got {callables!r}")
    value_kw = {k: kw.pop(k) for k in ("discount", "terminal_value", "target_critic") if k in kw}
    if value_kw:  # hipets.value: discounted returns, the agent's critic as the tail (a PlaNet model raises ValueError there)
        from .value import ValueTrajectoryEvalFn

        return ValueTrajectoryEvalFn(model, num_particles, agent=value_kw.get("terminal_value"), discount=value_kw.get("discount", 1.0),
                                     target_critic=bool(value_kw.get("target_critic", False)), **kw)
    if isinstance(model, PlaNetSpec) or is_planet_model(getattr(model, "dynamics_model", model)):
        return PlaNetTrajectoryEvalFn(model, num_particles, **kw)
    try:
        return HipTrajectoryEvalFn(model, num_particles, **kw)
    except UnsupportedModelError:
        if isinstance(model, ModelSpec):
            raise
        spec = spec_from_model_env(model, allow_custom_fns=True)  # raises again if something else is unsupported
        if spec.custom_reward_fn is None and spec.custom_termination_fn is None:
            raise
        if callables == "trajectory":
            return CallableTrajectoryEvalFn(model, num_particles, **kw)
        kw2 = {k: v for k, v in kw.items() if k in ("engine", "seed", "device", "particle_reduce")}
        if kw.get("mode") in ("fast", "device"):
            kw2["step_mode"] = kw["mode"]
        return UnfusedTrajectoryEvalFn(model, num_particles, **kw2)


class _BoundObjective:
    """``obj_fun(action_sequences)`` with the observation bound (trajectory_opt.py:680-681); carries the
    engine handle so optimizers can take the fused path."""

    def __init__(self, eval_fn, obs):
        self.eval_fn = eval_fn
        self.obs = obs

    def __call__(self, action_sequences):
        return self.eval_fn(self.obs, action_sequences)
