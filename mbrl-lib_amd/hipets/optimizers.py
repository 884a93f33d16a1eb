"""Drop-in counterparts of mbrl.planning's trajectory optimizers, backed by libhipets.

Same names, constructor arguments and error behaviour as the reference so that the stock Hydra
configs only swap ``_target_``:

* ``CEMOptimizer``                 <- mbrl/planning/trajectory_opt.py:43-188
* ``MPPIOptimizer``                <- mbrl/planning/trajectory_opt.py:191-311
* ``ICEMOptimizer``                <- mbrl/planning/trajectory_opt.py:314-487

There is no CPU fallback anywhere in this module: every optimizer needs a gfx950 device.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import dist as hdist
from . import reference_draws as rd
from ._lib import IcemParams
from .engine import Engine, get_engine
from .objectives import HipTrajectoryEvalFn, PlaNetTrajectoryEvalFn, _BoundObjective, _device_f32


def _prepare_fused(fused: HipTrajectoryEvalFn, population_sizes: Sequence[int]):
    """What ``fused.__call__`` would do before a rollout, for plans that run as one library call: re-pack the
    weights if the live model changed, make them the engine's current model, validate every batch size."""
    fused.bind_model()
    for n in population_sizes:
        fused.check_batch(int(n))
    if fused.engine.plan_mode != fused.kernel_mode:
        fused.engine.set_plan_mode(fused.kernel_mode)


def _planet_start_states(eval_fn, n_env: int, obs_batch, latent, belief):
    """The start states of a batched PlaNet plan: ``latent`` [n_env, latent] / ``belief`` [n_env, belief], one posterior sample and
    belief per environment (``PlaNetModel.update_posterior`` of each env, planet.py:600-640).  Like ``PlaNetModel.reset``
    (planet.py:656-672), ``obs_batch`` only fixes the batch size.  Also makes the objective's weights the engine's PlaNet model."""
    if len(obs_batch) != n_env:
        raise ValueError(f"obs_batch holds {len(obs_batch)} observations, the agent plans for n_env = {n_env}")
    if latent is None or belief is None:
        raise ValueError("a PlaNet objective plans from per-environment start states: pass latent=[n_env, latent] and belief=[n_env, belief]")
    spec, dev = eval_fn.spec, eval_fn.device
    states = []
    for name, t, width in (("latent", latent, spec.latent_size), ("belief", belief, spec.belief_size)):
        t = torch.as_tensor(t)
        if tuple(t.shape) != (n_env, width):
            raise ValueError(f"{name} must have shape {(n_env, width)}, got {tuple(t.shape)}")
        states.append(t.detach().to(device=dev, dtype=torch.float32).contiguous())
    eval_fn.bind_model()
    return states


def _run_fused_plan(kind: str, args, fused, obs, seed: int, plan_id: Callable[[], int], population_sizes: Sequence[int],
                    n_env: Optional[int] = None, latent=None, belief=None, in_place: Optional[torch.Tensor] = None, **kw):
    """One whole plan inside the library.  ``kind`` is 'cem', 'mppi' or 'icem' and ``args`` the arguments of ``Engine.plan_<kind>``
    up to the start state; the start state, the particles of ``fused``, ``seed``, the plan id and ``kw`` follow.  ``plan_id()`` is
    asked once the start states are accepted (the batched agents count the plans that reach the library).
    ``n_env`` None: an optimizer's plan from the observation ``obs`` (a PlaNet objective: from the model's saved posterior,
    ``prepare``); else a batched agent's, from the observation batch or the ``latent`` / ``belief`` states of a PlaNet objective.
    A PlaNet objective runs ``Engine.plan_planet_<kind>``; an optimizer's plan on an engine with a communicator
    (hipets.dist.init_engine_comm) is shared by the ranks, ``Engine.plan_<kind>_sharded`` under ``hipets.dist.run_sharded``'s
    policy, which puts ``in_place`` -- the persistent state the plan overwrites: MPPI's mean, iCEM's elites, replicated bit for
    bit -- back before a fallback."""
    eng = fused.engine
    planet = isinstance(fused, PlaNetTrajectoryEvalFn)
    if planet:
        plan = getattr(eng, "plan_planet_" + kind)
        start = fused.prepare() if n_env is None else _planet_start_states(fused, n_env, obs, latent, belief)
    else:
        plan = getattr(eng, "plan_" + kind)
        if n_env is not None:
            obs = np.asarray(obs, dtype=np.float32)
            assert obs.shape[0] == n_env
        _prepare_fused(fused, population_sizes)
        start = [obs]
    args = (*args, *start, fused.num_particles)
    kw.update(seed=seed, plan_id=plan_id())
    if n_env is not None:
        return plan(*args, n_env=n_env, **kw)
    if eng.comm_world > 1 and not planet:
        return hdist._plan_sharded(eng, getattr(eng, f"plan_{kind}_sharded"), plan, args, eng.comm_group, in_place, **kw)[0]
    return plan(*args, **kw)


# ---------------------------------------------------------------------------------------------
# optimizers
# ---------------------------------------------------------------------------------------------
class Optimizer:  # trajectory_opt.py:21-40
    def __init__(self):
        pass

    def optimize(self, obj_fun, x0=None, callback=None, **kwargs) -> torch.Tensor:
        raise NotImplementedError


_SEED_COUNTER = [0]


def _default_seed(seed: Optional[int]) -> int:
    """Seed of an optimizer's counter-based streams.  ``None`` derives one from ``torch.initial_seed()`` (what
    ``torch.manual_seed`` set) and a per-process construction counter: reproducible under ``torch.manual_seed`` +
    the same construction order, different for every optimizer built -- WITHOUT consuming torch's global generator (the
    reference's constructors draw nothing: an extra draw here would shift every later reference-order draw, e.g. the
    ``sampler='torch'`` / ``mode='exact'`` replays and model initialisation, by one)."""
    if seed is None:
        _SEED_COUNTER[0] += 1
        z = (int(torch.initial_seed()) + 0x9E3779B97F4A7C15 * _SEED_COUNTER[0]) & (2**64 - 1)  # splitmix64 finaliser
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        seed = z ^ (z >> 31)
    return int(seed) & (2**63 - 1)


class _PlanOptimizer(Optimizer):
    """The front end of the three optimizers: the sampler choice, the engine, the bounds on its device, the seed of the
    counter-based streams and the plan counter; per ``optimize()`` call, whether and how the plan runs inside the library."""

    def __init__(self, device, lower_bound, upper_bound, seed: Optional[int], sampler: str):
        super().__init__()
        if sampler not in ("philox", "torch"):
            raise ValueError("sampler must be 'philox' (device-side, default) or 'torch' (the reference's draws)")
        self.sampler = sampler
        self.engine = get_engine(device)
        self.device = self.engine.device
        self.lower_bound = torch.tensor(lower_bound, device=self.device, dtype=torch.float32).contiguous()
        self.upper_bound = torch.tensor(upper_bound, device=self.device, dtype=torch.float32).contiguous()
        self.seed = _default_seed(seed)
        self.calls = 0

    def _fused_objective(self, obj_fun, eligible: bool = True, planet_ok: bool = False):
        """(fused, seed) of one plan.  ``fused`` is the hipets objective behind ``obj_fun`` when it draws its randomness in-kernel
        on this optimizer's engine, else None.  With one, iteration i of the plan samples AND rolls out with the counter-based
        streams of (seed = this seed ^ the objective's seed, the plan's stream of iteration i), whether the loop runs inside the
        library (one plan call) or here (callback / injected draws / force_generic): both give the same numbers.  ``eligible``:
        the optimizer's own condition; ``planet_ok``: PlaNet latent objectives count too (CEM has a fused PlaNet plan)."""
        fn = obj_fun.eval_fn if isinstance(obj_fun, _BoundObjective) else None
        kinds = (HipTrajectoryEvalFn, PlaNetTrajectoryEvalFn) if planet_ok else HipTrajectoryEvalFn
        if eligible and self.sampler == "philox" and isinstance(fn, kinds) and fn.kernel_mode is not None and fn.engine is self.engine:
            return fn, self.seed ^ fn.seed
        return None, self.seed

    @staticmethod
    def _whole_plan(fused, callback, injected, kwargs) -> bool:
        """Does the plan run as one library call?  With a fused objective and no callback, injected draws (parity tests),
        ``extra_candidates`` or ``force_generic``."""
        return (fused is not None and callback is None and injected is None and kwargs.get("extra_candidates") is None
                and not kwargs.get("force_generic", False))

    def _extra_candidates(self, kwargs, shape, smallest: int):
        """The ``extra_candidates`` of one ``optimize()`` call, checked before anything runs: None, or (rows [num, H, A] clamped to
        the bounds on the device, mask [num, 1, 1] of the rows that are finite throughout).  ``shape``: the plan variable's, ``smallest``:
        the fewest rows an iteration of this plan samples.  Every iteration's population takes them in :meth:`_inject`."""
        extra = kwargs.get("extra_candidates")
        if extra is None:
            return None
        if self.engine.comm_world > 1:
            raise ValueError("extra_candidates on a sharded engine (one with a communicator) is not supported: every rank would have to hold the same rows")
        if len(shape) != 2:
            raise ValueError(f"extra_candidates needs a plan variable [H, A], this plan's is {tuple(shape)}")
        if not isinstance(extra, torch.Tensor) or extra.dtype != torch.float32 or extra.ndim != 3 or tuple(extra.shape[1:]) != tuple(shape):
            got = (tuple(extra.shape), extra.dtype) if isinstance(extra, torch.Tensor) else type(extra).__name__
            raise ValueError(f"extra_candidates must be a float32 tensor [num, {shape[0]}, {shape[1]}], got {got}")
        num = int(extra.shape[0])
        if num > smallest:
            raise ValueError(f"extra_candidates holds {num} rows, the smallest iteration of this plan samples {smallest}")
        extra = extra.detach().to(self.device)
        finite = torch.isfinite(extra).all(dim=2).all(dim=1)[:, None, None]
        return torch.minimum(torch.maximum(extra, self.lower_bound), self.upper_bound), finite

    @staticmethod
    def _inject(population: torch.Tensor, extra):
        """Rows [0, num) of the freshly sampled ``population`` <- the clamped candidates; a candidate row holding a non-finite value
        leaves its row as sampled.  Torch ops on the current stream: no host synchronisation."""
        if extra is not None and extra[0].shape[0]:
            rows, finite = extra
            head = population[:rows.shape[0]]
            head.copy_(torch.where(finite, rows, head))


class CEMOptimizer(_PlanOptimizer):
    """Cross-Entropy Method with device-side sampling and elite refit (trajectory_opt.py:43-188).

    Works with ANY ``obj_fun`` (generic path: one sample kernel + ``obj_fun`` + one refit kernel per
    iteration, no host synchronisation of its own); when ``obj_fun`` is a hipets objective that draws in-kernel (device or fast mode)
    and no callback is given, the whole optimisation is one ``hipets_plan_cem`` call."""

    def __init__(self, num_iterations: int, elite_ratio: float, population_size: int,
                 lower_bound: Sequence[Sequence[float]], upper_bound: Sequence[Sequence[float]], alpha: float,
                 device: torch.device, return_mean_elites: bool = False, clipped_normal: bool = False,
                 seed: Optional[int] = None, sampler: str = "philox"):
        # sampler='torch': the population noise is drawn exactly like the reference does on a CPU device (torch's GLOBAL
        # generator, redraw-until-inside loop of mbrl.util.math.truncated_normal_, util/math.py:69-92), so that with the
        # same torch.manual_seed an agent reproduces the reference's action selection (a parity aid: it synchronises)
        super().__init__(device, lower_bound, upper_bound, seed, sampler)
        self.num_iterations = num_iterations
        self.elite_ratio = elite_ratio
        self.population_size = population_size
        self.elite_num = np.ceil(self.population_size * self.elite_ratio).astype(np.int32)  # :89-91
        self.alpha = alpha
        self.return_mean_elites = return_mean_elites
        self._clipped_normal = clipped_normal
        # the reference's CEM is shape-generic (notebooks/cem_rosenbrock_ex.ipynb optimises a [2] vector):
        # kernels only see the flattened variable; [H, A] bounds keep their meaning for the fused plan path
        if self.lower_bound.ndim == 2:
            H, A = self.lower_bound.shape
        else:
            H, A = int(self.lower_bound.numel()), 1
        self._params = Engine.cem_params(population_size, H, A, num_iterations, int(self.elite_num), alpha,
                                         return_mean_elites, clipped_normal, unbiased_var=True)

    def _init_population_params(self, x0: torch.Tensor):  # :100-108
        mean = x0.clone()
        if self._clipped_normal:
            dispersion = torch.ones_like(mean)
        else:
            dispersion = ((self.upper_bound - self.lower_bound) ** 2) / 16
        return mean, dispersion

    def optimize(self, obj_fun: Callable[[torch.Tensor], torch.Tensor], x0: Optional[torch.Tensor] = None,
                 callback: Optional[Callable[[torch.Tensor, torch.Tensor, int], None]] = None, **kwargs) -> torch.Tensor:
        x0 = x0.to(device=self.device, dtype=torch.float32).contiguous()
        extra = self._extra_candidates(kwargs, x0.shape, int(self.population_size))
        self.calls += 1
        fused, seed = self._fused_objective(obj_fun, eligible=x0.ndim == 2, planet_ok=True)
        noise = kwargs.get("noise")  # optional injected z per iteration (parity tests)
        if self._whole_plan(fused, callback, noise, kwargs):
            return _run_fused_plan("cem", (self._params, x0, self.lower_bound, self.upper_bound), fused, obj_fun.obs, seed,
                                   lambda: self.calls, [self.population_size])  # (a PlaNet objective: hipets_plan_planet_cem)
        p = self._params
        mu, dispersion = self._init_population_params(x0)
        mu, dispersion = mu.contiguous(), dispersion.contiguous()
        best_solution = torch.zeros_like(mu)
        best_value = torch.full((1,), -float("inf"), device=self.device, dtype=torch.float32)
        population = torch.empty((self.population_size,) + tuple(x0.shape), device=self.device, dtype=torch.float32)
        for i in range(self.num_iterations):
            stream = self.calls * self.num_iterations + i
            z = None if noise is None else noise[i].to(self.device, torch.float32).contiguous()
            if z is None and self.sampler == "torch":
                z = rd.population_noise(tuple(population.shape), self._clipped_normal).to(self.device).contiguous()
            self.engine.cem_sample(p, mu, dispersion, self.lower_bound, self.upper_bound, population, z=z, seed=seed, stream_id=stream)
            self._inject(population, extra)
            values = fused.evaluate_seeded(obj_fun.obs, population, seed, stream) if fused is not None else obj_fun(population)
            if callback is not None:
                callback(population, values, i)
            values = _device_f32(values, self.device)
            elites = rd.elite_indices(values, self.elite_num).to(self.device).contiguous() if self.sampler == "torch" else None
            self.engine.cem_refit(p, values, population, mu, dispersion, best_value, best_solution, elites=elites)
        return mu if self.return_mean_elites else best_solution


class MPPIOptimizer(_PlanOptimizer):
    """Model Predictive Path Integral optimizer (trajectory_opt.py:191-311) with device-side sampling, smoothing
    recurrence and importance-weighted update.  Reproduces the reference's behaviour including its quirks
    (SURVEY.md Appendix B4-B6): ``self.mean`` persists across calls and is NOT cleared by ``agent.reset()``;
    ``past_action`` aliases the already-shifted ``mean[0]``; ``sigma`` never reaches the population."""

    def __init__(self, num_iterations: int, population_size: int, gamma: float, sigma: float, beta: float,
                 lower_bound: Sequence[Sequence[float]], upper_bound: Sequence[Sequence[float]], device: torch.device,
                 seed: Optional[int] = None, sampler: str = "philox"):
        # sampler='torch': noise like the reference (global generator, truncated_normal_, :262-271)
        super().__init__(device, lower_bound, upper_bound, seed, sampler)
        self.planning_horizon = len(lower_bound)
        self.population_size = population_size
        self.action_dimension = len(lower_bound[0])
        self.mean = torch.zeros((self.planning_horizon, self.action_dimension), device=self.device, dtype=torch.float32)
        self.var = sigma**2 * torch.ones_like(self.lower_bound)  # kept for API parity; dead in the reference too
        self.beta = beta
        self.gamma = gamma
        self.refinements = num_iterations

    def optimize(self, obj_fun: Callable[[torch.Tensor], torch.Tensor], x0: Optional[torch.Tensor] = None,
                 callback: Optional[Callable[[torch.Tensor, torch.Tensor, int], None]] = None, **kwargs) -> torch.Tensor:
        H, A, pop = self.planning_horizon, self.action_dimension, self.population_size
        extra = self._extra_candidates(kwargs, (H, A), int(pop))
        self.calls += 1
        fused, seed = self._fused_objective(obj_fun)
        noise = kwargs.get("noise")
        if self._whole_plan(fused, callback, noise, kwargs):
            self.mean = self.mean.contiguous()
            _run_fused_plan("mppi", (pop, H, A, self.refinements, self.gamma, self.beta, self.mean, self.lower_bound, self.upper_bound),
                            fused, obj_fun.obs, seed, lambda: self.calls, [pop], in_place=self.mean)
            return self.mean.clone()
        shifted = self.mean.clone()
        shifted[:-1] = self.mean[1:]  # :258
        self.mean = shifted.contiguous()
        past_action = self.mean[0].clone()  # :257 (a view of the shifted tensor; constant across refinements)
        population = torch.empty((pop, H, A), device=self.device, dtype=torch.float32)
        for k in range(self.refinements):
            stream = self.calls * self.refinements + k
            z = None if noise is None else noise[k].to(self.device, torch.float32).contiguous()
            if z is None and self.sampler == "torch":
                z = rd.population_noise((pop, H, A), False).to(self.device).contiguous()
            self.engine.mppi_sample(pop, H, A, self.beta, self.mean, past_action, self.lower_bound, self.upper_bound, population,
                                    z=z, seed=seed, stream_id=stream)
            self._inject(population, extra)
            values = fused.evaluate_seeded(obj_fun.obs, population, seed, stream) if fused is not None else obj_fun(population)
            values = _device_f32(values, self.device)
            if callback is not None:  # the reference calls back after the NaN filter here (:297-300)
                values[values.isnan()] = -1e-10
                callback(population, values, k)
            new_mean = torch.empty_like(self.mean)
            self.engine.mppi_update(pop, H, A, self.gamma, values, population, new_mean)
            self.mean = new_mean
        return self.mean.clone()


class ICEMOptimizer(_PlanOptimizer):
    """Improved CEM (trajectory_opt.py:314-487): decaying population, coloured-noise sampling (device-side inverse
    real DFT), kept / shifted elites, biased variance refit.  ``self.elite`` persists across calls (Appendix B6)."""

    def __init__(self, num_iterations: int, elite_ratio: float, population_size: int, population_decay_factor: float,
                 colored_noise_exponent: float, lower_bound: Sequence[Sequence[float]], upper_bound: Sequence[Sequence[float]],
                 keep_elite_frac: float, alpha: float, device: torch.device, return_mean_elites: bool = False,
                 population_size_module: Optional[int] = None, seed: Optional[int] = None, sampler: str = "philox"):
        # 'torch': every draw of an iteration comes from torch's global CPU generator in the reference's order -- the two
        # spectrum normals of powerlaw_psd_gaussian (util/math.py:372-377), randperm(elite_num) for the kept elites
        # (trajectory_opt.py:446-448), the tail-action normal of the shifted elites (:451-457)
        super().__init__(device, lower_bound, upper_bound, seed, sampler)
        self.num_iterations = num_iterations
        self.elite_ratio = elite_ratio
        self.population_size = population_size
        self.population_decay_factor = population_decay_factor
        self.elite_num = np.ceil(self.population_size * self.elite_ratio).astype(np.int32)
        self.colored_noise_exponent = colored_noise_exponent
        self.initial_var = ((self.upper_bound - self.lower_bound) ** 2) / 16
        self.keep_elite_frac = keep_elite_frac
        self.keep_elite_size = np.ceil(keep_elite_frac * self.elite_num).astype(np.int32)
        self.elite = None
        self.alpha = alpha
        self.return_mean_elites = return_mean_elites
        self.population_size_module = population_size_module
        if self.population_size_module:
            self.keep_elite_size = self._round_up_to_module(self.keep_elite_size, self.population_size_module)

    @staticmethod
    def _round_up_to_module(value: int, module: int) -> int:  # :385-389
        if value % module == 0:
            return value
        return value + (module - value % module)

    def _iteration_size(self, i: int) -> int:  # :419-431
        n = np.ceil(np.max((self.population_size * self.population_decay_factor**-i, 2 * self.elite_num))).astype(np.int32)
        if self.population_size_module:
            n = self._round_up_to_module(n, self.population_size_module)
        return int(n)

    def _extra_rows(self, i: int, has_elite: bool) -> int:
        """Rows iteration i of a plan evaluates beyond its population (trajectory_opt.py:450-466), ``has_elite``: the plan started
        with elites.  None in the first iteration of a plan without elites, the mean in the last of several iterations, else the
        kept elites."""
        if not (has_elite or i > 0):
            return 0
        return 1 if (i == self.num_iterations - 1 and i != 0) else int(self.keep_elite_size)

    def _fused_plan(self, H: int, A: int, has_elite: bool):
        """The fused plan of one optimize(): the rows every iteration evaluates (its population plus its extra rows) and the
        library's IcemParams."""
        iters, keep = int(self.num_iterations), int(self.keep_elite_size)
        sizes = [self._iteration_size(i) + self._extra_rows(i, has_elite) for i in range(iters)]
        p = IcemParams(population_size=int(self.population_size), horizon=H, act_dim=A, num_iterations=iters, elite_num=int(self.elite_num),
                       keep_elite_size=keep, population_size_module=int(self.population_size_module or 0),
                       return_mean_elites=int(bool(self.return_mean_elites)), alpha=float(self.alpha),
                       population_decay_factor=float(self.population_decay_factor), colored_noise_exponent=float(self.colored_noise_exponent))
        return sizes, p

    def optimize(self, obj_fun: Callable[[torch.Tensor], torch.Tensor], x0: Optional[torch.Tensor] = None,
                 callback: Optional[Callable[[torch.Tensor, torch.Tensor, int], None]] = None, **kwargs) -> torch.Tensor:
        eng = self.engine
        x0 = x0.to(device=self.device, dtype=torch.float32).contiguous()
        H, A = x0.shape
        K, keep = int(self.elite_num), int(self.keep_elite_size)
        extra = self._extra_candidates(kwargs, (H, A), min([self._iteration_size(i) for i in range(self.num_iterations)], default=0))
        self.calls += 1
        fused, seed = self._fused_objective(obj_fun)
        inject = kwargs.get("inject")  # optional injected draws per iteration (parity tests)
        if self._whole_plan(fused, callback, inject, kwargs):
            has_elite = self.elite is not None
            sizes, p = self._fused_plan(H, A, has_elite)
            elite = self.elite.contiguous() if has_elite else torch.empty((K, H, A), device=self.device, dtype=torch.float32)
            out = _run_fused_plan("icem", (p, x0, self.lower_bound, self.upper_bound, elite, has_elite), fused, obj_fun.obs, seed,
                                  lambda: self.calls, sizes, in_place=elite, keep_idx=kwargs.get("keep_idx"))
            if self.num_iterations > 0:
                self.elite = elite
            return out
        mu = x0.clone()
        var = self.initial_var.clone().contiguous()
        best_solution = torch.zeros_like(mu)
        best_value = torch.full((1,), -float("inf"), device=self.device, dtype=torch.float32)
        elite_idx = torch.empty(K, dtype=torch.int32, device=self.device)
        for i in range(self.num_iterations):
            n = self._iteration_size(i)
            inj = inject[i] if inject is not None else {}
            if inject is None and self.sampler == "torch":
                inj = rd.icem_iteration_draws(n, H, A, K, keep, self.elite is not None, i == 0)
            sid = (self.calls * self.num_iterations + i) * 4
            population = torch.empty((n + self._extra_rows(i, self.elite is not None), H, A), device=self.device, dtype=torch.float32)
            normals = inj.get("normals")
            if normals is not None:
                normals = normals.to(self.device, torch.float32).contiguous()
            eng.icem_sample(n, H, A, self.colored_noise_exponent, mu, var, self.lower_bound, self.upper_bound, population,
                            normals=normals, seed=seed, stream_id=sid)
            self._inject(population[:n], extra)  # (the sampled part: kept / shifted elites and the mean row stay)
            if self.elite is not None:
                if "keep_perm" in inj:
                    perm = inj["keep_perm"].to(self.device)
                else:  # torch.randperm(elite_num)[:keep] (:446-448): index plumbing, stays a torch op
                    perm = torch.randperm(K, device=self.device)
                kept = torch.index_select(self.elite, dim=0, index=perm[:keep]).contiguous()
                if i == 0:  # :450-462
                    en = inj.get("end_noise")
                    if en is not None:
                        en = en.to(self.device, torch.float32).contiguous()
                    eng.icem_shift(kept.shape[0], H, A, kept, mu, var, population[n:], end_noise=en, seed=seed,
                                   stream_id=sid + 1)
                elif i == self.num_iterations - 1:  # :463-464
                    population[n:] = mu.unsqueeze(0)
                else:  # :465-466
                    population[n:] = kept
            values = fused.evaluate_seeded(obj_fun.obs, population, seed, sid + 3) if fused is not None else obj_fun(population)
            if callback is not None:
                callback(population, values, i)
            values = _device_f32(values, self.device)
            p = Engine.cem_params(population.shape[0], H, A, self.num_iterations, K, self.alpha, self.return_mean_elites,
                                  clipped_normal=False, unbiased_var=False)  # biased variance (:479)
            elites = rd.elite_indices(values, K).to(self.device).contiguous() if (self.sampler == "torch" and inject is None) else None
            eng.cem_refit(p, values, population, mu, var, best_value, best_solution, elite_idx, elites=elites)
            new_elite = torch.empty((K, H, A), device=self.device, dtype=torch.float32)
            eng.gather_rows(population, elite_idx, new_elite)  # self.elite = population[elite_idx] (:476)
            self.elite = new_elite
        return mu if self.return_mean_elites else best_solution
