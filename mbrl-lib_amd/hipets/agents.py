"""Drop-in counterparts of mbrl.planning's agents, backed by libhipets.

Same names, constructor arguments and error behaviour as the reference so that the stock Hydra
configs only swap ``_target_``:

* ``TrajectoryOptimizer``          <- mbrl/planning/trajectory_opt.py:490-572
* ``TrajectoryOptimizerAgent``     <- mbrl/planning/trajectory_opt.py:575-716
* ``create_trajectory_optim_agent_for_model`` <- :719-749

and the batched agents, which plan for many environments in one set of launches.
"""
from __future__ import annotations

import importlib
import time
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import dist as hdist
from ._lib import HipetsError
from .engine import Engine
from .objectives import HipTrajectoryEvalFn, PlaNetTrajectoryEvalFn, _BoundObjective, make_eval_fn
from .optimizers import ICEMOptimizer, Optimizer, _PlanOptimizer, _run_fused_plan

# ---------------------------------------------------------------------------------------------
# TrajectoryOptimizer / Agent
# ---------------------------------------------------------------------------------------------
_TARGET_ALIASES = {
    # stock targets are redirected to the fused implementations when an agent of this module builds them
    "mbrl.planning.CEMOptimizer": "hipets.planning.CEMOptimizer",
    "mbrl.planning.trajectory_opt.CEMOptimizer": "hipets.planning.CEMOptimizer",
    "mbrl.planning.ICEMOptimizer": "hipets.planning.ICEMOptimizer",
    "mbrl.planning.trajectory_opt.ICEMOptimizer": "hipets.planning.ICEMOptimizer",
    "mbrl.planning.MPPIOptimizer": "hipets.planning.MPPIOptimizer",
    "mbrl.planning.trajectory_opt.MPPIOptimizer": "hipets.planning.MPPIOptimizer",
    # conf/algorithm/pets.yaml:5 handed to hipets.create_trajectory_optim_agent_for_model unchanged
    "mbrl.planning.TrajectoryOptimizerAgent": "hipets.planning.TrajectoryOptimizerAgent",
    "mbrl.planning.trajectory_opt.TrajectoryOptimizerAgent": "hipets.planning.TrajectoryOptimizerAgent",
}


def _cfg_to_dict(cfg) -> dict:
    """Top-level keys of a plain dict or an OmegaConf ``DictConfig`` as a dict.  OmegaConf raises ``MissingMandatoryValue``
    (not a KeyError) when a key that holds ``???`` is read -- and the stock configs ship ``lower_bound: ???``,
    ``upper_bound: ???``, ``action_lb: ???``, ``action_ub: ???`` (conf/action_optimizer/*.yaml, conf/algorithm/pets.yaml)
    -- so missing values are returned as the string "???" and filtered by the callers, like hydra's instantiate is fed by
    the reference only after it has written the bounds into the config (trajectory_opt.py:525-527, core.py:101-106)."""
    try:
        from omegaconf import OmegaConf  # real OmegaConf: resolves interpolations too

        if OmegaConf.is_config(cfg):
            return dict(OmegaConf.to_container(cfg, resolve=True, throw_on_missing=False))
    except ImportError:
        pass
    out = {}
    for k in list(cfg.keys()):
        try:
            out[k] = cfg[k]
        except Exception as exc:  # omegaconf.errors.MissingMandatoryValue of a DictConfig-like object
            if type(exc).__name__ != "MissingMandatoryValue":
                raise
            out[k] = "???"
    return out


def _is_missing(v) -> bool:
    return isinstance(v, str) and v == "???"


def _instantiate(cfg, **overrides):
    """A minimal ``_target_`` resolver (object construction only; the reference does exactly this through
    hydra.utils.instantiate at trajectory_opt.py:527,741).  Works on plain dicts and OmegaConf nodes; placeholders
    ("???") that no override filled are dropped so the target's own defaults / errors apply."""
    kwargs = _cfg_to_dict(cfg)
    kwargs.update(overrides)
    target = kwargs.pop("_target_")
    target = _TARGET_ALIASES.get(target, target)
    kwargs = {k: v for k, v in kwargs.items() if not _is_missing(v)}
    mod, _, name = target.rpartition(".")
    return getattr(importlib.import_module(mod), name)(**kwargs)


class _OptimizerSnapshot:
    """What one ``optimizer.optimize`` call changes besides returning a plan -- the counter-based stream positions
    (``calls`` of the optimizer and of a hipets objective) and the state that persists across plans (MPPI ``mean``, iCEM
    ``elite``: SURVEY.md Appendix B6) -- so that a plan whose rollouts were cut short can be re-run as if it never ran."""

    def __init__(self, optimizer, obj_fun):
        self.optimizer = optimizer
        self.eval_fn = getattr(obj_fun, "eval_fn", obj_fun)
        inner = getattr(self.eval_fn, "eval_fn", None)  # dist.ShardedEvalFn wraps the hipets objective
        self.counters = [o for o in (optimizer, self.eval_fn, inner) if isinstance(getattr(o, "calls", None), int)]
        self.calls = [o.calls for o in self.counters]
        self.state = {k: (getattr(optimizer, k).clone() if torch.is_tensor(getattr(optimizer, k)) else getattr(optimizer, k))
                      for k in ("mean", "elite") if hasattr(optimizer, k)}
        self.engines = []
        for o in (optimizer, self.eval_fn, inner):
            eng = getattr(o, "engine", None)
            if isinstance(eng, Engine) and eng not in self.engines:
                self.engines.append(eng)

    def engines_report_timeout(self) -> bool:
        """Did a persistent DEVICE-mode rollout of the plan give up on THIS rank -- or, when the ranks plan in lockstep, on ANY rank?
        With a ``dist.ShardedEvalFn`` objective every iteration is a host-side collective all ranks must take part in: a rank that
        re-ran its plan alone would issue a second series of all-gathers its peers never match.  The flag is therefore all-reduced
        over the objective's group first, and the plan is re-run on every rank or on none.  (The fused sharded plans agree inside
        ``hipets.dist.run_sharded`` and have consumed the flag by the time this is asked.)"""
        hit = False
        for eng in self.engines:
            hit = eng.check_async_error() or hit
        if isinstance(self.eval_fn, hdist.ShardedEvalFn) and hdist.is_distributed():
            hit = bool(hdist._worst_status(int(hit), self.eval_fn.group))
        return hit

    def restore(self):
        for o, c in zip(self.counters, self.calls):
            o.calls = c
        for k, v in self.state.items():
            setattr(self.optimizer, k, v.clone() if torch.is_tensor(v) else v)


def _refuse_latent_prior(eval_fn):
    if isinstance(eval_fn, PlaNetTrajectoryEvalFn):
        raise ValueError("a policy prior rolls an actor over observations: a PlaNet objective plans over latent states, for which there is none")


class TrajectoryOptimizer:
    """trajectory_opt.py:490-572: tiles the action bounds over the horizon, instantiates the optimizer,
    warm-starts each call from the previous solution shifted by ``replan_freq``."""

    def __init__(self, optimizer_cfg, action_lb: np.ndarray, action_ub: np.ndarray, planning_horizon: int,
                 replan_freq: int = 1, keep_last_solution: bool = True):
        lower = np.tile(action_lb, (planning_horizon, 1)).tolist()  # :525
        upper = np.tile(action_ub, (planning_horizon, 1)).tolist()  # :526
        self.optimizer: Optimizer = _instantiate(optimizer_cfg, lower_bound=lower, upper_bound=upper)  # :527
        device = self.optimizer.device
        self.initial_solution = ((torch.tensor(action_lb) + torch.tensor(action_ub)) / 2).float().to(device)
        self.initial_solution = self.initial_solution.repeat((planning_horizon, 1))
        self.previous_solution = self.initial_solution.clone()
        self.replan_freq = replan_freq
        self.keep_last_solution = keep_last_solution
        self.horizon = planning_horizon

    def optimize(self, trajectory_eval_fn: Callable[[torch.Tensor], torch.Tensor],
                 callback: Optional[Callable] = None, extra_candidates: Optional[torch.Tensor] = None) -> np.ndarray:
        """(A plan that is re-run after a timed-out rollout -- see below -- invokes ``callback`` again for every iteration of the
        second run: a callback that accumulates sees the iterations of the voided attempt followed by those of the valid one.)
        ``extra_candidates`` [num, H, A]: rows every iteration's population takes (the optimizers' keyword); a re-run reuses them."""
        kw = {}
        if extra_candidates is not None:
            if not isinstance(self.optimizer, _PlanOptimizer):  # (a stock optimizer's **kwargs would swallow the rows unused)
                raise TypeError(f"{type(self.optimizer).__name__}.optimize takes no extra_candidates keyword: a policy prior needs one of "
                                "hipets' optimizers (CEMOptimizer, MPPIOptimizer, ICEMOptimizer)")
            kw["extra_candidates"] = extra_candidates
        snapshot = _OptimizerSnapshot(self.optimizer, trajectory_eval_fn)
        best_solution = self.optimizer.optimize(trajectory_eval_fn, x0=self.previous_solution, callback=callback, **kw)
        plan = best_solution.cpu().numpy()  # the one device->host sync of a plan (:568)
        # Everything the plan enqueued has executed now.  If a persistent DEVICE-mode rollout inside it gave up waiting for
        # another workgroup's rows (CUs taken by another process: hipets.h, hipets_check_async_error) the plan was built on
        # invalid returns: never hand it out.  The engine has switched to per-step launches, which return the same bits the
        # persistent form would have: put the optimizer back where it was and run the SAME plan again.
        for _ in range(2):
            if not snapshot.engines_report_timeout():
                break
            snapshot.restore()
            best_solution = self.optimizer.optimize(trajectory_eval_fn, x0=self.previous_solution, callback=callback, **kw)
            plan = best_solution.cpu().numpy()
        else:
            if snapshot.engines_report_timeout():
                raise HipetsError("DEVICE-mode rollouts keep timing out although persistent launches are off")
        if self.keep_last_solution:  # :563-567
            self.previous_solution = best_solution.roll(-self.replan_freq, dims=0)
            self.previous_solution[-self.replan_freq:] = self.initial_solution[0]
        return plan

    def reset(self):
        self.previous_solution = self.initial_solution.clone()


class Agent:  # mbrl/planning/core.py:18-49
    def act(self, obs: np.ndarray, **_kwargs) -> np.ndarray:
        raise NotImplementedError

    def plan(self, obs: np.ndarray, **_kwargs) -> np.ndarray:
        return self.act(obs, **_kwargs)

    def reset(self):
        pass


class TrajectoryOptimizerAgent(Agent):
    """trajectory_opt.py:575-716 with the same public methods (``set_trajectory_eval_fn``, ``reset``,
    ``act``, ``plan``) and the same RuntimeError when no objective was set (:673-676)."""

    def __init__(self, optimizer_cfg, action_lb: Sequence[float], action_ub: Sequence[float], planning_horizon: int = 1,
                 replan_freq: int = 1, verbose: bool = False, keep_last_solution: bool = True):
        self.optimizer = TrajectoryOptimizer(optimizer_cfg, np.array(action_lb), np.array(action_ub),
                                             planning_horizon=planning_horizon, replan_freq=replan_freq,
                                             keep_last_solution=keep_last_solution)
        self.optimizer_args = {"optimizer_cfg": optimizer_cfg, "action_lb": np.array(action_lb),
                               "action_ub": np.array(action_ub)}
        self.trajectory_eval_fn = None
        self.policy_prior = None
        self.actions_to_use: List[np.ndarray] = []
        self.replan_freq = replan_freq
        self.verbose = verbose

    def set_trajectory_eval_fn(self, trajectory_eval_fn):
        if self.policy_prior is not None:
            _refuse_latent_prior(trajectory_eval_fn)
        self.trajectory_eval_fn = trajectory_eval_fn

    def set_policy_prior(self, prior):
        """``prior``: a :class:`hipets.PolicyPrior` -- per plan its action sequences, the learned policy rolled through the model from
        the plan's observation, enter every iteration's population (the optimizers' ``extra_candidates``); None: plans run as
        without one (the fused one-call plan where the objective allows it)."""
        if prior is not None:
            if not callable(getattr(prior, "sequences", None)):
                raise TypeError(f"a policy prior needs a sequences(obs, horizon=...) method, got {type(prior).__name__}")
            _refuse_latent_prior(self.trajectory_eval_fn)
        self.policy_prior = prior

    def _prior_candidates(self, obs):
        """the plan's extra candidates: computed ONCE per plan, before the optimizer runs (a re-run plan reuses them)"""
        if self.policy_prior is None:
            return None
        return self.policy_prior.sequences(obs, horizon=self.optimizer.horizon)

    def reset(self, planning_horizon: Optional[int] = None):
        if planning_horizon:  # :644-651
            old = self.optimizer.optimizer
            self.optimizer = TrajectoryOptimizer(self.optimizer_args["optimizer_cfg"], self.optimizer_args["action_lb"],
                                                 self.optimizer_args["action_ub"], planning_horizon=planning_horizon,
                                                 replan_freq=self.replan_freq)
            # the rebuilt optimizer continues the old one's counter-based streams (same seed, call counter carried over)
            # instead of replaying them from plan 1: the reference's global generator keeps advancing across resets too
            new = self.optimizer.optimizer
            if hasattr(old, "calls") and hasattr(new, "calls"):
                new.calls = old.calls
                if hasattr(old, "seed") and _cfg_to_dict(self.optimizer_args["optimizer_cfg"]).get("seed") is None:
                    new.seed = old.seed
        self.optimizer.reset()

    def _require_eval_fn(self):
        if self.trajectory_eval_fn is None:
            raise RuntimeError("Please call `set_trajectory_eval_fn()` before using TrajectoryOptimizerAgent")

    def act(self, obs: np.ndarray, optimizer_callback: Optional[Callable] = None, **_kwargs) -> np.ndarray:
        self._require_eval_fn()
        plan_time = 0.0
        if not self.actions_to_use:  # re-plan is necessary (:678)
            start_time = time.time()
            plan = self.optimizer.optimize(_BoundObjective(self.trajectory_eval_fn, obs), callback=optimizer_callback,
                                           extra_candidates=self._prior_candidates(obs))
            plan_time = time.time() - start_time
            self.actions_to_use.extend([a for a in plan[: self.replan_freq]])
        action = self.actions_to_use.pop(0)
        if self.verbose:
            print(f"Planning time: {plan_time:.3f}")
        return action

    def plan(self, obs: np.ndarray, **_kwargs) -> np.ndarray:
        self._require_eval_fn()
        return self.optimizer.optimize(_BoundObjective(self.trajectory_eval_fn, obs), extra_candidates=self._prior_candidates(obs))


class _BatchedAgent(Agent):
    """What the batched agents share: action bounds tiled over the horizon, the warm start (the bounds' midpoint, shifted by
    ``replan_freq`` after every plan, trajectory_opt.py:563-567), an objective with in-kernel randomness, and the start states of
    a plan: the observation batch of an ensemble objective, or the ``latent=`` / ``belief=`` states of a PlaNet one."""

    def __init__(self, eval_fn: HipTrajectoryEvalFn, n_env: int, action_lb: Sequence[float], action_ub: Sequence[float],
                 planning_horizon: int, replan_freq: int = 1, seed: int = 0):
        if eval_fn.kernel_mode is None:
            raise ValueError("batched planning needs an objective with in-kernel randomness (mode='device' or 'fast')")
        self.eval_fn, self.engine, self.device = eval_fn, eval_fn.engine, eval_fn.device
        self.n_env, self.horizon, self.replan_freq = int(n_env), int(planning_horizon), int(replan_freq)
        lb, ub = np.asarray(action_lb, np.float32), np.asarray(action_ub, np.float32)
        self.act_dim = int(lb.shape[0])
        self.lower = torch.tensor(np.tile(lb, (planning_horizon, 1)), device=self.device).contiguous()
        self.upper = torch.tensor(np.tile(ub, (planning_horizon, 1)), device=self.device).contiguous()
        self.initial_solution = torch.tensor((lb + ub) / 2, device=self.device).repeat(self.n_env, planning_horizon, 1).contiguous()
        self.previous_solution = self.initial_solution.clone()
        self.seed, self.calls = int(seed), 0

    def reset(self):
        self.previous_solution = self.initial_solution.clone()

    def _next_plan_id(self) -> int:
        self.calls += 1
        return self.calls

    def set_policy_prior(self, prior):
        raise NotImplementedError("batched plans run inside the library, which takes no extra candidates: a policy prior needs a TrajectoryOptimizerAgent")

    @staticmethod
    def _refuse_extra(kwargs):
        if kwargs.get("extra_candidates") is not None:
            raise ValueError("batched plans run inside the library, which takes no extra_candidates: use a TrajectoryOptimizerAgent with a policy prior")

    def _plan(self, kind: str, args, obs_batch, latent, belief, population_sizes, **kw):
        """One plan call for all environments, see :func:`_run_fused_plan`."""
        return _run_fused_plan(kind, args, self.eval_fn, obs_batch, self.seed ^ self.eval_fn.seed, self._next_plan_id, population_sizes,
                               n_env=self.n_env, latent=latent, belief=belief, **kw)

    def _shift(self, best: torch.Tensor) -> np.ndarray:
        """The next plan's warm start from this plan's ``best`` [n_env, H, A]; returns ``best`` on the host."""
        self.previous_solution = best.roll(-self.replan_freq, dims=1)
        self.previous_solution[:, -self.replan_freq:] = self.initial_solution[:, :1]
        self.previous_solution = self.previous_solution.contiguous()
        return best.cpu().numpy()

    def act(self, obs_batch: np.ndarray, latent=None, belief=None, **_kwargs) -> np.ndarray:
        """One action per environment, [n_env, A]."""
        self._refuse_extra(_kwargs)
        return self.plan(obs_batch, latent=latent, belief=belief)[:, 0]


class BatchedCEMAgent(_BatchedAgent):
    """Batched planning: one CEM plan per environment for ``n_env`` environments (vectorised envs,
    MPC for many agents) in ONE set of launches.  Same algorithm per environment as ``TrajectoryOptimizerAgent`` +
    ``CEMOptimizer`` (warm start shifted by ``replan_freq`` per environment, trajectory_opt.py:563-567); a single cfg2
    plan leaves 36 of 256 CUs idle, a batch fills the chip.  The rollouts run the objective's randomness mode: 'device' (default:
    one balanced permutation per step over the rows of ALL environments -- every row meets every member with probability 1 / M and
    the members stay exactly balanced, as in a single reference plan) or 'fast'.

    With a ``PlaNetTrajectoryEvalFn`` the environments' latent start states come as keyword arguments:
    ``plan(obs_batch, latent=[n_env, latent], belief=[n_env, belief])``; eps are drawn in-kernel (hipets_plan_planet_cem_batched)."""

    def __init__(self, eval_fn: HipTrajectoryEvalFn, n_env: int, action_lb: Sequence[float], action_ub: Sequence[float],
                 planning_horizon: int, num_iterations: int, elite_ratio: float, population_size: int, alpha: float,
                 return_mean_elites: bool = True, clipped_normal: bool = False, replan_freq: int = 1, seed: int = 0):
        super().__init__(eval_fn, n_env, action_lb, action_ub, planning_horizon, replan_freq, seed)
        self.elite_num = int(np.ceil(population_size * elite_ratio))
        self._params = Engine.cem_params(population_size, planning_horizon, self.act_dim, num_iterations, self.elite_num, alpha,
                                         return_mean_elites, clipped_normal, unbiased_var=True)

    def plan(self, obs_batch: np.ndarray, latent=None, belief=None, **_kwargs) -> np.ndarray:
        self._refuse_extra(_kwargs)
        best = self._plan("cem", (self._params, self.previous_solution, self.lower, self.upper), obs_batch, latent, belief,
                          [self._params.population_size])
        return self._shift(best)


class BatchedMPPIAgent(_BatchedAgent):
    """Batched planning with MPPI: ``MPPIOptimizer.optimize`` (trajectory_opt.py:238-311) for ``n_env``
    environments in one set of launches (hipets_plan_mppi_batched).  Every environment keeps its own persistent mean,
    shifted one step per plan like the reference's (Appendix B4-B6).  A ``PlaNetTrajectoryEvalFn`` plans from
    ``latent=`` / ``belief=`` start states as in :class:`BatchedCEMAgent` (hipets_plan_planet_mppi_batched)."""

    def __init__(self, eval_fn: HipTrajectoryEvalFn, n_env: int, action_lb: Sequence[float], action_ub: Sequence[float],
                 planning_horizon: int, num_iterations: int, population_size: int, gamma: float, sigma: float, beta: float,
                 seed: int = 0):
        super().__init__(eval_fn, n_env, action_lb, action_ub, planning_horizon, seed=seed)
        self.mean = torch.zeros(self.n_env, self.horizon, self.act_dim, device=self.device)
        self.refinements, self.population_size, self.gamma, self.sigma, self.beta = int(num_iterations), int(population_size), gamma, sigma, beta

    def plan(self, obs_batch: np.ndarray, latent=None, belief=None, **_kwargs) -> np.ndarray:
        self._refuse_extra(_kwargs)
        self._plan("mppi", (self.population_size, self.horizon, self.act_dim, self.refinements, self.gamma, self.beta,
                   self.mean, self.lower, self.upper), obs_batch, latent, belief, [self.population_size])
        return self.mean.cpu().numpy()


class BatchedICEMAgent(_BatchedAgent):
    """Batched planning with iCEM: ``ICEMOptimizer.optimize`` (trajectory_opt.py:391-487) for ``n_env``
    environments in one set of launches (hipets_plan_icem_batched): per-environment mean / variance / persistent elites,
    warm start shifted by ``replan_freq`` per environment (trajectory_opt.py:563-567).  A ``PlaNetTrajectoryEvalFn`` plans from
    ``latent=`` / ``belief=`` start states as in :class:`BatchedCEMAgent` (hipets_plan_planet_icem_batched)."""

    def __init__(self, eval_fn: HipTrajectoryEvalFn, n_env: int, action_lb: Sequence[float], action_ub: Sequence[float],
                 planning_horizon: int, num_iterations: int, elite_ratio: float, population_size: int, population_decay_factor: float,
                 colored_noise_exponent: float, keep_elite_frac: float, alpha: float, return_mean_elites: bool = True,
                 population_size_module: Optional[int] = None, replan_freq: int = 1, seed: int = 0):
        super().__init__(eval_fn, n_env, action_lb, action_ub, planning_horizon, replan_freq, seed)
        # sizes and parameters exactly as ICEMOptimizer computes them (:363-389)
        self._opt = ICEMOptimizer(num_iterations, elite_ratio, population_size, population_decay_factor, colored_noise_exponent,
                                  self.lower.tolist(), self.upper.tolist(), keep_elite_frac, alpha, self.device,
                                  return_mean_elites=return_mean_elites, population_size_module=population_size_module, seed=seed)
        self.elite = torch.empty(self.n_env, int(self._opt.elite_num), self.horizon, self.act_dim, device=self.device)
        self.has_elite = False  # (the elites persist across reset(), like ICEMOptimizer.elite, Appendix B6)

    def plan(self, obs_batch: np.ndarray, keep_idx: Optional[torch.Tensor] = None, latent=None, belief=None, **_kwargs) -> np.ndarray:
        self._refuse_extra(_kwargs)
        sizes, params = self._opt._fused_plan(self.horizon, self.act_dim, self.has_elite)
        best = self._plan("icem", (params, self.previous_solution, self.lower, self.upper, self.elite, self.has_elite),
                          obs_batch, latent, belief, sizes, keep_idx=keep_idx)
        if params.num_iterations > 0:
            self.has_elite = True
        return self._shift(best)


def complete_agent_cfg(env, agent_cfg):
    """The subset of mbrl/planning/core.py:71-123 a trajectory-optimizer agent config needs: fill
    ``action_lb`` / ``action_ub`` placeholders ("???") from the action space.  Works on plain dicts and on
    OmegaConf DictConfigs (whose "???" values raise MissingMandatoryValue when read)."""
    have = _cfg_to_dict(agent_cfg)
    if "action_lb" in have and _is_missing(have["action_lb"]):
        agent_cfg["action_lb"] = env.action_space.low.tolist()
    if "action_ub" in have and _is_missing(have["action_ub"]):
        agent_cfg["action_ub"] = env.action_space.high.tolist()
    return agent_cfg


def create_trajectory_optim_agent_for_model(model_env, agent_cfg, num_particles: int = 1, policy_prior=None, **eval_kw):
    """trajectory_opt.py:719-749, with the objective bound to the fused kernel.  ``policy_prior``: a :class:`hipets.PolicyPrior` for
    ``agent.set_policy_prior``."""
    complete_agent_cfg(model_env, agent_cfg)
    agent = _instantiate(agent_cfg)
    agent.set_trajectory_eval_fn(make_eval_fn(model_env, num_particles, **eval_kw))
    if policy_prior is not None:
        agent.set_policy_prior(policy_prior)
    return agent
