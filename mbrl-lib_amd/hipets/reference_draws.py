"""What the reference draws from torch's generators, and in which order: the whole contract of ``mode='exact'`` objectives and
``sampler='torch'`` optimizers, stated once.  No engine, no GPU: every function consumes the generators exactly like the reference
lines it cites and returns CPU tensors; the callers move them to their device and hand them to the kernels.

Two generators are in play.  torch's GLOBAL generator supplies every ``randperm`` (GaussianMLP ignores the generator it is handed,
gaussian_mlp.py:203-205, 374-375) and all of the optimizers' noise (trajectory_opt.py draws without a generator); ``rng`` --
``ModelEnv._rng`` (model_env.py:56-59) -- supplies BasicEnsemble's ``randint`` member maps and every model's ``normal_``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch


def _basic(spec) -> bool:
    return spec.ensemble_kind == "basic_ensemble"


def reset_draws(spec, B: int, rng: torch.Generator) -> Optional[torch.Tensor]:
    """``ModelEnv.reset`` (model_env.py:62-85 -> model.py:404-407): the TS-infinity map of ``fixed_model`` propagation, None for the
    other propagations.  GaussianMLP: ``randperm(B)`` from the GLOBAL generator (gaussian_mlp.py:363-375); BasicEnsemble: [B] member
    slots, ``randint`` from ``rng`` (basic_ensemble.py:255-260)."""
    if spec.propagation != "fixed_model":
        return None
    if _basic(spec):
        return torch.randint(len(spec.members), (B,), generator=rng)
    return torch.randperm(B)  # gaussian_mlp.py:375 at reset


def step_draws(spec, B: int, rng: torch.Generator, sample: bool) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """``ModelEnv.step`` (model_env.py:87-140 -> model.py:440-473): (map, eps) of one transition.  ``map`` is this step's
    ``random_model`` draw, else None -- GaussianMLP: ``randperm(B)`` from the GLOBAL generator (gaussian_mlp.py:205), BasicEnsemble:
    ``randint`` from ``rng`` (basic_ensemble.py:122-129), BEFORE this step's normal.  ``eps`` [B, out] is the standard normal behind
    ``torch.normal(means, stds, generator=rng)`` (model.py:471-473), None for deterministic models and ``sample=False``."""
    perm = None
    if spec.propagation == "random_model":
        perm = torch.randint(len(spec.members), (B,), generator=rng) if _basic(spec) else torch.randperm(B)
    eps = None
    if sample and not spec.deterministic:
        eps = torch.empty(B, spec.out_dim).normal_(0.0, 1.0, generator=rng)
    return perm, eps


def rollout_draws(spec, B: int, H: int, rng: torch.Generator):
    """``ModelEnv.evaluate_action_sequences`` (model_env.py:145-191) is one reset and H sampling steps, so its draws are
    :func:`reset_draws` followed by H :func:`step_draws` (reference consumption order), stacked:
    returns (perms, members, eps) as ``Engine.rollout`` takes them.  The map -- [B] of the reset for ``fixed_model``, [H, B] of the
    steps for ``random_model`` -- is ``perms`` for a GaussianMLP model and ``members`` for a BasicEnsemble one; eps is [H, B, out]."""
    fixed = reset_draws(spec, B, rng)
    steps = [step_draws(spec, B, rng, True) for _ in range(H)]
    maps = torch.stack([m for m, _ in steps]) if spec.propagation == "random_model" else fixed
    eps = None if spec.deterministic else torch.stack([e for _, e in steps])
    return (None, maps, eps) if _basic(spec) else (maps, None, eps)


def device_generator_draws(spec, B: int, H: int, g: torch.Generator):
    """NOT reference order: the 'device' / 'exact_device' objective of a BasicEnsemble model (GaussianMLP models draw in-kernel) makes
    the reference's iid randint member maps (basic_ensemble.py:122-129, 255-260) and eps with a torch DEVICE generator, all maps
    first, then all eps.  Returns (members, eps) on the generator's device."""
    members = eps = None
    M = len(spec.members)
    if spec.propagation == "random_model":
        members = torch.randint(M, (H, B), device=g.device, generator=g)
    elif spec.propagation == "fixed_model":
        members = torch.randint(M, (B,), device=g.device, generator=g)
    if not spec.deterministic:
        eps = torch.randn(H, B, spec.out_dim, device=g.device, generator=g)
    return members, eps


def planet_rollout_draws(latent_size: int, B: int, H: int, rng: torch.Generator) -> torch.Tensor:
    """A PlaNet rollout (planet.py:531-581 -> 299-305): one ``randn([B, latent])`` per step from ``rng``, on the generator's own
    device (planet.py:223 builds it on the model's).  [H, B, latent]."""
    return torch.stack([torch.randn(B, latent_size, generator=rng, device=rng.device) for _ in range(H)])


def population_noise(shape, clipped_normal: bool) -> torch.Tensor:
    """The standard-normal draws of CEMOptimizer._sample_population on a CPU device, from torch's global generator:
    ``randn`` for the clipped-normal branch (trajectory_opt.py:116-117), otherwise mbrl.util.math.truncated_normal_
    (util/math.py:69-92): N(0, 1), entries outside [-2, 2] redrawn until none is left."""
    if clipped_normal:
        return torch.randn(shape)
    t = torch.zeros(shape)
    torch.nn.init.normal_(t, mean=0.0, std=1.0)
    while True:
        cond = torch.logical_or(t < -2.0, t > 2.0)
        n = int(torch.sum(cond).item())
        if n == 0:
            return t
        t[cond] = torch.normal(0.0, 1.0, size=(n,))


def icem_iteration_draws(n: int, H: int, A: int, elite_num: int, keep: int, has_elite: bool, first: bool) -> Dict[str, torch.Tensor]:
    """Every draw of one ICEMOptimizer iteration, from torch's global CPU generator in the reference's order: the two spectrum
    normals of powerlaw_psd_gaussian (util/math.py:372-377) as ``normals`` [2, n, A, H // 2 + 1]; with elites,
    ``randperm(elite_num)`` for the kept ones (trajectory_opt.py:446-448) as ``keep_perm``; in the plan's first iteration
    (``first``: i == 0) the tail-action normal of the shifted elites (:451-457) as ``end_noise`` [keep, A]."""
    F = H // 2 + 1
    draws = {"normals": torch.stack([torch.empty(n, A, F).normal_(0.0, 1.0), torch.empty(n, A, F).normal_(0.0, 1.0)])}
    if has_elite:
        draws["keep_perm"] = torch.randperm(elite_num)
        if first:
            draws["end_noise"] = torch.empty(keep, A).normal_(0.0, 1.0)
    return draws


def elite_indices(values: torch.Tensor, elite_num: int) -> torch.Tensor:
    """The elite indices the reference's optimizers pick on a CPU device (trajectory_opt.py:178-179, 467-470): NaN -> -1e-10, then
    ``torch.topk`` -- whose order among EQUAL values is an artefact of its partial sort.  The 0 / 1 rewards of the cartpole family
    (env/reward_fns.py:10-13, 27-30) tie dozens of candidates at the elite boundary, so a seed-identical replay
    (``sampler='torch'``: it synchronises with the host anyway) has to ask the same routine.  int32 indices."""
    v = values.detach().to("cpu", torch.float32).clone()
    v[v.isnan()] = -1e-10
    return torch.topk(v, int(elite_num)).indices.to(torch.int32)
