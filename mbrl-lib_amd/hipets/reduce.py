"""``ParticleReduce``: how an objective collapses the ``num_particles`` totals of a candidate into the value the optimizer ranks
(include/hipets.h, hipets_set_particle_reduce; the rule itself is csrc/particle_reduce.hpp).  The reference knows the mean only
(model_env.py:190-191); the other kinds rank by the spread the particles carry -- the model's own uncertainty about the candidate."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Union

from . import _lib

_BY_NAME = {"mean": "mean", "min": "min", "max": "max"}


@dataclass(frozen=True)
class ParticleReduce:
    """``kind``: 'mean' (default), 'mean_std' (mean - ``kappa`` * std; ``kappa`` > 0 risk-averse, < 0 optimistic), 'min', 'max',
    'worst_k' (the mean of the ``worst_k`` lowest totals) or 'cvar' (worst_k with k = ceil(``alpha`` * num_particles), resolved by
    the objective with its own particle count).  Build one with the constructors below; a bad argument raises ValueError."""

    kind: str = "mean"
    kappa: float = 0.0
    worst_k: int = 0
    alpha: float = 0.0

    def __post_init__(self):
        if self.kind not in _lib.REDUCE and self.kind != "cvar":
            raise ValueError(f"particle reduction kind must be one of {sorted(_lib.REDUCE) + ['cvar']}, got {self.kind!r}")
        if not isinstance(self.kappa, (int, float)) or not math.isfinite(self.kappa):
            raise ValueError(f"kappa must be a finite number, got {self.kappa!r}")
        if self.kind == "worst_k" and (not isinstance(self.worst_k, int) or isinstance(self.worst_k, bool) or self.worst_k < 1):
            raise ValueError(f"worst_k must be an integer >= 1, got {self.worst_k!r}")
        if self.kind == "cvar" and not (isinstance(self.alpha, (int, float)) and 0.0 < self.alpha <= 1.0):
            raise ValueError(f"cvar alpha must lie in (0, 1], got {self.alpha!r}")

    @classmethod
    def mean(cls) -> "ParticleReduce":
        return cls("mean")

    @classmethod
    def mean_std(cls, kappa: float) -> "ParticleReduce":
        return cls("mean_std", kappa=kappa)

    @classmethod
    def worst_case(cls) -> "ParticleReduce":
        return cls("min")

    @classmethod
    def best_case(cls) -> "ParticleReduce":
        return cls("max")

    @classmethod
    def cvar(cls, alpha: float) -> "ParticleReduce":
        return cls("cvar", alpha=alpha)

    @classmethod
    def coerce(cls, value: Union["ParticleReduce", str, None]) -> "ParticleReduce":
        """The ``particle_reduce=`` keyword of the objectives: a ParticleReduce, or 'mean' / 'min' / 'max'; None is the mean."""
        if value is None:
            return cls("mean")
        if isinstance(value, cls):
            return value
        if isinstance(value, str) and value in _BY_NAME:
            return cls(_BY_NAME[value])
        raise ValueError(f"particle_reduce must be a hipets.ParticleReduce or one of 'mean', 'min', 'max', got {value!r}")

    def resolve(self, num_particles: int) -> "ParticleReduce":
        """What the engine is told for an objective of ``num_particles`` particles: cvar(alpha) becomes worst_k(k) with
        k = max(1, ceil(round(alpha * P, 9))) (alpha 0.2, P 20 -> 4; alpha 1.0 -> P); every other kind is itself."""
        if self.kind != "cvar":
            return self
        return ParticleReduce("worst_k", worst_k=max(1, math.ceil(round(self.alpha * int(num_particles), 9))))

    def abi_args(self) -> dict:
        """kind / kappa / worst_k of hipets_set_particle_reduce (a resolved reduction: no 'cvar')"""
        return {"kind": _lib.REDUCE[self.kind], "kappa": float(self.kappa), "worst_k": int(self.worst_k)}


def _worst_k(cls, k: int) -> ParticleReduce:
    """The mean of the ``k`` lowest particle totals (1 <= k <= num_particles <= 256); k = num_particles is the mean."""
    return cls("worst_k", worst_k=k)


# The constructor shares its name with the field: it is attached once the dataclass has read the field's default (0) off the class.
# Instances keep their own ``worst_k`` (the field); ``ParticleReduce.worst_k(k)`` on the class is the constructor.
ParticleReduce.worst_k = classmethod(_worst_k)
