"""hipets -- MI355X-native PETS planning / rollout engine behind mbrl-lib's own plugin seams.

Public names follow mbrl-lib so the stock Hydra configs only swap ``_target_``:
``hipets.TrajectoryOptimizerAgent``, ``hipets.CEMOptimizer`` ... or, on a stock agent,
``agent.set_trajectory_eval_fn(hipets.make_eval_fn(model_env, num_particles))``.
"""
from ._lib import ERR_INVALID_ARGUMENT, ERR_NONE, ERR_RUNTIME, ERR_TIMEOUT, HipetsError, LIB_PATH  # noqa: F401
from .model import (  # noqa: F401
    BoxTermination,
    Interval,
    ModelSpec,
    ObsColumn,
    ObsColumns,
    PlaNetSpec,
    RewardTerm,
    RewardTerms,
    UnsupportedModelError,
    model_version,
    spec_from_checkpoint,
    spec_from_model_env,
    spec_from_planet_model,
)
from .engine import Engine  # noqa: F401
from .reduce import ParticleReduce  # noqa: F401
from .planning import (  # noqa: F401
    Agent,
    BatchedCEMAgent,
    BatchedICEMAgent,
    BatchedMPPIAgent,
    CEMOptimizer,
    CallableTrajectoryEvalFn,
    HipTrajectoryEvalFn,
    ICEMOptimizer,
    MPPIOptimizer,
    ModelEnv,
    Optimizer,
    PlaNetTrajectoryEvalFn,
    TrajectoryOptimizer,
    TrajectoryOptimizerAgent,
    UnfusedTrajectoryEvalFn,
    complete_agent_cfg,
    create_trajectory_optim_agent_for_model,
    get_engine,
    make_eval_fn,
)
from .propagation import (  # noqa: F401
    propagate,
    propagate_expectation,
    propagate_fixed_model,
    propagate_from_indices,
    propagate_random_model,
)
from .trainer import ModelTrainer, make_model_trainer  # noqa: F401
from .mbpo import rollout_model_and_populate_sac_buffer  # noqa: F401
from .replay import DeviceReplayBuffer, maybe_replace_sac_buffer  # noqa: F401
from .sac import SACActor, SACCritic, SACUpdater, make_sac_updater  # noqa: F401
from .value import ValueTrajectoryEvalFn  # noqa: F401
from .ensemble import EnsemblePredictor, UncertaintyPenalty  # noqa: F401
from .policy_rollout import PolicyPrior, PolicyRollout  # noqa: F401
from . import dist  # noqa: F401

__version__ = "0.1.0"
