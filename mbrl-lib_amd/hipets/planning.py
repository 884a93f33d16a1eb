"""The import surface of the planning front end: the stock configs and ``_TARGET_ALIASES`` name ``hipets.planning.*``.  The code lives,
by layer, in ``objectives`` (eval functions, ``ModelEnv``), ``optimizers`` (CEM, MPPI, iCEM), ``agents`` (``TrajectoryOptimizer``, the
agents, the config helpers), ``reference_draws`` (the reference's RNG consumption order) and ``engine`` (``get_engine``)."""
from .agents import (Agent, BatchedCEMAgent, BatchedICEMAgent, BatchedMPPIAgent, TrajectoryOptimizer,  # noqa: F401
                     TrajectoryOptimizerAgent, _instantiate, _OptimizerSnapshot, complete_agent_cfg,
                     create_trajectory_optim_agent_for_model)
from .engine import get_engine  # noqa: F401
from .objectives import (CallableTrajectoryEvalFn, HipTrajectoryEvalFn, ModelEnv, PlaNetTrajectoryEvalFn, UnfusedTrajectoryEvalFn, _BoundObjective,  # noqa: F401
                         make_eval_fn)
from .optimizers import CEMOptimizer, ICEMOptimizer, MPPIOptimizer, Optimizer  # noqa: F401
from .reference_draws import population_noise as _reference_noise  # noqa: F401
