"""ctypes binding of libhipets.so (include/hipets.h).  No CPU fallback: if the shared library
or a gfx950 device is missing, engine construction raises -- loudly, never silently."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HIPETS_LIB selects another build of the SAME library (kernel-variant experiments under profiles/); there is no fallback
LIB_PATH = os.environ.get("HIPETS_LIB") or os.path.join(_HERE, "libhipets.so")

ABI_VERSION = 9
MAX_LAYERS = 8

ACT = {"relu": 0, "silu": 1, "leaky_relu": 2, "tanh": 3, "sigmoid": 4}
TRAIN_LOSS = {"nll": 0, "mse": 1}  # HIPETS_TRAIN_LOSS_*
PROP = {"random_model": 0, "fixed_model": 1, "expectation": 2}
OBS = {"none": 0, "halfcheetah": 1, "cartpole_pets": 2, "columns": 3}  # (columns: a hipets.ObsColumns table, HIPETS_OBS_COLUMNS)
REW = {None: 0, "learned": 0, "cartpole": 1, "cartpole_pets": 2, "inverted_pendulum": 3, "halfcheetah": 4, "pusher": 5, "none": 6,
       "terms": 7}  # (terms: a hipets.RewardTerms table, HIPETS_REW_TERMS)
TERM = {"no_termination": 0, "cartpole": 1, "inverted_pendulum": 2, "hopper": 3, "walker2d": 4, "ant": 5, "humanoid": 6,
        "box": 7}  # (box: a hipets.BoxTermination, HIPETS_TERM_BOX)
NORM = {"none": 0, "f32": 1, "f64": 2}
ENSEMBLE = {"gaussian_mlp": 0, "basic_ensemble": 1}
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2}
MODE_EXACT, MODE_FAST, MODE_DEVICE = 0, 1, 2
MODES = {"exact": MODE_EXACT, "fast": MODE_FAST, "device": MODE_DEVICE}
TERM_FN = {"linear": 0, "square": 1, "abs": 2, "sin": 3, "cos": 4, "exp": 5, "sqrt": 6}  # HIPETS_TERM_FN_*
TERM_SRC = {"obs": 0, "act": 1, "group": 2, "const": 3}  # HIPETS_TERM_SRC_*
TERM_OP = {"add": 0, "mul": 1, "div": 2}  # HIPETS_TERM_OP_*
TERM_MAX_LEVEL = 2


def term_word(fn: int, op: int = 0, level: int = 0) -> int:
    """hipets_reward_term.fn (HIPETS_TERM_WORD): fn | op << 8 | level << 16; a bare fn code is level 0, add -- the v9 meaning"""
    return int(fn) | (int(op) << 8) | (int(level) << 16)


def term_word_fields(word: int):
    """(fn, op, level) of a packed word (HIPETS_TERM_WORD_FN / _OP / _LEVEL)"""
    return word & 0xFF, (word >> 8) & 0xFF, (word & 0xFFFFFFFF) >> 16


BOX_LO_OPEN, BOX_HI_OPEN = 1, 2  # hipets_term_interval.flags
MAX_REWARD_TERMS, MAX_TERM_INTERVALS = 64, 64
COL_FN = {"id": 0, "sin": 1, "cos": 2}  # HIPETS_COL_*
MAX_OBS_COLUMNS = 512
KERNEL_CLASSES = ("generic", "hidden_static", "fused", "wide", "bf16")  # HIPETS_KERNEL_*
REDUCE = {"mean": 0, "mean_std": 1, "min": 2, "max": 3, "worst_k": 4}  # HIPETS_REDUCE_*
POLICY_MAX_OBS, POLICY_MAX_HIDDEN, POLICY_MAX_ACT = 512, 1024, 32  # HIPETS_POLICY_MAX_*
TRAIN_MAX_MEMBERS, TRAIN_MAX_HID, TRAIN_MAX_IN, TRAIN_MAX_OUT, TRAIN_MAX_BATCH = 16, 256, 512, 512, 256  # HIPETS_TRAIN_MAX_*
SAC_N_PTRS, SAC_MAX_BATCH = 78, 1024  # HIPETS_SAC_N_PTRS, HIPETS_SAC_MAX_BATCH
CRITIC_N_PTRS = 12  # HIPETS_CRITIC_N_PTRS
ENSEMBLE_MAX_MEMBERS, ENSEMBLE_MAX_IN, ENSEMBLE_MAX_OUT = 16, 512, 512  # HIPETS_ENSEMBLE_MAX_*
ENSEMBLE_STATS = ("max_std", "disagreement", "total_std", "max_deviation")  # columns of hipets_ensemble_predict's stats


class RewardTermC(C.Structure):  # hipets_reward_term
    _fields_ = [("fn", C.c_int32), ("source", C.c_int32), ("i", C.c_int32), ("j", C.c_int32), ("c", C.c_float), ("w", C.c_float)]


class TermIntervalC(C.Structure):  # hipets_term_interval
    _fields_ = [("dim", C.c_int32), ("flags", C.c_int32), ("lo", C.c_float), ("hi", C.c_float)]


class ObsColumnC(C.Structure):  # hipets_obs_column
    _fields_ = [("dim", C.c_int32), ("fn", C.c_int32)]


class ModelDesc(C.Structure):
    _fields_ = [
        ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("in_dim", C.c_int32), ("out_dim", C.c_int32),
        ("hid", C.c_int32), ("n_layers", C.c_int32), ("ensemble_size", C.c_int32), ("n_members", C.c_int32),
        ("members", C.POINTER(C.c_int32)),
        ("activation", C.c_int32), ("leaky_slope", C.c_float), ("propagation", C.c_int32),
        ("deterministic", C.c_int32), ("obs_process", C.c_int32), ("reward_fn", C.c_int32),
        ("termination_fn", C.c_int32), ("target_is_delta", C.c_int32), ("learned_rewards", C.c_int32),
        ("n_no_delta", C.c_int32), ("no_delta", C.POINTER(C.c_int32)),
        ("normalizer", C.c_int32), ("norm_mean", C.POINTER(C.c_double)), ("norm_std", C.POINTER(C.c_double)),
        ("min_logvar", C.POINTER(C.c_float)), ("max_logvar", C.POINTER(C.c_float)),
        ("weights", C.POINTER(C.c_void_p)), ("biases", C.POINTER(C.c_void_p)),
        ("ensemble_kind", C.c_int32),
        ("precision", C.c_int32),
        ("reward_terms", C.POINTER(RewardTermC)), ("term_intervals", C.POINTER(TermIntervalC)),
        ("n_reward_terms", C.c_int32), ("n_term_intervals", C.c_int32),
        ("reward_bias", C.c_float), ("alive_bonus", C.c_float), ("term_require_finite", C.c_int32),
    ]


class RolloutOpts(C.Structure):
    _fields_ = [
        ("mode", C.c_int32),
        ("perms", C.c_void_p), ("eps", C.c_void_p),
        ("seed", C.c_uint64), ("stream_id", C.c_uint64),
        ("member_schedule", C.c_void_p), ("fast_eps", C.c_void_p),
        ("trace_next_obs", C.c_void_p), ("trace_rewards", C.c_void_p),
        ("rows_per_group", C.c_int32),
        ("phase_cycles", C.c_void_p),
        ("no_sample", C.c_int32),
        ("rows_per_member", C.c_int32),
        ("n_env", C.c_int32),
        ("generic_kernel", C.c_int32),
        ("member_schedule_len", C.c_int32),
        ("perm_stream_id", C.c_uint64),
    ]


class CemParams(C.Structure):
    _fields_ = [
        ("population_size", C.c_int32), ("horizon", C.c_int32), ("act_dim", C.c_int32),
        ("num_iterations", C.c_int32), ("elite_num", C.c_int32), ("alpha", C.c_double),
        ("return_mean_elites", C.c_int32), ("clipped_normal", C.c_int32), ("unbiased_var", C.c_int32),
    ]


class IcemParams(C.Structure):
    _fields_ = [
        ("population_size", C.c_int32), ("horizon", C.c_int32), ("act_dim", C.c_int32),
        ("num_iterations", C.c_int32), ("elite_num", C.c_int32), ("keep_elite_size", C.c_int32),
        ("population_size_module", C.c_int32), ("return_mean_elites", C.c_int32), ("alpha", C.c_double),
        ("population_decay_factor", C.c_double), ("colored_noise_exponent", C.c_double),
    ]


class PlanTrace(C.Structure):
    _fields_ = [("populations", C.c_void_p), ("values", C.c_void_p), ("mus", C.c_void_p), ("dispersions", C.c_void_p),
                ("elite_idx", C.c_void_p), ("max_rows", C.c_int32)]


_PLANET_TENSORS = ("w_embed", "b_embed", "w_ih", "b_ih", "w_hh", "b_hh", "w_prior1", "b_prior1", "w_prior2", "b_prior2",
                   "w_rew1", "b_rew1", "w_rew2", "b_rew2", "w_rew3", "b_rew3")


class PlanetDesc(C.Structure):
    _fields_ = [("latent_size", C.c_int32), ("action_size", C.c_int32), ("belief_size", C.c_int32), ("hidden_size", C.c_int32),
                ("min_std", C.c_float)] + [(n, C.c_void_p) for n in _PLANET_TENSORS]


class PlanetOpts(C.Structure):
    _fields_ = [("eps", C.c_void_p), ("seed", C.c_uint64), ("stream_id", C.c_uint64), ("no_sample", C.c_int32),
                ("trace_latent", C.c_void_p), ("trace_belief", C.c_void_p), ("trace_rewards", C.c_void_p), ("phase_cycles", C.c_void_p),
                ("n_env", C.c_int32)]


class TrainDesc(C.Structure):
    _fields_ = [
        ("ensemble_size", C.c_int32), ("n_layers", C.c_int32), ("in_dim", C.c_int32), ("hid", C.c_int32), ("out_dim", C.c_int32),
        ("activation", C.c_int32), ("leaky_slope", C.c_float), ("max_batch", C.c_int32),
        ("weights", C.POINTER(C.c_void_p)), ("biases", C.POINTER(C.c_void_p)),
        ("exp_avg_w", C.POINTER(C.c_void_p)), ("exp_avg_b", C.POINTER(C.c_void_p)),
        ("exp_avg_sq_w", C.POINTER(C.c_void_p)), ("exp_avg_sq_b", C.POINTER(C.c_void_p)),
        ("min_logvar", C.c_void_p), ("max_logvar", C.c_void_p),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
        ("steps_per_launch", C.c_int32),
    ]


_CTYPES = {"": C.c_void_p, "i32": C.c_int32, "i64": C.c_int64, "u64": C.c_uint64, "f32": C.c_float, "f64": C.c_double, "int": C.c_int,
           "ptr": C.c_void_p}


def _sig(params: str, restype=C.c_int):
    """'e p:CemParams* seed:u64 out' -> (restype, [("e", c_void_p), ("p", POINTER(CemParams)), ("seed", c_uint64), ("out", c_void_p)]):
    a bare name is a void* (any pointer to caller-owned memory), 'T*' a pointer to the scalar or struct T"""
    out = []
    for name, _, t in (p.partition(":") for p in params.split()):
        base = _CTYPES[t.rstrip("*")] if t.rstrip("*") in _CTYPES else globals()[t.rstrip("*")]  # (a struct of this module)
        out.append((name, C.POINTER(base) if t.endswith("*") else base))
    return restype, out


# every symbol include/hipets.h declares: name -> (restype, [(parameter name, ctype), ...]), names and order exactly the header's
# (tests/test_abi.py compares them with its prototypes); Engine calls by these names
SYMBOLS = {
    "hipets_abi_version": _sig(""),
    "hipets_last_error": _sig("", C.c_char_p),
    "hipets_last_error_kind": _sig(""),
    "hipets_create": _sig("device:int out:ptr*"),
    "hipets_destroy": _sig("e", None),
    "hipets_set_model": _sig("e desc:ModelDesc* stream"),
    "hipets_set_model_columns": _sig("e desc:ModelDesc* cols:ObsColumnC* n_cols:i32 stream"),
    "hipets_rollout": _sig("e actions s0 pop:i32 horizon:i32 num_particles:i32 opts:RolloutOpts* returns stream"),
    "hipets_step": _sig("e obs actions batch:i32 opts:RolloutOpts* next_obs rewards dones stream"),
    "hipets_trajectory_returns": _sig("e rewards dones pop:i32 horizon:i32 num_particles:i32 returns row_totals first_done stream"),
    "hipets_set_particle_reduce": _sig("e kind:i32 kappa:f32 worst_k:i32"),
    "hipets_particle_reduce": _sig("e totals pop:i32 num_particles:i32 returns stream"),
    "hipets_fast_geometry": _sig("e pop:i32 num_particles:i32 horizon:i32 rows_per_group:i32 n_workgroups:i32* row_tiles:i32*"),
    "hipets_kernel_class": _sig("e pop:i32 num_particles:i32 horizon:i32 mode:i32 rows_per_group:i32 kernel_class:i32* row_tiles:i32*"),
    "hipets_fast_schedule": _sig("e horizon:i32 n_workgroups:i32 seed:u64 stream_id:u64 schedule stream"),
    "hipets_fast_normals": _sig("e horizon:i32 batch:i32 seed:u64 stream_id:u64 normals stream"),
    "hipets_device_perms": _sig("e horizon:i32 batch:i32 seed:u64 stream_id:u64 perms stream"),
    "hipets_set_plan_mode": _sig("e mode:i32"),
    "hipets_set_persistent": _sig("e on:i32"),
    "hipets_set_handover_timeout": _sig("e seconds:f64"),
    "hipets_check_async_error": _sig("e timed_out:i32*"),
    "hipets_set_plan_trace": _sig("e trace:PlanTrace*"),
    "hipets_cem_sample": _sig("e p:CemParams* mu dispersion lower upper z seed:u64 stream_id:u64 population stream"),
    "hipets_cem_refit": _sig("e p:CemParams* values population mu dispersion best_value best_solution elite_idx stream"),
    "hipets_cem_refit_elites": _sig("e p:CemParams* values population elites mu dispersion best_value best_solution stream"),
    "hipets_gather_rows": _sig("e rows:i32 dim:i32 src index dst stream"),
    "hipets_mppi_sample": _sig("e pop:i32 horizon:i32 act_dim:i32 beta:f64 mean past_action lower upper z seed:u64 stream_id:u64 population stream"),
    "hipets_mppi_update": _sig("e pop:i32 horizon:i32 act_dim:i32 gamma:f64 values population mean stream"),
    "hipets_icem_sample": _sig("e n:i32 horizon:i32 act_dim:i32 exponent:f64 mu var lower upper normals seed:u64 stream_id:u64 population stream"),
    "hipets_icem_shift": _sig("e keep:i32 horizon:i32 act_dim:i32 kept mu var end_noise seed:u64 stream_id:u64 out stream"),
    "hipets_plan_cem": _sig("e p:CemParams* x0 lower upper s0 num_particles:i32 seed:u64 plan_id:u64 out stream"),
    "hipets_plan_cem_batched": _sig("e p:CemParams* n_env:i32 x0 lower upper s0 num_particles:i32 seed:u64 plan_id:u64 out stream"),
    "hipets_plan_mppi": _sig("e population_size:i32 horizon:i32 act_dim:i32 num_iterations:i32 gamma:f64 beta:f64 mean lower upper s0 "
                             "num_particles:i32 seed:u64 plan_id:u64 stream"),
    "hipets_plan_mppi_batched": _sig("e population_size:i32 horizon:i32 act_dim:i32 num_iterations:i32 gamma:f64 beta:f64 n_env:i32 mean lower "
                                     "upper s0 num_particles:i32 seed:u64 plan_id:u64 stream"),
    "hipets_plan_icem": _sig("e p:IcemParams* x0 lower upper elite has_elite:i32 keep_idx s0 num_particles:i32 seed:u64 plan_id:u64 out stream"),
    "hipets_plan_icem_batched": _sig("e p:IcemParams* n_env:i32 x0 lower upper elite has_elite:i32 keep_idx s0 num_particles:i32 seed:u64 "
                                     "plan_id:u64 out stream"),
    "hipets_comm_unique_id": _sig("id_out"),
    "hipets_comm_init": _sig("e unique_id rank:i32 world_size:i32"),
    "hipets_comm_destroy": _sig("e"),
    "hipets_comm_info": _sig("e rank:i32* world_size:i32*"),
    "hipets_plan_cem_sharded": _sig("e p:CemParams* x0 lower upper s0 num_particles:i32 seed:u64 plan_id:u64 out stream"),
    "hipets_plan_mppi_sharded": _sig("e population_size:i32 horizon:i32 act_dim:i32 num_iterations:i32 gamma:f64 beta:f64 mean lower upper s0 "
                                     "num_particles:i32 seed:u64 plan_id:u64 stream"),
    "hipets_plan_icem_sharded": _sig("e p:IcemParams* x0 lower upper elite has_elite:i32 keep_idx s0 num_particles:i32 seed:u64 plan_id:u64 "
                                     "out stream"),
    "hipets_planet_set_model": _sig("e d:PlanetDesc* stream"),
    "hipets_planet_rollout": _sig("e actions latent0 belief0 pop:i32 horizon:i32 num_particles:i32 opts:PlanetOpts* returns stream"),
    "hipets_planet_kernel_class": _sig("e is_static:i32*"),
    "hipets_plan_planet_cem": _sig("e p:CemParams* x0 lower upper latent0 belief0 num_particles:i32 seed:u64 plan_id:u64 out stream"),
    "hipets_plan_planet_cem_batched": _sig("e p:CemParams* n_env:i32 x0 lower upper latent0 belief0 num_particles:i32 seed:u64 plan_id:u64 "
                                           "out stream"),
    "hipets_plan_planet_mppi_batched": _sig("e population_size:i32 horizon:i32 act_dim:i32 num_iterations:i32 gamma:f64 beta:f64 n_env:i32 mean "
                                            "lower upper latent0 belief0 num_particles:i32 seed:u64 plan_id:u64 stream"),
    "hipets_plan_planet_icem_batched": _sig("e p:IcemParams* n_env:i32 x0 lower upper elite has_elite:i32 keep_idx latent0 belief0 "
                                            "num_particles:i32 seed:u64 plan_id:u64 out stream"),
    "hipets_train_steps": _sig("e d:TrainDesc* x y n_rows:i64 idx rows n_steps:i32 step0:i64 loss grad_sq stream"),
    "hipets_train_eval": _sig("e d:TrainDesc* x y n_rows:i64 order score row_score stream"),
    "hipets_train_steps_loss": _sig("e d:TrainDesc* x y n_rows:i64 idx rows n_steps:i32 step0:i64 loss grad_sq stream loss_kind:i32 "
                                    "bounds_per_member:i32 grad_scale:f32"),
    "hipets_train_eval_loss": _sig("e d:TrainDesc* x y n_rows:i64 order score row_score stream loss_kind:i32"),
    "hipets_policy_set": _sig("e obs_dim:i32 hidden:i32 act_dim:i32 w1 b1 w2 b2 wm bm ws bs action_scale action_bias stream"),
    "hipets_policy_act": _sig("e obs batch:i32 sample:i32 seed:u64 stream_id:u64 eps actions mean_out log_std_out stream"),
    "hipets_policy_normals": _sig("e batch:i32 act_dim:i32 seed:u64 stream_id:u64 out stream"),
    "hipets_policy_geometry": _sig("e batch:i32 row_tiles:i32* lds_bytes:i32*"),
    "hipets_compact_transitions": _sig("e obs action next_obs rewards dones accum_dones n:i32 obs_dim:i32 act_dim:i32 staging cap:i64 offset "
                                       "count_out stream"),
    "hipets_ring_compact_transitions": _sig("e obs action next_obs rewards dones accum_dones n:i32 obs_dim:i32 act_dim:i32 ring capacity:i64 "
                                            "cursor count_out stream"),
    "hipets_replay_gather": _sig("e ring capacity:i64 obs_dim:i32 act_dim:i32 indices n_rows:i64 reverse_mask:i32 out stream"),
    "hipets_sac_bind": _sig("e obs_dim:i32 act_dim:i32 hidden:i32 tuning:i32 gamma:f64 tau:f64 target_entropy:f64 target_update_interval:i32 "
                            "adam:f64* ptrs n_ptrs:i32"),
    "hipets_sac_update": _sig("e batch batch_size:i32 eps_next eps_cur update_index:i64 step_critic:i64 step_policy:i64 step_alpha:i64 "
                              "lr_critic:f64 lr_policy:f64 lr_alpha:f64 result stream"),
    "hipets_sac_forward_taps": _sig("e batch_size:i32 q1 q2 y log_pi_next log_pi stream"),
    "hipets_critic_set": _sig("e obs_dim:i32 act_dim:i32 hidden:i32 ptrs n_ptrs:i32 stream"),
    "hipets_critic_q": _sig("e obs actions batch:i32 q1 q2 qmin stream"),
    "hipets_critic_geometry": _sig("e batch:i32 row_tiles:i32* lds_bytes:i32*"),
    "hipets_discounted_returns": _sig("e rewards dones terminal_values gamma:f32 pop:i32 horizon:i32 num_particles:i32 returns row_totals "
                                      "first_done stream"),
    "hipets_ensemble_set": _sig("e desc:ModelDesc* cols:ObsColumnC* n_cols:i32 stream"),
    "hipets_ensemble_predict": _sig("e obs actions model_in batch:i32 only_elite:i32 mean logvar stats stream"),
    "hipets_ensemble_geometry": _sig("e batch:i32 row_tiles:i32* lds_bytes:i32*"),
    "hipets_uncertainty_penalty": _sig("e stats stat:i32 coef:f32 halt_threshold:f32 halt_reward:f32 use_halt_reward:i32 batch:i32 rewards dones "
                                       "stream"),
    "hipets_policy_rollout": _sig("e s0 n:i32 horizon:i32 mean_rows:i32 only_elite:i32 seed:u64 stream_id:u64 eps actions states stream"),
    "hipets_policy_rollout_geometry": _sig("e n:i32 row_tiles:i32* lds_bytes:i32*"),
    "hipets_timing_enable": _sig("e on:i32"),
    "hipets_timing_read": _sig("e launches:i64* total_ms:f64* reset:i32"),
}

_lib = None


COMM_ID_BYTES = 128


ERR_NONE, ERR_INVALID_ARGUMENT, ERR_RUNTIME, ERR_TIMEOUT = 0, 1, 2, 3


class HipetsError(RuntimeError):
    """A failed libhipets call.  ``kind`` = hipets_last_error_kind(): ERR_INVALID_ARGUMENT (the library refused the arguments: the
    same on every rank that passed them), ERR_RUNTIME (a HIP / RCCL call, an allocation or a launch failed), ERR_TIMEOUT.  An error
    raised on the Python side without a kind (a missing library, an engine without a model) counts as a runtime failure: only the C
    library's own verdict marks an error as a deterministic rejection of the arguments (hipets.dist.run_sharded relies on that)."""

    def __init__(self, message="", kind: int = ERR_RUNTIME):
        super().__init__(message)
        self.kind = kind


def load():
    """dlopen libhipets.so and bind every declared symbol.  Raises if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipetsError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "hipets has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = [t for _, t in args]
    if lib.hipets_abi_version() != ABI_VERSION:
        raise HipetsError(f"libhipets ABI {lib.hipets_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        lib = load()
        raise HipetsError(lib.hipets_last_error().decode(), lib.hipets_last_error_kind())
