/*
 * hipets.h -- C ABI of libhipets.so, the MI355X (gfx950) PETS planning / rollout engine.
 *
 * Drop-in boundary for ONE hot path of facebookresearch/mbrl-lib (v0.2.0):
 *
 *   TrajectoryOptimizerAgent.act -> {CEM,iCEM,MPPI}Optimizer.optimize
 *       -> ModelEnv.evaluate_action_sequences -> GaussianMLP ensemble -> reward/termination
 *
 * The reference is pure Python/PyTorch, so "the reference's FFI for this path" is a ctypes
 * binding; every entry point below names the reference interface it replaces
 * (file:line relative to the reference root).  Plain pointers and sizes only, no torch types.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; hipets_last_error() gives the
 *     thread-local message.  Nothing throws across the ABI.
 *   - pointers marked DEVICE point into caller-owned HBM (e.g. torch storage); pointers marked
 *     HOST are read during the call only.  The library retains no caller pointer past a call,
 *     except hipets_set_model which copies weights into its own packed layout.
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); all work is enqueued asynchronously on it.
 *     An engine's workspace is shared by its calls, so their work executes in call order: a call on another stream than the
 *     previous call's makes its stream wait (device side) for that call's work.  The launch-only helpers take no part in that
 *     ordering, because they use no workspace: each launches on `stream` a kernel that touches the caller's buffers alone, waits
 *     for no other call and is waited for by none, so the caller orders them as it orders its own kernels.  They are
 *     hipets_cem_sample, hipets_cem_refit, hipets_cem_refit_elites, hipets_gather_rows, hipets_mppi_sample, hipets_mppi_update,
 *     hipets_icem_sample, hipets_icem_shift, hipets_particle_reduce, hipets_fast_schedule, hipets_fast_normals,
 *     hipets_device_perms and hipets_policy_normals.  Four entry points take part in the ordering and also synchronise `stream`
 *     before returning, because they read caller-owned DEVICE tensors and HOST staging that may be freed right after the call:
 *     hipets_set_model, hipets_set_model_columns, hipets_planet_set_model and hipets_ensemble_set.  hipets_timing_read waits for
 *     the events it reports; the one-time co-residency self-test of a persistent DEVICE-mode kernel instance synchronises once
 *     (hipets_set_persistent); hipets_sac_bind makes one blocking 16-byte copy.  Nothing else synchronises.
 *   - HOST arrays are consumed before the call returns, so temporaries are fine: observations are copied into
 *     pinned staging buffers owned by the engine and uploaded asynchronously from there; model descriptors are
 *     uploaded inside hipets_set_model, which synchronises.
 *   - one engine per device; an engine is not thread-safe (the reference is single-threaded).  Engines of DIFFERENT devices may
 *     be driven from different host threads (the library's per-device residency table is locked).
 */
#ifndef HIPETS_H
#define HIPETS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPETS_ABI_VERSION 9
#define HIPETS_MAX_LAYERS 8
#define HIPETS_MAX_REWARD_TERMS 64   /* entries of a reward term table (HIPETS_REW_TERMS)  */
#define HIPETS_MAX_TERM_INTERVALS 64 /* interval tests of a healthy box (HIPETS_TERM_BOX)     */
#define HIPETS_MAX_OBS_COLUMNS 512   /* columns of an observation column table (HIPETS_OBS_COLUMNS) */

typedef struct hipets_engine hipets_engine;

/* activation module of GaussianMLP (mbrl/models/gaussian_mlp.py:88-96) */
enum { HIPETS_ACT_RELU = 0, HIPETS_ACT_SILU = 1, HIPETS_ACT_LEAKY_RELU = 2, HIPETS_ACT_TANH = 3, HIPETS_ACT_SIGMOID = 4 };
/* Ensemble.propagation_method (mbrl/models/gaussian_mlp.py:201-216) */
enum { HIPETS_PROP_RANDOM_MODEL = 0, HIPETS_PROP_FIXED_MODEL = 1, HIPETS_PROP_EXPECTATION = 2 };
/* obs_process_fn (mbrl/env/pets_halfcheetah.py:91-113, mbrl/env/pets_cartpole.py:78-101) */
enum { HIPETS_OBS_NONE = 0, HIPETS_OBS_HALFCHEETAH = 1, HIPETS_OBS_CARTPOLE_PETS = 2,
       HIPETS_OBS_COLUMNS = 3 /* the model's own column table (hipets_obs_column below, hipets_set_model_columns) */ };
/* reward_fn (mbrl/env/reward_fns.py:10-53); LEARNED = last model output (model_env.py:124-128) */
enum { HIPETS_REW_LEARNED = 0, HIPETS_REW_CARTPOLE = 1, HIPETS_REW_CARTPOLE_PETS = 2, HIPETS_REW_INVERTED_PENDULUM = 3,
       HIPETS_REW_HALFCHEETAH = 4, HIPETS_REW_PUSHER = 5,
       HIPETS_REW_NONE = 6, /* rewards are computed by the caller (arbitrary Python reward_fn on hipets_step's next_obs) */
       HIPETS_REW_TERMS = 7 /* ABI v9: the model's own term table (hipets_reward_term below), no mbrl.env counterpart   */ };
/* termination_fn (mbrl/env/termination_fns.py:12-95) */
enum { HIPETS_TERM_NONE = 0, HIPETS_TERM_CARTPOLE = 1, HIPETS_TERM_INVERTED_PENDULUM = 2, HIPETS_TERM_HOPPER = 3,
       HIPETS_TERM_WALKER2D = 4, HIPETS_TERM_ANT = 5, HIPETS_TERM_HUMANOID = 6,
       HIPETS_TERM_BOX = 7 /* ABI v9: the model's own healthy box (hipets_term_interval below) */ };
/* Normalizer dtype (mbrl/util/math.py:108-111; normalize_double_precision, one_dim_tr_model.py:87-92) */
enum { HIPETS_NORM_NONE = 0, HIPETS_NORM_F32 = 1, HIPETS_NORM_F64 = 2 };
/* Ensemble container: GAUSSIAN_MLP = one GaussianMLP with E members: balanced random shuffles and the batch % members
 * check (mbrl/models/gaussian_mlp.py:179-216); BASIC_ENSEMBLE = mbrl.models.BasicEnsemble of E single-member
 * GaussianMLPs (conf/dynamics_model/basic_ensemble.yaml): every row draws its member independently
 * (basic_ensemble.py:122-129, 255-260), any batch size, no elites (:262-266), per-member logvar bounds. */
enum { HIPETS_ENSEMBLE_GAUSSIAN_MLP = 0, HIPETS_ENSEMBLE_BASIC = 1 };
/* arithmetic of the ensemble MLP's linear layers */
enum { HIPETS_PREC_F32 = 0,    /* v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulate (the graded mode)              */
       HIPETS_PREC_BF16X3 = 1, /* fp32 operands carried as three bf16 pieces, six exact partial products per product     */
                               /* on v_mfma_f32_16x16x32_bf16, fp32 accumulate: fp32-accurate to a few product ulps      */
                               /* (|error| <= 2^-22 |a||b| per product), reported SEPARATELY from the fp32-MFMA mode     */
       HIPETS_PREC_BF16 = 2    /* reduced precision, reported SEPARATELY with its own parity tolerance: for every linear  */
                               /* layer both operands are rounded to bf16 (round-to-nearest-even), products are exact,   */
                               /* accumulation is fp32 on v_mfma_f32_16x16x32_bf16 (ONE MFMA per 16x16x32 block), bias   */
                               /* is added in fp32, SiLU is computed in fp32.  A hidden layer's activated result is     */
                               /* stored as one bf16 per value: that store is the rounding of the next layer's operand; */
                               /* the output layer's results stay fp32.  Everything outside the linear layers (f64      */
                               /* normaliser, logvar clamps, sampling, delta add, reward / termination, totals, the     */
                               /* fp32 state and its hand-over, Philox streams and permutations) is the fp32 mode's.    */ };
/* randomness source of a rollout */
enum { HIPETS_MODE_EXACT = 0,  /* reference semantics, injected perms / eps (parity mode)                              */
       HIPETS_MODE_FAST = 1,   /* whole-horizon kernel, block-balanced member schedule, in-kernel Philox             */
       HIPETS_MODE_DEVICE = 2  /* reference semantics (ONE balanced permutation of all B rows per step,              */
                               /* gaussian_mlp.py:203-205; iid eps per row and dim, model.py:471-473) with both      */
                               /* drawn in-kernel from (seed, stream_id): a keyed bijection of [0, B) and Philox     */
                               /* normals.  No input tensors; exportable through hipets_device_perms /              */
                               /* hipets_fast_normals for replay through a reference implementation.                 */ };

/* ---- parametric closed forms (ABI v9): rewards and terminations of environments mbrl.env does not ship ----------------
 * Both are defined op by op in fp32 (no fused multiply-add), on the step's next_obs s' and its action a:
 *
 * HIPETS_REW_TERMS   r = reward_bias + sum_k w_k * f_k(e_k)  [+ alive_bonus * (done ? 0 : 1)]
 *     accumulated in table order starting from reward_bias; e_k = v[i_k] - (j_k >= 0 ? v[j_k] : c_k) with v = s' (source
 *     OBS) or a (source ACT); f = identity, square or absolute value.  The alive bonus is added last, and only when it is
 *     non-zero; `done` is the model's own termination test on the same s' (reward_fns.cartpole: (~termination_fn).float()).
 *     NaN and inf propagate as IEEE arithmetic does.
 * HIPETS_TERM_BOX    healthy = every interval test holds (lo < or <= s'[dim] < or <= hi, each bound open or closed by its
 *     flag, +-inf allowed; a NaN fails every test) and, with term_require_finite, all obs_dim dims of s' are finite;
 *     done = !healthy.  Restates termination_fns.cartpole / inverted_pendulum / hopper / walker2d / ant exactly, and
 *     humanoid on finite rows only (the reference's humanoid leaves a NaN row alive; a box ends it).
 * The parametric forms run on the GENERIC and HIDDEN_STATIC kernel instances (hipets_kernel_class): a model that uses one
 * has no shape-specialised instance, and is therefore refused under HIPETS_PREC_BF16X3 / HIPETS_PREC_BF16.
 *
 * Grouped terms (additive to ABI v9: no struct changed, a v9 table means what it meant).  The table is a small expression form
 * over three accumulators: A0 starts at reward_bias, A1 and A2 at 0.  Entries run in table order, op by op in fp32:
 *     e = v[i] - (j >= 0 ? v[j] : c)          source OBS (v = s') or ACT (v = a)
 *     e = c                                   source CONST
 *     e = A[level + 1] - c;  A[level + 1] = 0 source GROUP: consumes the finished deeper group (level 0 or 1 only)
 *     t = w * f(e)                            f: linear | square | abs | sinf | cosf | expf | sqrtf
 *     A[level] = A[level] + t | A[level] * t | A[level] / t          op: ADD | MUL | DIV
 *     r = A0, then the alive bonus as above.  sqrt of a negative is NaN, x / 0 is +-inf; NaN and inf propagate.
 * `level` and `op` travel in the upper bits of hipets_reward_term.fn, which a v9 client leaves zero (level 0, ADD):
 * HIPETS_TERM_WORD below.  A table is well formed, and hipets_set_model refuses it otherwise naming the entry, when level is in
 * 0..2, GROUP is not at level 2 and does not consume an empty group (no entry since its last consumption or the table start),
 * MUL / DIV do not go into an empty group at level 1 or 2, no group is left open at the end of the table, and GROUP / CONST
 * entries have j < 0.  i and j of a GROUP / CONST entry are not read.                                                       */
enum { HIPETS_TERM_FN_LINEAR = 0, HIPETS_TERM_FN_SQUARE = 1, HIPETS_TERM_FN_ABS = 2,
       HIPETS_TERM_FN_SIN = 3, HIPETS_TERM_FN_COS = 4, HIPETS_TERM_FN_EXP = 5, HIPETS_TERM_FN_SQRT = 6 };
enum { HIPETS_TERM_SRC_OBS = 0, HIPETS_TERM_SRC_ACT = 1, HIPETS_TERM_SRC_GROUP = 2, HIPETS_TERM_SRC_CONST = 3 };
enum { HIPETS_TERM_OP_ADD = 0, HIPETS_TERM_OP_MUL = 1, HIPETS_TERM_OP_DIV = 2 };
#define HIPETS_TERM_MAX_LEVEL 2
/* hipets_reward_term.fn: fn | op << 8 | level << 16 (bits 24..31 zero) */
#define HIPETS_TERM_WORD(fn, op, level) ((int32_t)((fn) | ((op) << 8) | ((level) << 16)))
#define HIPETS_TERM_WORD_FN(word) ((int32_t)((word) & 0xff))
#define HIPETS_TERM_WORD_OP(word) ((int32_t)(((word) >> 8) & 0xff))
#define HIPETS_TERM_WORD_LEVEL(word) ((int32_t)(((uint32_t)(word)) >> 16))
enum { HIPETS_BOX_LO_OPEN = 1, HIPETS_BOX_HI_OPEN = 2 }; /* hipets_term_interval.flags: the bound is strict (0 = closed) */
typedef struct {
    int32_t fn;     /* HIPETS_TERM_WORD(HIPETS_TERM_FN_*, HIPETS_TERM_OP_*, level); a bare HIPETS_TERM_FN_* = level 0, ADD */
    int32_t source; /* HIPETS_TERM_SRC_*: the vector i and j index, the deeper group, or the constant c */
    int32_t i;      /* dim of the minuend                                                */
    int32_t j;      /* dim of the subtrahend, or < 0: the constant c                     */
    float c;
    float w;        /* weight of the term                                                */
} hipets_reward_term;
typedef struct {
    int32_t dim;    /* observation dim                                                   */
    int32_t flags;  /* HIPETS_BOX_LO_OPEN | HIPETS_BOX_HI_OPEN                           */
    float lo;       /* lo <= hi; -INFINITY / INFINITY = no bound on that side            */
    float hi;
} hipets_term_interval;

/* ---- parametric observation preprocessing: obs_process_fn of environments mbrl.env does not ship -----------------------
 * HIPETS_OBS_COLUMNS   column k of obs_process_fn(obs) is fn_k(obs[dim_k]), fn = identity, sinf or cosf in fp32 -- the form of both
 *     shipped preprocessors (halfcheetah: [s1, sin s2, cos s2, s3:]; cartpole_pets: [sin s1, cos s1, s0, s2:]) and of any
 *     environment that feeds joint angles to its model as sin / cos.  A dim may enter several columns, in any order, or none; the
 *     table has in_dim - act_dim entries, whatever obs_dim is.  NaN and inf propagate as sinf / cosf do (sin(inf) = NaN).
 * Runs on the GENERIC and HIDDEN_STATIC kernel instances, like the parametric forms above, and is refused under
 * HIPETS_PREC_BF16X3 / HIPETS_PREC_BF16 likewise.                                                                         */
enum { HIPETS_COL_ID = 0, HIPETS_COL_SIN = 1, HIPETS_COL_COS = 2 };
typedef struct {
    int32_t dim; /* observation dim the column reads                                  */
    int32_t fn;  /* HIPETS_COL_*                                                      */
} hipets_obs_column;

/*
 * Snapshot of what ModelEnv.evaluate_action_sequences reads from the live objects
 * (OneDTransitionRewardModel mbrl/models/one_dim_tr_model.py:29-116, GaussianMLP
 * mbrl/models/gaussian_mlp.py:69-127, EnsembleLinearLayer mbrl/models/util.py:31-65).
 */
typedef struct {
    int32_t obs_dim;         /* raw observation width                                             */
    int32_t act_dim;         /* action width                                                      */
    int32_t in_dim;          /* model input width = width(obs_process_fn(obs)) + act_dim          */
    int32_t out_dim;         /* model output width = obs_dim + learned_rewards                    */
    int32_t hid;             /* hidden width                                                      */
    int32_t n_layers;        /* number of linear layers = hidden layers + 1 (<= HIPETS_MAX_LAYERS) */
    int32_t ensemble_size;   /* E: leading dim of every weight tensor                             */
    int32_t n_members;       /* M: number of ACTIVE members (elite set, gaussian_mlp.py:161-163)  */
    const int32_t* members;  /* HOST [M] indices into E                                           */
    int32_t activation;      /* HIPETS_ACT_*                                                      */
    float leaky_slope;       /* negative slope for LEAKY_RELU                                     */
    int32_t propagation;     /* HIPETS_PROP_*                                                     */
    int32_t deterministic;   /* model has no logvar head (gaussian_mlp.py:113-114)                */
    int32_t obs_process;     /* HIPETS_OBS_*                                                      */
    int32_t reward_fn;       /* HIPETS_REW_*                                                      */
    int32_t termination_fn;  /* HIPETS_TERM_*                                                     */
    int32_t target_is_delta; /* one_dim_tr_model.py:281-286                                       */
    int32_t learned_rewards;
    int32_t n_no_delta;
    const int32_t* no_delta; /* HOST [n_no_delta] observation dims predicted absolutely           */
    int32_t normalizer;      /* HIPETS_NORM_*                                                     */
    const double* norm_mean; /* HOST [in_dim] (f32 stats widened exactly; arithmetic stays f32)   */
    const double* norm_std;  /* HOST [in_dim]                                                     */
    const float* min_logvar; /* HOST [out_dim] ([M,out_dim] for BASIC_ENSEMBLE: every member owns */
    const float* max_logvar; /*   its bounds) or NULL if deterministic                            */
    const void* const* weights; /* HOST array [n_layers] of DEVICE float [E, in_l, out_l]         */
    const void* const* biases;  /* HOST array [n_layers] of DEVICE float [E, 1, out_l]            */
    int32_t ensemble_kind;   /* HIPETS_ENSEMBLE_*                                                 */
    int32_t precision;       /* HIPETS_PREC_*: BF16X3 / BF16 run only where a shape-specialised kernel instance */
                             /*   exists for the model and the call (else the rollout call fails)           */
    /* ABI v9: the tables of the parametric closed forms above.  A zeroed tail = none (reward_fn / termination_fn then  */
    /* must not ask for them); present exactly when the enum does.  Copied into engine-owned device memory.            */
    const hipets_reward_term* reward_terms;     /* HOST [n_reward_terms] for HIPETS_REW_TERMS, else NULL                */
    const hipets_term_interval* term_intervals; /* HOST [n_term_intervals] for HIPETS_TERM_BOX, else NULL               */
    int32_t n_reward_terms;    /* 0 .. HIPETS_MAX_REWARD_TERMS (0 with HIPETS_REW_TERMS: bias and alive bonus only)     */
    int32_t n_term_intervals;  /* 0 .. HIPETS_MAX_TERM_INTERVALS (0 with HIPETS_TERM_BOX: the finite test only)         */
    float reward_bias;         /* HIPETS_REW_TERMS: the sum starts here                                                 */
    float alive_bonus;         /* HIPETS_REW_TERMS: != 0 needs a termination_fn other than HIPETS_TERM_NONE             */
    int32_t term_require_finite; /* HIPETS_TERM_BOX: every observation dim must be finite                               */
} hipets_model_desc;

/* options of one evaluate_action_sequences call */
typedef struct {
    int32_t mode;            /* HIPETS_MODE_*                                                     */
    /* EXACT mode: the reference's random draws, injected                */
    const int64_t* perms;    /* DEVICE: random_model [H,B] (one torch.randperm(B) per step,       */
                             /*   gaussian_mlp.py:205); fixed_model [B] (:375); else NULL         */
    const float* eps;        /* DEVICE [H,B,out_dim] standard normals consumed by torch.normal    */
                             /*   (model.py:471-473); NULL => predictions are the mean            */
    /* FAST and DEVICE modes: counter-based RNG                                                   */
    uint64_t seed;
    uint64_t stream_id;      /* e.g. plan counter * iterations + iteration                        */
    const int32_t* member_schedule; /* DEVICE [H, n_workgroups] optional override of the FAST-mode */
                             /*   member draws (testing; TS-infinity ModelEnv.step); see member_schedule_len */
    const float* fast_eps;   /* DEVICE [H,B,out_dim] optional override of the Philox normals      */
    /* optional debug taps (DEVICE, may be NULL)                                                  */
    float* trace_next_obs;   /* [H,B,obs_dim]                                                     */
    float* trace_rewards;    /* [H,B] reward of the step before termination masking               */
    int32_t rows_per_group;  /* 0 = auto; else force R (row tiles of 16 per workgroup)            */
    int64_t* phase_cycles;   /* DEVICE [8,16] optional: per-wave, per-phase shader-cycle counters of     */
                             /*   workgroup 0, accumulated (profiling aid): cycles in the  */
                             /*   low 44 bits of an entry, the number of marks that fed it above them    */
    int32_t no_sample;       /* FAST: predictions are the mean (no eps), like ModelEnv.step(sample=False) */
    int32_t rows_per_member; /* EXACT, > 0: explicit per-row member maps.  perms is [H, M*rows_per_member]             */
                             /*   ([M*rows_per_member] for fixed_model): slot m*rows_per_member + j = j-th row of        */
                             /*   member m, -1 = padding (members may own unequal row counts).  Required for            */
                             /*   BASIC_ENSEMBLE (randint maps, basic_ensemble.py:122-129); for GAUSSIAN_MLP it          */
                             /*   expresses mbrl.util.math.propagate_from_indices (util/math.py:180-196): any            */
                             /*   row -> member assignment, no batch % members rule                                      */
    int32_t n_env;           /* FAST / DEVICE batched planning: the pop candidates are n_env groups of */
                             /*   pop / n_env, group g starts from s0[g] (s0 is then HOST [n_env, obs_dim]); 0/1 = one.     */
                             /*   DEVICE: ONE balanced permutation per step over the rows of all environments               */
    int32_t generic_kernel;  /* 1 = only the fully generic kernel instance.  (The library also instantiates the rollout     */
                             /*   kernel (a) for hidden widths of 193..208 -- the reference's default 200 -- with the hidden  */
                             /*   layers' shape as a compile-time fact and everything else generic, and (b) for the BASELINE */
                             /*   shapes with all layer shapes / reward / termination fns as compile-time facts; same        */
                             /*   arithmetic -- tests compare them bit for bit.)  2 = (a) allowed, (b) not                   */
    /* ABI v6 */
    int32_t member_schedule_len; /* entries of member_schedule (horizon x n_workgroups of hipets_fast_geometry); 0 = not stated.  */
                             /*   A stated length that does not match the call's geometry fails the call instead of reading   */
                             /*   the schedule with another stride (the geometry of FAST calls changed in ABI v5 -> v6)       */
    uint64_t perm_stream_id; /* hipets_step, DEVICE mode, fixed_model propagation: stream of the TS-infinity permutation (the     */
                             /*   stream of the rollout's reset: model.py:404-407) while stream_id -- the step's -- keys the eps; */
                             /*   0 = stream_id                                                                                   */
} hipets_rollout_opts;

/* ---- lifecycle -------------------------------------------------------------------------- */
int hipets_abi_version(void);
const char* hipets_last_error(void);
/* Class of this thread's last failure, for callers that must tell "the arguments were refused" (deterministic: every rank of
 * a sharded job that passed the same arguments got the same answer) from "the machine failed" (may have hit one rank only):  */
#define HIPETS_ERR_NONE 0
#define HIPETS_ERR_INVALID_ARGUMENT 1 /* a value, shape or configuration the library rejects                                */
#define HIPETS_ERR_RUNTIME 2          /* a HIP or RCCL call, an allocation or a kernel launch failed                         */
#define HIPETS_ERR_TIMEOUT 3          /* a persistent DEVICE-mode rollout gave up waiting for another workgroup's rows       */
int hipets_last_error_kind(void);
int hipets_create(int device, hipets_engine** out);
void hipets_destroy(hipets_engine* e);

/* Re-snapshot weights / normaliser / elite set (call after ModelTrainer.train,
 * mbrl/models/model_trainer.py:288-296).  Packs into the MFMA fragment layout. */
int hipets_set_model(hipets_engine* e, const hipets_model_desc* desc, void* stream);
/* hipets_set_model for a model whose obs_process is HIPETS_OBS_COLUMNS: column k of obs_process_fn(obs) is fn_k(obs[dim_k]);
 * desc->in_dim must equal n_cols + act_dim (1 <= n_cols <= HIPETS_MAX_OBS_COLUMNS).  cols is HOST memory, copied.  (An entry point
 * of its own, not a field of hipets_model_desc: the descriptor's layout and HIPETS_ABI_VERSION stay what they were; plain
 * hipets_set_model refuses HIPETS_OBS_COLUMNS.)                                                                               */
int hipets_set_model_columns(hipets_engine* e, const hipets_model_desc* desc, const hipets_obs_column* cols, int32_t n_cols, void* stream);

/* ---- ModelEnv.evaluate_action_sequences (mbrl/models/model_env.py:145-191) ---------------- */
/* actions DEVICE [pop,H,A] f32; s0 HOST [obs_dim] f32; returns DEVICE [pop] f32.              */
int hipets_rollout(hipets_engine* e, const float* actions, const float* s0, int32_t pop, int32_t horizon,
                   int32_t num_particles, const hipets_rollout_opts* opts, float* returns, void* stream);
/* ---- ModelEnv.step (mbrl/models/model_env.py:87-140; MBPO-style one-step model rollouts) ---
 * One transition for B independent rows: obs DEVICE [B,obs_dim], actions DEVICE [B,act_dim] ->
 * next_obs DEVICE [B,obs_dim], rewards DEVICE [B] f32, dones DEVICE [B] uint8.  opts as for hipets_rollout with
 * horizon 1 and one particle per row: EXACT takes perms [B] (one torch.randperm, or the fixed_model indices) and eps
 * [1,B,out_dim] (NULL => the deterministic mean, i.e. ModelEnv.step(sample=False)); DEVICE (the reference's per-row balanced
 * shuffle, gaussian_mlp.py:203-205) and FAST (one member per workgroup of 16 R consecutive rows) draw both in-kernel from
 * (seed, stream_id); set opts->no_sample for the deterministic mean.  DEVICE + fixed_model: see opts->perm_stream_id.          */
int hipets_step(hipets_engine* e, const float* obs, const float* actions, int32_t batch, const hipets_rollout_opts* opts,
                float* next_obs, float* rewards, uint8_t* dones, void* stream);

/* ---- model_env.py:186-191 over a finished trajectory: masked returns for rewards / terminations evaluated outside the kernel ----
 * For rollouts whose reward_fn / termination_fn are the caller's own code: run hipets_rollout once with opts->trace_next_obs (and
 * trace_rewards), evaluate the callables over all H * B traced rows, and reduce here.  rewards DEVICE [H,B] f32 and dones DEVICE [H,B]
 * uint8 (non-zero = the row terminates at that step), B = pop * num_particles, row c * num_particles + p = particle p of candidate c.
 * Per row, for t = 0 .. H-1 in order:  r = terminated ? 0 : rewards[t][row];  terminated |= dones[t][row] != 0;  total += r  -- the
 * zeroing is a select (the reference assigns rewards[terminated] = 0): a NaN or inf reward after termination adds exactly 0, one before
 * it propagates, and the reward of the terminating step itself counts.  returns DEVICE [pop] = the mean of a candidate's
 * num_particles row totals, the same sequential f32 sum and division as hipets_rollout's own (bit-identical to it on the same
 * rewards) -- or the engine's other reduction over the particles (hipets_set_particle_reduce below).  Optional outputs (NULL = not wanted): row_totals DEVICE [B] f32; first_done DEVICE [B] int32 = the first step with
 * dones != 0, horizon if none.  Needs no model.  (An entry point of its own: no struct changes, HIPETS_ABI_VERSION stays.)          */
int hipets_trajectory_returns(hipets_engine* e, const float* rewards, const uint8_t* dones, int32_t pop, int32_t horizon,
                              int32_t num_particles, float* returns, float* row_totals, int32_t* first_done, void* stream);

/* ---- the reduction over a candidate's particles (risk-aware planning) ----
 * A candidate is rolled out as num_particles rows (row c * P + p = particle p of candidate c); its value is ONE rule over the P row
 * totals t[0..P), fp32 op by op, the same in every entry point that reduces particles -- hipets_rollout, hipets_planet_rollout,
 * hipets_trajectory_returns, hipets_particle_reduce and every hipets_plan_* (batched, sharded and PlaNet plans included):
 *   MEAN      s = 0; for p: s += t[p]; v = s / P                        (model_env.py:190-191; the state of a new engine)
 *   MEAN_STD  m as MEAN; q = 0; for p: q += (t[p] - m)^2; v = m - kappa * sqrtf(q / P)   (kappa > 0 risk-averse, < 0 optimistic)
 *   MIN, MAX  the lowest / highest total; NaN if any total is NaN
 *   WORST_K   the mean of the worst_k lowest totals (CVaR): NaN if any total is NaN; else the totals are ranked ascending, ties to the
 *             lower particle, those of rank < worst_k summed in particle order, / worst_k.  worst_k = P gives MEAN's bits.
 *             Needs 1 <= worst_k <= P <= 256.
 * The optimizers' NaN filter, best values, MPPI's weights and the plan traces all see the reduced value.                        */
enum { HIPETS_REDUCE_MEAN = 0, HIPETS_REDUCE_MEAN_STD = 1, HIPETS_REDUCE_MIN = 2, HIPETS_REDUCE_MAX = 3, HIPETS_REDUCE_WORST_K = 4 };
/* Engine state, like hipets_set_plan_mode; host only.  kappa is read for MEAN_STD (finite), worst_k for WORST_K (>= 1; checked against
 * num_particles by the call that knows it: worst_k > num_particles or num_particles > 256 fail there).  Anything else fails with
 * HIPETS_ERR_INVALID_ARGUMENT and leaves the engine's reduction as it was.                                                      */
int hipets_set_particle_reduce(hipets_engine* e, int32_t kind, float kappa, int32_t worst_k);
/* totals DEVICE f32 [pop * num_particles] -> returns DEVICE f32 [pop] under the engine's reduction.  Needs no model.           */
int hipets_particle_reduce(hipets_engine* e, const float* totals, int32_t pop, int32_t num_particles, float* returns, void* stream);

/* geometry the FAST kernel will use for (pop, P): workgroups and rows per group (for member_schedule).  rows_per_group 0: the
 * library's own choice for a DEFAULT call (hipets_rollout without injected eps / traces, the fused plans); > 0: forced.
 * rows_per_group -1: the choice for calls that run the general kernel layout whatever the model -- hipets_step, rollouts with
 * injected eps or traces.  The two differ only for models with a wide-output shape-specialised instance (Humanoid-v4's 376 obs
 * dims: two row tiles per workgroup there, one in the general layout); a call of the second kind that brings its own
 * member_schedule on such a model must size it with -1 and pass the reported row-tile count as opts->rows_per_group.        */
int hipets_fast_geometry(hipets_engine* e, int32_t pop, int32_t num_particles, int32_t horizon, int32_t rows_per_group,
                         int32_t* n_workgroups, int32_t* row_tiles);

/* Which instance of the rollout kernel a DEFAULT call (hipets_rollout / the fused plans with in-kernel randomness, no injected
 * eps, no traces) of this size runs on the engine's model, and with how many row tiles per workgroup.  mode: HIPETS_MODE_FAST or
 * HIPETS_MODE_DEVICE.  rows_per_group: 0 = the library's own choice (what a default call does); 1..4 = the answer for a call that
 * forces this row-tile count through opts->rows_per_group (ABI v6).  The instances compute the same arithmetic (the GPU suite compares them bit for bit); they differ in how
 * much of the model's shape is a compile-time fact:
 *   GENERIC        everything decided at run time (any widths, activations, propagation, normaliser)
 *   HIDDEN_STATIC  SiLU models whose hidden layers are 193..208 wide -- the reference's default 200
 *                  (conf/dynamics_model/gaussian_mlp_ensemble.yaml:8) --, 113..128 or 241..256 wide, whatever their reward /
 *                  termination / preprocessing / output width
 *   FUSED          hidden AND output layer shapes, reward / termination closed form (or learned reward) and obs preprocessing are
 *                  compile-time facts; the output layer's accumulators feed the step's tail from registers (launch.hpp's tables:
 *                  the BASELINE.json configurations and the conf/overrides/pets_*.yaml workloads without a termination function
 *                  that reads every state dim)
 *   WIDE           FUSED for output layers wider than 8 column tiles (Humanoid-v4)
 *   BF16           a shape-specialised instance in HIPETS_PREC_BF16 arithmetic (launch.hpp HIPETS_BF16_SHAPES_R*)
 * Diagnostic only -- nothing needs to call it; a profile (rocprofv3 --kernel-trace) shows the same thing as a kernel name.      */
enum { HIPETS_KERNEL_GENERIC = 0, HIPETS_KERNEL_HIDDEN_STATIC = 1, HIPETS_KERNEL_FUSED = 2, HIPETS_KERNEL_WIDE = 3,
       HIPETS_KERNEL_BF16 = 4 /* a shape-specialised instance in HIPETS_PREC_BF16 arithmetic */ };
int hipets_kernel_class(hipets_engine* e, int32_t pop, int32_t num_particles, int32_t horizon, int32_t mode, int32_t rows_per_group,
                        int32_t* kernel_class, int32_t* row_tiles);

/* FAST-mode randomness, exported so a FAST rollout can be replayed through a reference implementation:
 * schedule DEVICE int32 [H, n_workgroups] = member slot of workgroup w at step t (the B = pop * P rows form one run,
 * particle-major -- run index g = p * pop + c for particle p of candidate c, i.e. row c * P + p of the batch -- and
 * workgroup w owns run indices [w * 16 * row_tiles, (w + 1) * 16 * row_tiles): n_workgroups = ceil(ceil(B / 16) /
 * row_tiles)).  Since ABI v6 the slot is position p_t(w) * M / n_workgroups of the step's keyed bijection p_t of the
 * workgroup indices (the Feistel network DEVICE mode applies to rows): every workgroup evaluates its own entry, there is
 * no schedule kernel or buffer behind a default call, and this export returns exactly those integers.
 * NOTE (small populations): a workgroup's 16 * row_tiles rows are CONSECUTIVE run indices, so when pop < 16 * row_tiles -- or
 * where a workgroup straddles the end of one particle's run -- several particles of the same candidate sit in one workgroup
 * and share a member at every step; the reference's per-row assignment (gaussian_mlp.py:267-275) gives them independent,
 * balanced members.  DEVICE mode (the default of the Python layer) has the reference's semantics at every size.
 * normals DEVICE f32 [H, B, out_dim] = the eps the kernel draws for (step, row, dim) with the same (seed, stream_id).     */
int hipets_fast_schedule(hipets_engine* e, int32_t horizon, int32_t n_workgroups, uint64_t seed, uint64_t stream_id,
                         int32_t* schedule, void* stream);
int hipets_fast_normals(hipets_engine* e, int32_t horizon, int32_t batch, uint64_t seed, uint64_t stream_id,
                        float* normals, void* stream);

/* DEVICE-mode randomness, exported for replay: perms DEVICE int64 [H, B] (random_model; [1, B] for fixed_model) = the
 * permutation a DEVICE rollout of `batch` = pop * particles rows with the same (seed, stream_id) uses at every step, in
 * the reference's convention (slot j holds row perms[t][j]; slot j runs on active member j / (B / M)); the eps of that
 * rollout are hipets_fast_normals(seed, stream_id).                                                              */
int hipets_device_perms(hipets_engine* e, int32_t horizon, int32_t batch, uint64_t seed, uint64_t stream_id, int64_t* perms,
                        void* stream);

/* DEVICE-mode rollouts with a fresh permutation per step (random_model) run as ONE persistent launch: only as many workgroups
 * as are resident at once are launched, rows change workgroups every step through a table of 16-byte {value, tag, value, tag}
 * granule pairs in HBM (write-through stores, polled loads; no grid barrier), and a batch with more logical workgroups than that
 * is served in turns by the launched ones (except where two workgroups fit a CU and the batch still exceeds the chip: those
 * launch once per step).  What makes that safe:
 *   - residency is VERIFIED, not assumed: the first time a kernel instance is to run persistently at a larger grid than before,
 *     the library launches that very instance in a self-test mode in which every workgroup waits for all the others (one extra
 *     launch and ONE synchronisation of `stream`, once per instance, LDS size (model / horizon) and grid size -- so the first plan
 *     of a new shape is not capturable into a hipGraph, later ones are); if they cannot meet, the runtime's smaller
 *     occupancy answer is tried, and failing that the engine launches per step.  What the self-tests found is kept per device,
 *     kernel instance and LDS size behind one lock per device: engines on one device driven from two host threads serialise the
 *     enqueue of their persistent launches there, and a persistent launch never exceeds the grid that was validated;
 *   - every poll is bounded (hipets_set_handover_timeout, default 0.2 s): if a producer never shows up (another process or
 *     stream took CUs after the self-test) the kernel raises a host-visible flag and drains in milliseconds.  The results of
 *     that launch, and everything computed from them, are INVALID;
 *   - hipets_check_async_error tells: call it once the results have reached the host (after the device-to-host copy of a plan,
 *     or any synchronisation of `stream`), before acting on them.  On *timed_out = 1 the engine has already fallen back to
 *     per-step launches: re-run the call (hipets.planning does exactly this).  A caller that never asks gets the report as an
 *     error from its NEXT rollout / plan call instead.
 * The persistent form assumes what the reference's deployment gives it -- one planning process per GPU; on = 0 forces per-step
 * launches (also: env HIPETS_NO_PERSISTENT=1).  Env HIPETS_MAX_WORKGROUPS=n caps the workgroups of a persistent launch at n (the
 * rest of the batch is served in turns, as when the chip is the limit): processes that share a GPU can leave each other room.
 * (The wide-output instances -- Humanoid-v4: 752 output columns, two row tiles per workgroup -- deal the LAST turn of a step in one-tile
 * workgroups when the row tiles left for it fit one per launched workgroup; same results bit for bit, a shorter step.  Env
 * HIPETS_RAGGED_LAST_TURN=0 keeps two-tile turns throughout: A/B measurements.)                                               */
int hipets_set_persistent(hipets_engine* e, int32_t on);
int hipets_set_handover_timeout(hipets_engine* e, double seconds);
int hipets_check_async_error(hipets_engine* e, int32_t* timed_out);

/* ---- CEMOptimizer pieces (mbrl/planning/trajectory_opt.py:100-188) ------------------------- */
typedef struct {
    int32_t population_size;
    int32_t horizon;
    int32_t act_dim;
    int32_t num_iterations;
    int32_t elite_num;          /* ceil(pop * elite_ratio), trajectory_opt.py:89-91             */
    double alpha;               /* momentum; (1 - alpha) is formed in double like the Python reference */
    int32_t return_mean_elites;
    int32_t clipped_normal;
    int32_t unbiased_var;       /* 1 = CEM (:137), 0 = iCEM (:479)                               */
} hipets_cem_params;

/* _sample_population (:110-128).  z DEVICE [pop,H,A] optional injected N(0,1) draws (already
 * truncated for the truncated-normal branch); NULL => Philox(seed, stream_id).  lower/upper/mu/
 * dispersion DEVICE [H,A]; population DEVICE [pop,H,A] out.                                    */
int hipets_cem_sample(hipets_engine* e, const hipets_cem_params* p, const float* mu, const float* dispersion,
                      const float* lower, const float* upper, const float* z, uint64_t seed, uint64_t stream_id,
                      float* population, void* stream);
/* NaN->-1e-10 (:178), topk (:179), elite mean/var refit with momentum (:130-140), best-so-far
 * (:184-186).  values DEVICE [pop] (modified in place like the reference); mu/dispersion in-out;
 * best_value DEVICE [1] in-out (init -inf); best_solution DEVICE [H,A] in-out;
 * elite_idx DEVICE [elite_num] int32 out (optional).                                           */
int hipets_cem_refit(hipets_engine* e, const hipets_cem_params* p, float* values, const float* population,
                     float* mu, float* dispersion, float* best_value, float* best_solution, int32_t* elite_idx,
                     void* stream);

/* The same refit with the elites CHOSEN BY THE CALLER: elites DEVICE [elite_num] int32 candidate indices, best first (values must
 * hold no index twice; out-of-range indices are the caller's error).  For seed-identical replays of the reference: the order
 * torch.topk (:179) leaves among EQUAL values is an artefact of its partial sort, and 0 / 1 reward functions (cartpole,
 * inverted pendulum: env/reward_fns.py:10-13, 27-30) tie dozens of candidates at the elite boundary -- the host runs the
 * reference's own topk on the returned values and hands the indices in.  NaN -> -1e-10 still happens in place.           */
int hipets_cem_refit_elites(hipets_engine* e, const hipets_cem_params* p, float* values, const float* population,
                            const int32_t* elites, float* mu, float* dispersion, float* best_value, float* best_solution,
                            void* stream);

/* population[elite_idx] -> dst (the persistent ICEMOptimizer.elite, trajectory_opt.py:476): rows of src
 * [n_src, D] selected by index DEVICE int32 [rows].                                                          */
int hipets_gather_rows(hipets_engine* e, int32_t rows, int32_t dim, const float* src, const int32_t* index, float* dst,
                       void* stream);

/* ---- MPPIOptimizer pieces (mbrl/planning/trajectory_opt.py:238-311) -------------------------------------- */
/* noise + beta-smoothing recurrence + clipping (:262-295).  mean DEVICE [H,A] (already shifted, :257-258),
 * past_action DEVICE [A], z DEVICE [pop,H,A] optional injected truncated normals, population DEVICE out.     */
int hipets_mppi_sample(hipets_engine* e, int32_t pop, int32_t horizon, int32_t act_dim, double beta, const float* mean,
                       const float* past_action, const float* lower, const float* upper, const float* z, uint64_t seed,
                       uint64_t stream_id, float* population, void* stream);
/* NaN -> -1e-10, exp(gamma (v - max v)) weights, weighted mean (:296-309).  values DEVICE [pop] in place.     */
int hipets_mppi_update(hipets_engine* e, int32_t pop, int32_t horizon, int32_t act_dim, double gamma, float* values,
                       const float* population, float* mean, void* stream);

/* ---- ICEMOptimizer pieces (mbrl/planning/trajectory_opt.py:391-487, mbrl/util/math.py:318-396) ------------ */
/* coloured-noise population (:433-441): n rows of population DEVICE [>= n, H, A].  normals DEVICE
 * [2, n, A, H/2+1] optional injected unit normals (real, imaginary parts of the spectrum).                   */
int hipets_icem_sample(hipets_engine* e, int32_t n, int32_t horizon, int32_t act_dim, double exponent, const float* mu,
                       const float* var, const float* lower, const float* upper, const float* normals, uint64_t seed,
                       uint64_t stream_id, float* population, void* stream);
/* kept elites shifted one step with a fresh tail action (:450-462).  kept DEVICE [keep,H,A]; end_noise DEVICE
 * [keep, A] optional injected N(0,1); out DEVICE [keep,H,A].                                                   */
int hipets_icem_shift(hipets_engine* e, int32_t keep, int32_t horizon, int32_t act_dim, const float* kept, const float* mu,
                      const float* var, const float* end_noise, uint64_t seed, uint64_t stream_id, float* out, void* stream);

/* ---- fused plans: a whole optimizer.optimize() with the engine's rollout as objective -------- */
/* Randomness mode of the rollouts inside the hipets_plan_* calls: HIPETS_MODE_FAST (default) or HIPETS_MODE_DEVICE
 * (reference propagation semantics).  Iteration i of plan `plan_id` uses stream_id = plan_id * num_iterations + i for
 * both its population noise and its rollout (iCEM: 4 * that, + 0..3 for noise / shifted tail / kept-elite draw / rollout). */
int hipets_set_plan_mode(hipets_engine* e, int32_t mode);

/* Optional per-iteration record of the following fused plans (NULL pointers are skipped, a NULL trace switches recording
 * off).  All DEVICE, written asynchronously on the plan's stream; for a batched plan n_env > 1, else n_env = 1:
 *   populations [iters, max_rows, H, A]  the candidates iteration i evaluated, environment after environment (max_rows
 *                                        >= n_env * the largest per-environment count; rows beyond an iteration's untouched)
 *   values      [iters, max_rows]        their returns after the NaN filter
 *   mus, dispersions [iters, n_env, H, A]  optimizer state after iteration i (MPPI: mus = the refined mean)
 *   elite_idx   [iters, n_env, elite_num]  int32, best first, indices into the environment's own candidates (CEM / iCEM)
 * This is what lets a test replay a fused plan through a reference implementation draw by draw.                      */
typedef struct {
    float* populations;
    float* values;
    float* mus;
    float* dispersions;
    int32_t* elite_idx;
    int32_t max_rows;
} hipets_plan_trace;
int hipets_set_plan_trace(hipets_engine* e, const hipets_plan_trace* trace);

/* Whole CEMOptimizer.optimize with the engine's rollout as objective, no host round trip
 * (replaces trajectory_opt.py:142-188 + the closure at :743-748).  x0/lower/upper DEVICE [H,A];
 * out DEVICE [H,A] = mu if return_mean_elites else best.  Rollouts in the engine's plan mode;
 * workspace is engine-owned.                                                                  */
int hipets_plan_cem(hipets_engine* e, const hipets_cem_params* p, const float* x0, const float* lower,
                    const float* upper, const float* s0, int32_t num_particles, uint64_t seed, uint64_t plan_id,
                    float* out, void* stream);
/* The same for n_env independent environments in ONE set of launches (vectorised envs / many agents): x0 and out
 * DEVICE [n_env,H,A], s0 HOST [n_env,obs_dim], bounds shared.  p->population_size is PER environment.  Fills all 256 CUs
 * where a single plan cannot (cfg2 has 2.4 row tiles per CU).                                                    */
int hipets_plan_cem_batched(hipets_engine* e, const hipets_cem_params* p, int32_t n_env, const float* x0, const float* lower,
                            const float* upper, const float* s0, int32_t num_particles, uint64_t seed, uint64_t plan_id,
                            float* out, void* stream);

/* Whole MPPIOptimizer.optimize (trajectory_opt.py:238-311) with the engine's FAST rollout as objective.
 * mean DEVICE [H,A] in-out = the optimizer's persistent self.mean: shifted one step in place (:257-258), then
 * refined num_iterations times (:262-309); the refined mean is what optimize() returns (:311).              */
int hipets_plan_mppi(hipets_engine* e, int32_t population_size, int32_t horizon, int32_t act_dim, int32_t num_iterations,
                     double gamma, double beta, float* mean, const float* lower, const float* upper, const float* s0,
                     int32_t num_particles, uint64_t seed, uint64_t plan_id, void* stream);

/* The same for n_env environments in ONE set of launches (FAST-mode rollouts): mean DEVICE [n_env,H,A] in-out, s0 HOST
 * [n_env,obs_dim], bounds shared, population_size PER environment.                                               */
int hipets_plan_mppi_batched(hipets_engine* e, int32_t population_size, int32_t horizon, int32_t act_dim, int32_t num_iterations,
                             double gamma, double beta, int32_t n_env, float* mean, const float* lower, const float* upper,
                             const float* s0, int32_t num_particles, uint64_t seed, uint64_t plan_id, void* stream);

typedef struct {
    int32_t population_size;
    int32_t horizon;
    int32_t act_dim;
    int32_t num_iterations;
    int32_t elite_num;              /* ceil(pop * elite_ratio), trajectory_opt.py:368-370                      */
    int32_t keep_elite_size;        /* ceil(keep_elite_frac * elite_num), rounded up to the module (:378-383)  */
    int32_t population_size_module; /* 0 = none (:419-431)                                                     */
    int32_t return_mean_elites;
    double alpha;
    double population_decay_factor;
    double colored_noise_exponent;
} hipets_icem_params;

/* Whole ICEMOptimizer.optimize (trajectory_opt.py:391-487) with the engine's FAST rollout as objective.
 * elite DEVICE [elite_num,H,A] in-out = the optimizer's persistent self.elite (read only when has_elite != 0,
 * always written: it holds the last iteration's elites on return).  keep_idx DEVICE int32 [num_iterations,
 * keep_elite_size] optional injected randperm(elite_num)[:keep] per iteration (:446-448); NULL => Philox.
 * out DEVICE [H,A] = mu if return_mean_elites else best.                                                      */
int hipets_plan_icem(hipets_engine* e, const hipets_icem_params* p, const float* x0, const float* lower, const float* upper,
                     float* elite, int32_t has_elite, const int32_t* keep_idx, const float* s0, int32_t num_particles,
                     uint64_t seed, uint64_t plan_id, float* out, void* stream);

/* The same for n_env environments in ONE set of launches (FAST-mode rollouts): x0 / out DEVICE [n_env,H,A], elite DEVICE
 * [n_env,elite_num,H,A] in-out, keep_idx DEVICE int32 [num_iterations, n_env, keep_elite_size] or NULL, s0 HOST
 * [n_env,obs_dim]; bounds and the per-iteration population sizes are shared by the environments.                   */
int hipets_plan_icem_batched(hipets_engine* e, const hipets_icem_params* p, int32_t n_env, const float* x0, const float* lower,
                             const float* upper, float* elite, int32_t has_elite, const int32_t* keep_idx, const float* s0,
                             int32_t num_particles, uint64_t seed, uint64_t plan_id, float* out, void* stream);

/* ---- multi-GPU: population sharding with ONE all-gather of returns per iteration --------------------- */
/* The library talks to RCCL itself (librccl is loaded on first use, no link-time dependency): rank 0 makes an id, the
 * host broadcasts its HIPETS_COMM_ID_BYTES bytes by any means (MPI, torch.distributed, a file), every rank joins.        */
#define HIPETS_COMM_ID_BYTES 128
int hipets_comm_unique_id(void* id_out);
int hipets_comm_init(hipets_engine* e, const void* unique_id, int32_t rank, int32_t world_size);
int hipets_comm_destroy(hipets_engine* e);
/* rank and size as the communicator itself reports them (ncclCommUserRank / ncclCommCount); 0 / 1 without a communicator.
 * Env HIPETS_RCCL_LIB=<path> makes the library load that shared object instead of librccl (tests/fake_rccl builds a stand-in
 * that runs N ranks as N processes on ONE GPU, so the world > 1 path of hipets_plan_cem_sharded is testable on a 1-GPU box). */
int hipets_comm_info(hipets_engine* e, int32_t* rank, int32_t* world_size);
/* hipets_plan_cem over all ranks of the communicator as one device-side loop per rank: every rank passes IDENTICAL
 * arguments; the population is sampled identically everywhere (counter-based RNG), rank r rolls out candidates
 * [r * pop / world ...) (first pop % world ranks hold one more), one ncclAllGather of the per-candidate returns per
 * iteration over xGMI, then the same refit on the same data everywhere (bit-identical mu / dispersion, no broadcast).
 * With world_size == 1 it equals hipets_plan_cem.  Shard sizes that the rollout mode cannot take (DEVICE mode: rows % members)
 * are refused on every rank before the first collective; a rank on which an iteration cannot be enqueued keeps taking part in
 * the collectives and returns its error at the end (no peer is left waiting) -- agree on the outcome across ranks before using
 * a plan (hipets.dist.plan_cem_sharded does).  hipets_set_plan_trace records the gathered values like hipets_plan_cem's.   */
int hipets_plan_cem_sharded(hipets_engine* e, const hipets_cem_params* p, const float* x0, const float* lower, const float* upper,
                            const float* s0, int32_t num_particles, uint64_t seed, uint64_t plan_id, float* out, void* stream);

/* The same scheme for the other two optimizers ("MPPI: same all-gather of values (weights need global max and
 * sum)"; "iCEM: kept elites are replicated state, so same scheme"): arguments as hipets_plan_mppi / hipets_plan_icem, identical
 * on every rank; sampling (MPPI's smoothed noise; iCEM's coloured noise, kept / shifted elites, the +1 mu row) is replicated,
 * every iteration's population -- iCEM's shrinks from iteration to iteration, the shards with it -- is rolled out shard-wise and
 * its returns all-gathered, the importance-weighted mean (:297-311) / the elite refit (:474-485) then runs on identical data
 * everywhere: bit-identical persistent state (`mean`, `elite`) on all ranks.  Same refusal / failure rules as above.       */
int hipets_plan_mppi_sharded(hipets_engine* e, int32_t population_size, int32_t horizon, int32_t act_dim, int32_t num_iterations,
                             double gamma, double beta, float* mean, const float* lower, const float* upper, const float* s0,
                             int32_t num_particles, uint64_t seed, uint64_t plan_id, void* stream);
int hipets_plan_icem_sharded(hipets_engine* e, const hipets_icem_params* p, const float* x0, const float* lower, const float* upper,
                             float* elite, int32_t has_elite, const int32_t* keep_idx, const float* s0, int32_t num_particles,
                             uint64_t seed, uint64_t plan_id, float* out, void* stream);

/* ---- PlaNet latent planner (mbrl/models/planet.py) ----------------------------------- */
/* The tensors PlaNetModel.sample reads (planet.py:531-581), DEVICE f32 in nn.Linear layout: weights [out, in]
 * row-major, biases [out].  The library packs private copies; call again after every model update.            */
typedef struct {
    int32_t latent_size;     /* latent_state_size                                                               */
    int32_t action_size;
    int32_t belief_size;
    int32_t hidden_size;     /* hidden_size_fcs                                                                 */
    float min_std;           /* MeanStdCat (planet.py:104-115)                                                  */
    const void* w_embed;     /* belief_model.embedding_layer[0]  [belief, latent + action]   (planet.py:86-88)  */
    const void* b_embed;
    const void* w_ih;        /* belief_model.rnn (GRUCell) weight_ih [3 belief, belief], gates r | z | n  (:89) */
    const void* b_ih;
    const void* w_hh;        /* weight_hh [3 belief, belief]                                                    */
    const void* b_hh;
    const void* w_prior1;    /* prior_transition_model[0] [hidden, belief]                        (:229-234)   */
    const void* b_prior1;
    const void* w_prior2;    /* prior_transition_model[2] [2 latent, hidden]                                    */
    const void* b_prior2;
    const void* w_rew1;      /* reward_model[0] [hidden, belief + latent]                          (:260-266)   */
    const void* b_rew1;
    const void* w_rew2;      /* reward_model[2] [hidden, hidden]                                                */
    const void* b_rew2;
    const void* w_rew3;      /* reward_model[4] [1, hidden]                                                     */
    const void* b_rew3;
} hipets_planet_desc;
int hipets_planet_set_model(hipets_engine* e, const hipets_planet_desc* d, void* stream);

typedef struct {
    const float* eps;        /* DEVICE [H,B,latent] injected N(0,1) draws of planet.py:299-305; NULL => Philox   */
    uint64_t seed;
    uint64_t stream_id;
    int32_t no_sample;       /* latent = prior mean (sample(deterministic=True))                                 */
    float* trace_latent;     /* optional DEVICE taps: [H,B,latent], [H,B,belief], [H,B]                          */
    float* trace_belief;
    float* trace_rewards;
    int64_t* phase_cycles;   /* ABI v6: DEVICE [8,16] phase accumulators of workgroup 0, as hipets_rollout_opts.phase_cycles;    */
                             /*   filled by profiling builds (-DHIPETS_LEAN_PROF=1) only, ignored by the shipped library         */
    int32_t n_env;           /* ABI v7: batched rollouts: the pop candidates are n_env groups of pop / n_env (pop must divide),  */
                             /*   group g starts from latent0[g] / belief0[g] (then [n_env, latent] / [n_env, belief]); 0/1 = one */
} hipets_planet_opts;
/* ModelEnv.evaluate_action_sequences on a PlaNetModel with no_termination and the learned reward head
 * (model_env.py:145-191, mbrl/algorithms/planet.py): actions DEVICE [pop,H,A]; latent0 / belief0 DEVICE [latent] /
 * [belief] = the model's saved posterior sample and belief (planet.py:669-672), tiled over the pop * P rows (one per
 * environment with opts.n_env > 1); returns DEVICE [pop] particle-averaged.  One kernel launch for the whole horizon.
 * eps, the traces and the in-kernel draws are indexed by the launch-global row (candidate * P + particle).          */
int hipets_planet_rollout(hipets_engine* e, const float* actions, const float* latent0, const float* belief0, int32_t pop,
                          int32_t horizon, int32_t num_particles, const hipets_planet_opts* opts, float* returns, void* stream);
/* Diagnostic: which instance of the PlaNet rollout kernel the next hipets_planet_rollout (and every PlaNet plan) launches for the
 * model set last: *is_static = 1 the instance specialised for the tile counts of conf/dynamics_model/planet.yaml, 0 the run-time
 * generic one (always with HIPETS_PLANET_GENERIC=1 in the environment).  The same bits either way.                              */
int hipets_planet_kernel_class(hipets_engine* e, int32_t* is_static);

/* The PlaNet planner as one call: CEMOptimizer.optimize (trajectory_opt.py:142-188; the PlaNet configs use the clipped-normal
 * branch :116-120, conf/overrides/planet_cheetah_run.yaml:29-35) with hipets_planet_rollout as objective, no host round trip.
 * Arguments as hipets_plan_cem, with the latent start state of hipets_planet_rollout instead of an observation.            */
int hipets_plan_planet_cem(hipets_engine* e, const hipets_cem_params* p, const float* x0, const float* lower, const float* upper,
                           const float* latent0, const float* belief0, int32_t num_particles, uint64_t seed, uint64_t plan_id,
                           float* out, void* stream);

/* Batched PlaNet planning: the three fused plans for n_env environments in ONE set of launches per
 * iteration, each environment rolled out from its own latent start state (planet.py:656-672 per environment).  Arguments as
 * hipets_plan_cem_batched / hipets_plan_mppi_batched / hipets_plan_icem_batched, with DEVICE latent0 [n_env, latent] /
 * belief0 [n_env, belief] instead of the HOST s0; population_size is PER environment, n_env = 1 is allowed.  The rollouts draw
 * their eps in-kernel (Philox, keyed by the launch-global row).  Local GPU only: an engine's communicator is not used.
 * hipets_set_plan_trace records them like the ensemble's batched plans.                                                  */
int hipets_plan_planet_cem_batched(hipets_engine* e, const hipets_cem_params* p, int32_t n_env, const float* x0, const float* lower,
                                   const float* upper, const float* latent0, const float* belief0, int32_t num_particles, uint64_t seed,
                                   uint64_t plan_id, float* out, void* stream);
int hipets_plan_planet_mppi_batched(hipets_engine* e, int32_t population_size, int32_t horizon, int32_t act_dim, int32_t num_iterations,
                                    double gamma, double beta, int32_t n_env, float* mean, const float* lower, const float* upper,
                                    const float* latent0, const float* belief0, int32_t num_particles, uint64_t seed, uint64_t plan_id,
                                    void* stream);
int hipets_plan_planet_icem_batched(hipets_engine* e, const hipets_icem_params* p, int32_t n_env, const float* x0, const float* lower,
                                    const float* upper, float* elite, int32_t has_elite, const int32_t* keep_idx, const float* latent0,
                                    const float* belief0, int32_t num_particles, uint64_t seed, uint64_t plan_id, float* out,
                                    void* stream);

/* ---- GaussianMLP ensemble training: ModelTrainer.train / evaluate (mbrl/models/model_trainer.py:70-262) --------- (ABI v8) */
/* One GaussianMLP of E members, NLL loss (gaussian_mlp.py:291-305), fixed logvar bounds, torch.optim.Adam with coupled weight
 * decay (model_trainer.py:63-68).  Parameters and Adam state are caller-owned DEVICE f32 tensors in torch's layout, updated in
 * place: weights[l] [E, d_l, d_{l+1}], biases[l] [E, 1, d_{l+1}] with d_0 = in_dim, d_1 .. d_{n_layers-1} = hid and
 * d_{n_layers} = 2 out_dim (mean | raw logvar columns).  Limits: E <= 16, 2 <= n_layers <= 8, in_dim <= 512, hid <= 256,
 * out_dim <= 512, max_batch <= 256 (the HIPETS_TRAIN_MAX_* limits); anything else fails with HIPETS_ERR_INVALID_ARGUMENT.  */
#define HIPETS_TRAIN_MAX_MEMBERS 16
#define HIPETS_TRAIN_MAX_HID 256
#define HIPETS_TRAIN_MAX_IN 512
#define HIPETS_TRAIN_MAX_OUT 512
#define HIPETS_TRAIN_MAX_BATCH 256
typedef struct {
    int32_t ensemble_size;   /* E                                                                                    */
    int32_t n_layers;        /* linear layers = num_layers of GaussianMLP + 1                                        */
    int32_t in_dim;
    int32_t hid;
    int32_t out_dim;         /* target columns (obs dims + learned reward)                                           */
    int32_t activation;      /* HIPETS_ACT_*                                                                         */
    float leaky_slope;
    int32_t max_batch;       /* rows of the widest minibatch of a hipets_train_steps call: sizes the idx rows       */
    void* const* weights;    /* HOST array [n_layers] of DEVICE f32 pointers                                         */
    void* const* biases;
    void* const* exp_avg_w;  /* Adam exp_avg of every weight / bias tensor, same layouts                             */
    void* const* exp_avg_b;
    void* const* exp_avg_sq_w; /* Adam exp_avg_sq                                                                   */
    void* const* exp_avg_sq_b;
    const float* min_logvar; /* DEVICE [out_dim] (constant: learn_logvar_bounds = False)                              */
    const float* max_logvar;
    double lr, beta1, beta2, eps, weight_decay; /* param_groups[0] of the optimizer                                   */
    int32_t steps_per_launch; /* 0 = the library's choice (launches of at most ~50 ms); else at most this many steps  */
} hipets_train_desc;
/* n_steps consecutive minibatch steps (Model.update, model.py:129-167): step s runs member e on dataset rows
 * idx[s, e, 0 .. rows[s]) of x DEVICE f32 [n_rows, in_dim] (model inputs, normalised) and y DEVICE f32 [n_rows, out_dim]
 * (targets); idx DEVICE int32 [n_steps, E, max_batch], rows DEVICE int32 [n_steps] (1 .. max_batch; an index outside
 * [0, n_rows) reads zeros).  step0 = Adam steps taken before the call (torch's state "step"): step s uses t = step0 + s + 1 in
 * its bias corrections (computed in double, as torch does).  Writes loss DEVICE f32 [n_steps, E] (each member's mean NLL;
 * the reference's loss is their sum + 0.01 (sum max_logvar - sum min_logvar)) and grad_sq DEVICE f32 [n_steps, E] (sum of
 * squares of the member's raw gradient, before weight decay: model.py:153-158 sums these over members and tensors).
 * Members run in parallel, steps in order; the call is cut into launches of steps_per_launch steps (results do not depend
 * on where the cuts fall).                                                                                                 */
int hipets_train_steps(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows,
                       const int32_t* idx, const int32_t* rows, int32_t n_steps, int64_t step0, float* loss, float* grad_sq,
                       void* stream);
/* ModelTrainer.evaluate over a whole dataset (GaussianMLP.eval_score, gaussian_mlp.py:337-361, averaged over rows and dims):
 * score DEVICE f32 [E] = mean over the n_rows rows and out_dim dims of (mean_e(x) - y)^2, the mean columns only.  order
 * DEVICE int32 [n_rows] or NULL: row r of the pass is dataset row order[r].  row_score DEVICE f32 [E, n_rows] or NULL: the
 * squared error of pass row r summed over dims (per-batch scores for a batch_callback).  As in training, an order entry
 * outside [0, n_rows) is never read out of bounds: that pass row contributes exactly zero to row_score and to the sum,
 * while the divisor of score stays n_rows * out_dim.  A row's arithmetic does not depend on its position in the pass
 * (row_score under order = a permutation is the permuted row_score, bit for bit).  Partial sums are reduced in a fixed
 * order: the result is deterministic.  The Adam fields of d are not read.                                                */
int hipets_train_eval(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows,
                      const int32_t* order, float* score, float* row_score, void* stream);
/* Loss kinds of hipets_train_steps_loss / hipets_train_eval_loss (additive entry points: hipets_train_desc keeps its layout and
 * HIPETS_ABI_VERSION its value; the new parameters travel as scalars). */
#define HIPETS_TRAIN_LOSS_NLL 0 /* GaussianMLP._nll_loss (gaussian_mlp.py:291-305): what hipets_train_steps trains               */
#define HIPETS_TRAIN_LOSS_MSE 1 /* GaussianMLP._mse_loss (gaussian_mlp.py:283-289) of a deterministic model                       */
/* hipets_train_steps with a loss kind, per-member logvar bounds and a gradient scale; (HIPETS_TRAIN_LOSS_NLL, 0, 1.0f) IS
 * hipets_train_steps.  Under HIPETS_TRAIN_LOSS_MSE the descriptor is read differently: the last layer is out_dim wide
 * (d_{n_layers} = out_dim, no logvar columns), min_logvar / max_logvar are ignored and may be NULL, and loss[s, e] is the
 * member's plain SUM over the step's rows and dims of the squared error (a sum, not a mean).  bounds_per_member != 0 (NLL): the
 * bounds are DEVICE [E, out_dim], member e reads row e -- a BasicEnsemble (mbrl/models/basic_ensemble.py) of one-member
 * GaussianMLPs stacked into one descriptor.  grad_scale (finite, > 0) multiplies the gradient of the loss before Adam and
 * is therefore part of grad_sq, but not of loss: BasicEnsemble.loss divides the sum of the member losses by E, so each of
 * its members trains with grad_scale = 1 / E.  1.0f changes no bit.  An unknown loss_kind, a grad_scale that is not finite or
 * is <= 0, and NULL bounds under NLL fail with HIPETS_ERR_INVALID_ARGUMENT before anything is launched.                     */
int hipets_train_steps_loss(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows,
                            const int32_t* idx, const int32_t* rows, int32_t n_steps, int64_t step0, float* loss,
                            float* grad_sq, void* stream, int32_t loss_kind, int32_t bounds_per_member, float grad_scale);
/* hipets_train_eval for either loss kind: under HIPETS_TRAIN_LOSS_MSE the last layer is out_dim wide (all of its columns are
 * means), under HIPETS_TRAIN_LOSS_NLL 2 out_dim wide (the first out_dim are).  The score is the same squared error.          */
int hipets_train_eval_loss(hipets_engine* e, const hipets_train_desc* d, const float* x, const float* y, int64_t n_rows,
                           const int32_t* order, float* score, float* row_score, void* stream, int32_t loss_kind);

/* ---- MBPO model rollouts: the SAC Gaussian actor and the compacting populate step (mbrl/algorithms/mbpo.py:31-63) ----
 * Additive entry points: scalars and pointers only, no struct, HIPETS_ABI_VERSION stays.  Needs no dynamics model.
 *
 * The actor is GaussianPolicy.forward / sample (mbrl/third_party/pytorch_sac_pranz24/model.py:88-108) as SAC.select_action uses it:
 *   h1 = relu(obs W1^T + b1);  h2 = relu(h1 W2^T + b2);  mean = h2 Wm^T + bm;  log_std = clamp(h2 Ws^T + bs, -20, 2)
 *   sample != 0:  action = tanh(mean + exp(log_std) * eps) * action_scale + action_bias
 *   sample == 0:  action = tanh(mean) * action_scale + action_bias
 * All products are fp32 MFMA with fp32 accumulation, everything after them fp32 op by op (no fused multiply-add).
 * hipets_policy_set copies DEVICE tensors in nn.Linear's layout -- w1 [hidden, obs_dim], w2 [hidden, hidden], wm / ws [act_dim, hidden],
 * b1 / b2 [hidden], bm / bs [act_dim] -- and the per-dimension action_scale / action_bias [act_dim] into the engine's own packed layout
 * (the two heads become ONE product of 2 act_dim columns); it does not synchronise: the source tensors must stay alive until the
 * work enqueued on `stream` has run (stream-ordered frees, as torch's allocator does them, are fine).
 * 1 <= obs_dim <= 512, 1 <= hidden <= 1024, 1 <= act_dim <= 32; anything else is HIPETS_ERR_INVALID_ARGUMENT.                       */
#define HIPETS_POLICY_MAX_OBS 512
#define HIPETS_POLICY_MAX_HIDDEN 1024
#define HIPETS_POLICY_MAX_ACT 32
int hipets_policy_set(hipets_engine* e, int32_t obs_dim, int32_t hidden, int32_t act_dim, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* wm, const float* bm, const float* ws, const float* bs, const float* action_scale,
                      const float* action_bias, void* stream);
/* One launch: obs DEVICE [batch, obs_dim] -> actions DEVICE [batch, act_dim]; batch >= 1.  eps DEVICE [batch, act_dim] or NULL: with
 * sample != 0 and eps == NULL the kernel draws eps[row][d] itself, Philox normals keyed by (seed, stream_id, row, d) in a key domain
 * of their own (independent of the rollouts' draws of the same (seed, stream_id)); hipets_policy_normals returns exactly that table.
 * Optional taps (NULL = not wanted): mean_out / log_std_out DEVICE [batch, act_dim], the heads before tanh (log_std after its clamp).
 * A row's arithmetic does not depend on the batch it arrives in: row r of any call equals the one-row call on obs[r].               */
int hipets_policy_act(hipets_engine* e, const float* obs, int32_t batch, int32_t sample, uint64_t seed, uint64_t stream_id, const float* eps,
                      float* actions, float* mean_out, float* log_std_out, void* stream);
/* out DEVICE f32 [batch, act_dim] = the eps hipets_policy_act draws in-kernel for (seed, stream_id).  Needs no policy.              */
int hipets_policy_normals(hipets_engine* e, int32_t batch, int32_t act_dim, uint64_t seed, uint64_t stream_id, float* out, void* stream);
/* Launch geometry of hipets_policy_act for `batch` rows of the policy set last: a workgroup owns 16 * row_tiles rows (row_tiles = the
 * largest of 4, 2, 1 whose activations fit the LDS opt-in limit, no more than the batch needs); lds_bytes = its dynamic LDS.         */
int hipets_policy_geometry(hipets_engine* e, int32_t batch, int32_t* row_tiles, int32_t* lds_bytes);
/* mbpo.py:53-63 for one rollout step, on the device.  obs / next_obs DEVICE f32 [n, obs_dim], action DEVICE f32 [n, act_dim], rewards
 * DEVICE f32 [n], dones / accum_dones DEVICE uint8 [n] (non-zero = set).  The rows with accum_dones == 0 are appended in row order
 * to the staging area, DEVICE f32 [cap * (2 obs_dim + act_dim + 2)]: five arrays one behind the other, obs [cap, obs_dim], action
 * [cap, act_dim], next_obs [cap, obs_dim], reward [cap], done [cap] (0.0f or 1.0f), every float a plain copy -- starting at row
 * *offset (DEVICE int64, the running fill); *count_out (DEVICE int32) = the rows kept, *offset += that count, then accum_dones |= dones.
 * A kept row that would land at or past `cap` is dropped (the counts still advance).
 * Three ordered launches (per-block counts, one workgroup's scan of them, the scatter); nothing waits on another workgroup.          */
int hipets_compact_transitions(hipets_engine* e, const float* obs, const float* action, const float* next_obs, const float* rewards,
                               const uint8_t* dones, uint8_t* accum_dones, int32_t n, int32_t obs_dim, int32_t act_dim, float* staging,
                               int64_t cap, int64_t* offset, int32_t* count_out, void* stream);

/* ---- a device-resident SAC replay buffer: the populate's ring form and the batch gather ----
 * Additive entry points: scalars and pointers only, no struct, HIPETS_ABI_VERSION stays.  Need no dynamics model.
 *
 * `ring` is a replay buffer's storage, DEVICE f32 [capacity * (2 obs_dim + act_dim + 2)]: the staging area's five arrays over
 * `capacity` rows, one behind the other -- obs [capacity, obs_dim], action [capacity, act_dim], next_obs [capacity, obs_dim], reward
 * [capacity], done [capacity] (0.0f or 1.0f).
 *
 * hipets_ring_compact_transitions is hipets_compact_transitions followed by mbrl.util.ReplayBuffer.add_batch (replay_buffer.py:553-599)
 * for one rollout step: inputs as there; `cursor` is a DEVICE int64[2] = (cur_idx, num_stored).  The k-th row with accum_dones == 0,
 * in row order, lands at ring row (cur_idx + k) % capacity, every float a plain copy.  Afterwards cur_idx = (cur_idx + kept) %
 * capacity, num_stored = min(num_stored + kept, capacity) -- add_batch's rule whenever num_stored >= cur_idx, which add_batch
 * maintains --, *count_out (DEVICE int32) = kept and accum_dones |= dones.  A cur_idx outside [0, capacity) is folded into it first.
 * n > capacity is HIPETS_ERR_INVALID_ARGUMENT (nothing is launched).  The same three ordered launches (the count kernel is shared);
 * nothing waits on another workgroup, no atomics; all row arithmetic is 64-bit.                                                     */
int hipets_ring_compact_transitions(hipets_engine* e, const float* obs, const float* action, const float* next_obs, const float* rewards,
                                    const uint8_t* dones, uint8_t* accum_dones, int32_t n, int32_t obs_dim, int32_t act_dim, float* ring,
                                    int64_t capacity, int64_t* cursor, int32_t* count_out, void* stream);
/* One launch: indices DEVICE int64 [n_rows] -> out DEVICE f32 [n_rows, 2 obs_dim + act_dim + 2], row j = (obs[i], action[i],
 * next_obs[i], reward[i], mask) of ring row i = indices[j]: the batch layout hipets_sac_update reads (any number of batches behind
 * each other).  mask = done when reverse_mask == 0, else (done == 0) ? 1.0f : 0.0f (mask_batch.logical_not(), sac.py:93-95).  Plain
 * copies.  An index outside [0, capacity) reads nothing and makes its whole output row quiet NaN; no error is raised.  n_rows >= 1,
 * 1 <= obs_dim, act_dim <= 4096, capacity >= 1; anything else is HIPETS_ERR_INVALID_ARGUMENT.                                      */
int hipets_replay_gather(hipets_engine* e, const float* ring, int64_t capacity, int32_t obs_dim, int32_t act_dim, const int64_t* indices,
                         int64_t n_rows, int32_t reverse_mask, float* out, void* stream);

/* ---- SAC updates: SAC.update_parameters (mbrl/third_party/pytorch_sac_pranz24/sac.py:76-173) on the device ----
 * Additive entry points: scalars and pointers only, no struct, HIPETS_ABI_VERSION stays.  Needs no dynamics model.
 *
 * hipets_sac_bind tells the engine where a Gaussian-policy SAC agent LIVES: `ptrs` is a HOST table of HIPETS_SAC_N_PTRS DEVICE
 * pointers to contiguous f32 tensors, nn.Linear's [out, in] layout, which hipets_sac_update reads and writes IN PLACE (no packed
 * copy is kept, nothing is written back):
 *    0 ..  7  policy: linear1.weight, .bias, linear2.weight, .bias, mean_linear.weight, .bias, log_std_linear.weight, .bias
 *    8 .. 15  their Adam exp_avg, 16 .. 23 their exp_avg_sq (policy_optim)
 *   24 .. 35  critic: linear1 .. linear6, weight then bias each (linear1-3 = Q1, linear4-6 = Q2; linear1 / 4 are [hidden, obs + act])
 *   36 .. 47  their exp_avg, 48 .. 59 their exp_avg_sq (critic_optim)
 *   60 .. 71  critic_target, as the critic
 *   72 .. 74  log_alpha [1], its exp_avg, its exp_avg_sq (alpha_optim; may be NULL when tuning == 0)
 *   75        alpha [1]: the entropy coefficient the update uses; with tuning != 0 the update leaves exp(new log_alpha) there
 *   76, 77    action_scale, action_bias [act_dim]
 * adam: HOST [3][3] = (beta1, beta2, eps) of critic_optim, policy_optim, alpha_optim (plain Adam: no amsgrad, weight decay, maximize).
 * 1 <= obs_dim <= 512, 1 <= hidden <= 1024, 1 <= act_dim <= 32 (the HIPETS_POLICY_MAX_* limits), target_update_interval >= 1;
 * anything else is HIPETS_ERR_INVALID_ARGUMENT.  The table is copied; the tensors must stay where they are until the next bind.   */
#define HIPETS_SAC_N_PTRS 78
#define HIPETS_SAC_MAX_BATCH 1024
int hipets_sac_bind(hipets_engine* e, int32_t obs_dim, int32_t act_dim, int32_t hidden, int32_t tuning, double gamma, double tau,
                    double target_entropy, int32_t target_update_interval, const double* adam, const void* ptrs, int32_t n_ptrs);
/* One update, a fixed sequence of 19 ordinary launches on `stream` (no kernel waits on another workgroup, no float atomics: a repeated
 * call gives the same bits).  batch DEVICE f32 [batch_size, 2 obs_dim + act_dim + 2]: a row is (state, action, next_state, reward,
 * mask), mask = what sac.py:93-95 leaves in mask_batch; 1 <= batch_size <= HIPETS_SAC_MAX_BATCH.  eps_next / eps_cur DEVICE f32
 * [batch_size, act_dim]: the normals of policy.sample(next_state) and policy.sample(state), in the order the reference draws them.
 * update_index = the reference's `updates` (the target's soft update runs when update_index % target_update_interval == 0, with the
 * critic's NEW values); step_* = the Adam steps each optimizer has taken BEFORE this update; lr_* its learning rate now.
 * result DEVICE f32 [8] = (qf1_loss, qf2_loss, policy_loss, alpha_loss, alpha, mean reward of the batch, -mean(log_pi), 0).
 * Products are fp32 MFMA with fp32 accumulation; everything else fp32 op by op in the reference's order.                          */
int hipets_sac_update(hipets_engine* e, const float* batch, int32_t batch_size, const float* eps_next, const float* eps_cur,
                      int64_t update_index, int64_t step_critic, int64_t step_policy, int64_t step_alpha, double lr_critic, double lr_policy,
                      double lr_alpha, float* result, void* stream);
/* Intermediates of the LAST update (batch_size must be that update's), each DEVICE f32 [batch_size] or NULL: the critic's q1 / q2 on
 * (state, action), the TD target y, log_pi of the next-state sample and of the state sample.                                      */
int hipets_sac_forward_taps(hipets_engine* e, int32_t batch_size, float* q1, float* q2, float* y, float* log_pi_next, float* log_pi,
                            void* stream);

/* ---- value-bootstrapped planning: the SAC critic and discounted returns with a terminal value ----
 * Additive entry points: scalars and pointers only, no struct, HIPETS_ABI_VERSION stays.  Need no dynamics model.
 *
 * The critic is QNetwork.forward (mbrl/third_party/pytorch_sac_pranz24/model.py:36-61) on xu = [state, action]:
 *   q1 = linear3(relu(linear2(relu(linear1(xu)))));  q2 = linear6(relu(linear5(relu(linear4(xu)))))
 * All products are fp32 MFMA with fp32 accumulation, bias and relu fp32 op by op; xu is never written to memory (the kernel reads the
 * two source arrays).  hipets_critic_set: `ptrs` is a HOST table of HIPETS_CRITIC_N_PTRS DEVICE pointers to contiguous f32 tensors in
 * nn.Linear's layout -- linear1 .. linear6, weight then bias each; linear1 / linear4 [hidden, obs_dim + act_dim], linear2 / linear5
 * [hidden, hidden], linear3 / linear6 [1, hidden] -- which it copies into the engine's own packed layout (a SNAPSHOT: call it again
 * after the critic changed); it does not synchronise: the tensors must stay alive until the work enqueued on `stream` has run.
 * 1 <= obs_dim <= 512, 1 <= hidden <= 1024, 1 <= act_dim <= 32 (the HIPETS_POLICY_MAX_* limits), n_ptrs == HIPETS_CRITIC_N_PTRS, no
 * null pointer; anything else is HIPETS_ERR_INVALID_ARGUMENT and leaves the engine without a critic.                                */
#define HIPETS_CRITIC_N_PTRS 12
int hipets_critic_set(hipets_engine* e, int32_t obs_dim, int32_t act_dim, int32_t hidden, const void* ptrs, int32_t n_ptrs, void* stream);
/* One launch: obs DEVICE [batch, obs_dim], actions DEVICE [batch, act_dim] -> q1, q2, qmin DEVICE [batch] f32, each optional (NULL = not
 * wanted); batch >= 1.  qmin is torch.min(q1, q2) (sac.py:101) as a select without fminf: q1 where q1 < q2 or q1 is NaN, else q2 --
 * the smaller value, NaN when either is NaN (torch.min's rule; fminf would drop the NaN), q2's bits on a tie.
 * A row's arithmetic does not depend on the batch it arrives in: row r of any call equals the one-row call on (obs[r], actions[r]).   */
int hipets_critic_q(hipets_engine* e, const float* obs, const float* actions, int32_t batch, float* q1, float* q2, float* qmin, void* stream);
/* Launch geometry of hipets_critic_q for `batch` rows of the critic set last, the actor's rule (hipets_policy_geometry): a workgroup
 * owns 16 * row_tiles rows, row_tiles = the largest of 4, 2, 1 whose two activation buffers -- 16 rows x (max(pad16(obs_dim +
 * act_dim), pad16(hidden)) + pad16(hidden) + 8) floats per row tile; Q1 and Q2 run one after the other through the same buffers --
 * fit the LDS opt-in limit, no more than the batch needs; lds_bytes = its dynamic LDS.                                              */
int hipets_critic_geometry(hipets_engine* e, int32_t batch, int32_t* row_tiles, int32_t* lds_bytes);
/* hipets_trajectory_returns with a discount and an optional terminal value (POLO / LOOP / TD-MPC style planning: a short horizon plus
 * a learned tail).  rewards, dones, pop, horizon, num_particles, the outputs and the particle reduction as there; terminal_values
 * DEVICE [B] f32 or NULL.  Per row, for t = 0 .. H-1 in order, every line ONE float32 operation (no fused multiply-add):
 *     disc = 1; total = 0; terminated = false
 *     r = terminated ? 0 : rewards[t][row];  terminated |= dones[t][row] != 0
 *     total = total + disc * r;  disc = disc * gamma
 *   and, with terminal_values:  total = total + (terminated ? 0 : disc * terminal_values[row])
 * Both zeroings are selects.  A row that terminated at any step, the last included, gets no bootstrap.  With gamma == 1 and
 * terminal_values == NULL all three outputs are hipets_trajectory_returns' bits.  gamma outside [0, 1] or NaN is
 * HIPETS_ERR_INVALID_ARGUMENT.  Needs no model.                                                                                   */
int hipets_discounted_returns(hipets_engine* e, const float* rewards, const uint8_t* dones, const float* terminal_values, float gamma,
                              int32_t pop, int32_t horizon, int32_t num_particles, float* returns, float* row_totals, int32_t* first_done,
                              void* stream);

/* ---- ensemble predictions and uncertainty: what every member predicts for a batch, and how much they disagree ----
 * Additive entry points: the descriptor hipets_set_model takes, scalars and pointers; no struct changes, HIPETS_ABI_VERSION stays.
 *
 * GaussianMLP.forward(x, use_propagation=False) (mbrl/models/gaussian_mlp.py:140-154, 277-281), BasicEnsemble._default_forward
 * (basic_ensemble.py:94-99) and OneDTransitionRewardModel.forward over _get_model_input (one_dim_tr_model.py:103-116, 138-140): every
 * requested member's forward of the SAME rows in one launch.  All products are fp32 MFMA with fp32 accumulation; bias, activation
 * (every HIPETS_ACT_*, leaky_slope for LEAKY_RELU; SiLU and sigmoid through the hardware's exp2 and reciprocal, as the rollout
 * kernels compute them) and the head fp32 op by op.  The head is gaussian_mlp.py:150-153 literally:
 *     mean = out[..., :out_dim];  logvar = max_logvar - softplus(max_logvar - out[..., out_dim:]);  logvar = min_logvar + softplus(logvar - min_logvar)
 * with F.softplus's definition (beta 1, threshold 20); the bounds are per member for HIPETS_ENSEMBLE_BASIC and shared otherwise; a
 * deterministic model has no log-variance head.
 *
 * hipets_ensemble_set takes the descriptor of hipets_set_model / hipets_set_model_columns (cols / n_cols: the column table of a
 * HIPETS_OBS_COLUMNS model, NULL / 0 for every other obs_process) and keeps a SNAPSHOT of its own -- all ensemble_size members' weights
 * and biases, the normaliser, the bounds, the member list (the elite set), the column table -- apart from the rollout model: with or
 * without an ensemble snapshot every other call behaves as before, and the model set by hipets_set_model is not touched.  fp32 only:
 * HIPETS_PREC_BF16X3 / HIPETS_PREC_BF16 are refused, and so are ensemble_size > 16, in_dim > 512, out_dim > 512 (the
 * HIPETS_ENSEMBLE_MAX_* limits below), hid > HIPETS_POLICY_MAX_HIDDEN and a shape whose LDS need at one row tile -- 16 rows x (pad16(in_dim) + 4 [the kept input] + pad16(hid) + 4 +
 * max(pad16(hid), pad16(out_total)) + 4 [the two activation buffers] + 2 out_dim [the per-row accumulators]) floats -- exceeds the LDS
 * opt-in limit (HIPETS_ERR_INVALID_ARGUMENT).  The reward / termination fields of the descriptor are not read.  A refused set leaves the
 * engine without an ensemble.  Synchronises `stream` before it returns.                                                              */
#define HIPETS_ENSEMBLE_MAX_MEMBERS 16
#define HIPETS_ENSEMBLE_MAX_IN 512
#define HIPETS_ENSEMBLE_MAX_OUT 512
int hipets_ensemble_set(hipets_engine* e, const hipets_model_desc* desc, const hipets_obs_column* cols, int32_t n_cols, void* stream);
/* One launch over `batch` >= 1 rows and n members: all ensemble_size members in index order (only_elite == 0), or the n_members of the
 * descriptor's member list in list order.  The model input is EITHER built from obs DEVICE [batch, obs_dim] and actions DEVICE [batch,
 * act_dim] -- obs_process, concatenation, the normaliser in the descriptor's dtype (HIPETS_NORM_F64: (x - mean) * (1 / std) in f64, as
 * the rollout kernels form it) -- with model_in NULL, OR read from model_in DEVICE [batch, in_dim] (what forward(x) takes) with obs and
 * actions NULL; it is built once per workgroup and kept for all members.  Outputs, DEVICE f32, each optional (NULL = not wanted; all
 * NULL is an error, and so is logvar for a deterministic model):
 *   mean [n, batch, out_dim], logvar [n, batch, out_dim]
 *   stats [batch, 4], reduced over the n members and all out_dim columns inside the launch:
 *     [0] max_std       = max_m sqrt(sum_d exp(logvar[m, d]))            (MOPO's penalty; 0 for a deterministic model)
 *     [1] disagreement  = sqrt(sum_d Var_m(mean[m, d]))                  (population variance: divided by n)
 *     [2] total_std     = sqrt(sum_d (Var_m(mean[m, d]) + mean_m exp(logvar[m, d])))   (the mixture's predictive std; = [1] if deterministic)
 *     [3] max_deviation = max_m sqrt(sum_d (mean[m, d] - mean[0, d])^2)  (the farthest member from the first requested one: a one-pass
 *                         discrepancy in the spirit of MOReL's)
 *   The variance is accumulated about the first requested member's mean (shifted sums), never as E[x^2] - E[x]^2 of the raw means.
 * A row's arithmetic depends neither on the batch it arrives in, nor on the row tiles of the launch, nor on which outputs are
 * requested; a NaN or inf in a row stays in that row (the two maxima follow torch.max: a NaN wins).                                  */
int hipets_ensemble_predict(hipets_engine* e, const float* obs, const float* actions, const float* model_in, int32_t batch, int32_t only_elite,
                            float* mean, float* logvar, float* stats, void* stream);
/* Launch geometry of hipets_ensemble_predict for `batch` rows of the ensemble set last, the actor's rule (hipets_policy_geometry): a
 * workgroup owns 16 * row_tiles rows, row_tiles = the largest of 4, 2, 1 whose LDS need (hipets_ensemble_set) fits the opt-in limit, no
 * more than the batch needs; lds_bytes = its dynamic LDS.                                                                            */
int hipets_ensemble_geometry(hipets_engine* e, int32_t batch, int32_t* row_tiles, int32_t* lds_bytes);
/* An uncertainty penalty and halt on a model step's rewards and dones (MOPO's r - lambda u; MOReL's halt): one elementwise launch over
 * stats DEVICE [batch, 4] (hipets_ensemble_predict), rewards DEVICE [batch] f32 and dones DEVICE [batch] uint8, both updated in place.
 * Per row, every line ONE float32 operation (no fused multiply-add), with u = stats[row * 4 + stat] (stat in 0 .. 3):
 *     p = coef * u;  rewards[row] = rewards[row] - p
 *     if halt_threshold is not NaN and u > halt_threshold:  dones[row] = 1, and with use_halt_reward: rewards[row] = halt_reward
 * A NaN u never halts; it makes the reward NaN through the subtraction (coef * NaN is NaN, for coef == 0 too).  dones may be NULL when
 * halt_threshold is NaN.  Needs no model.                                                                                                                    */
int hipets_uncertainty_penalty(hipets_engine* e, const float* stats, int32_t stat, float coef, float halt_threshold, float halt_reward,
                               int32_t use_halt_reward, int32_t batch, float* rewards, uint8_t* dones, void* stream);

/* ---- policy rollouts: the SAC actor rolled through the dynamics ensemble, the action sequences that seed a plan ----
 * Additive entry points: scalars and pointers; no struct changes, HIPETS_ABI_VERSION stays.  They read the snapshots hipets_policy_set
 * and hipets_ensemble_set hold and need no set call of their own.
 *
 * hipets_policy_rollout: ONE launch rolls n rows through `horizon` steps.  Row r at step t = 0 .. horizon - 1:
 *   a_t     = GaussianPolicy(s_t) exactly as hipets_policy_act computes it: the mean action tanh(mean) * scale + bias for rows r < mean_rows,
 *             tanh(mean + exp(log_std) * eps) * scale + bias for the others, eps from the table eps DEVICE [horizon, n, act_dim] or, with
 *             eps NULL, drawn in-kernel as hipets_policy_act draws row t * n + r under (seed, stream_id): hipets_policy_normals(batch =
 *             horizon * n) returns exactly that table.
 *   x       = the model input of (s_t, a_t) exactly as hipets_ensemble_predict builds it (obs_process including column tables,
 *             concatenation, the normaliser in its own dtype).
 *   pred    = the mean over the requested members -- the descriptor's member list in list order (only_elite != 0; all members where the
 *             model has no elite set, as for HIPETS_ENSEMBLE_BASIC) or all ensemble_size members in index order -- of each member's MEAN
 *             head, with the bits hipets_ensemble_predict gives: fp32, acc = m_0; acc += m_i in requested order; one division by the count.
 *             (propagation "expectation" with ModelEnv.step(..., sample=False): gaussian_mlp.py:213-215, basic_ensemble.py:131-136.)
 *   s_{t+1} = one_dim_tr_model.py:281-286: the learned-reward column (the last) is dropped; s_t + pred under target_is_delta except the
 *             no_delta dims, which take pred; otherwise pred.  No termination test; NaN and inf propagate within their row.
 * Outputs, DEVICE f32: actions [n, horizon, act_dim]; states [horizon + 1, n, obs_dim] (states[0] = s0) or NULL.  s0 DEVICE [n, obs_dim].
 * A workgroup owns 16 * row_tiles consecutive rows for the whole horizon and never waits for another.  A row's arithmetic depends
 * neither on n nor on the row tiles; only its in-kernel draws do (they are keyed on t * n + r).
 * HIPETS_ERR_INVALID_ARGUMENT, each with a message: no policy snapshot or no ensemble snapshot; the policy's (obs_dim, act_dim) differs
 * from the ensemble's; the ensemble's out_dim is not obs_dim + learned_rewards; n < 1; horizon < 1; horizon * n > 2^31 - 1; mean_rows outside
 * [0, n]; a pair of snapshots whose LDS need at one row tile -- 16 rows x (pad16(obs_dim) + 4 [the state] + act_dim rounded up to 4 + the larger of
 * the actor's two buffers (pad16(hidden) + 4 + max(pad16(hidden), pad16(2 act_dim)) + 4) and the model's areas (hipets_ensemble_set's input and
 * two buffers + out_dim [the members' sum])) floats -- exceeds the LDS opt-in limit (the message names the bytes).                            */
int hipets_policy_rollout(hipets_engine* e, const float* s0, int32_t n, int32_t horizon, int32_t mean_rows, int32_t only_elite, uint64_t seed,
                          uint64_t stream_id, const float* eps, float* actions, float* states, void* stream);
/* Launch geometry of hipets_policy_rollout for n rows, the actor's rule (hipets_policy_geometry) on the LDS need above; the same refusals
 * about the snapshots.                                                                                                                */
int hipets_policy_rollout_geometry(hipets_engine* e, int32_t n, int32_t* row_tiles, int32_t* lds_bytes);

/* ---- instrumentation (bench.py roofline leg) ----------------------------------------------- */
/* on = 1: every rollout-kernel launch carries a start / stop hipEvent pair on its dispatch packet; on = k > 1: every
 * k-th launch does (a completion signal per packet costs a few microseconds between back-to-back short launches -- the
 * per-step launches of DEVICE mode -- so bench.py samples them); on = 0: off.                                      */
int hipets_timing_enable(hipets_engine* e, int32_t on);
/* Synchronises the recorded events; returns number of launches and their summed duration.       */
int hipets_timing_read(hipets_engine* e, int64_t* launches, double* total_ms, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* HIPETS_H */
