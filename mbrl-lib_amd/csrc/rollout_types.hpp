// rollout_types.hpp -- the argument structs host and device share: the packed-layer table (LayerMeta), the model on the device
// (ModelDev), the arguments of one rollout launch (RolloutArgs), a wave's leftover GEMM units (Extras) and the "head pair" column
// order of the output layer's second pack.  ModelDev stands for what the reference keeps in GaussianMLP / OneDTransitionRewardModel /
// ModelEnv attributes (mbrl/models/gaussian_mlp.py:69-127, one_dim_tr_model.py:73-101, model_env.py:37-60); RolloutArgs for the
// arguments of ModelEnv.evaluate_action_sequences (model_env.py:145-191).
#pragma once
#include "common.hpp"

namespace hipets {

struct LayerMeta {
    int Kp, Np;          // K, N padded to multiples of 16
    int boff;            // float offset of the layer's bias inside a member block
    int tail_steps;      // MFMA k-steps (of 4) of the last chunk that hold real weights: ceil((K - (Kp - 16)) / 4)
    long long woff;      // float offset of the layer's packed weights inside a member block
    // bf16x3 / bf16 precision modes (operands as three bf16 pieces, or one, on the bf16 matrix pipe):
    int Kp32;            // K padded to a multiple of 32 (one v_mfma_f32_16x16x32_bf16 k-chunk)
    int pad_;
    long long woff3;     // 16-byte-unit offset of the layer's packed bf16 planes inside a member block
    // output layer of a stochastic model only: a SECOND pack of its weights / biases with the columns in "head pair" order
    // (head_pair_col below) for the kernel instances that sample straight from the accumulators (KSpec::FUSE); -1 = none
    long long woff_pairs;
    int boff_pairs;
    int pad2_;
};

// "Head pair" column order of the output layer (mean_and_logvar, gaussian_mlp.py:107-112): packed column p = 16 c + 4 g + i
// holds, for the output dim d = 8 c + 2 g + (i & 1), its mean (i < 2) or its log-variance (i >= 2).  Formed transposed, the
// product leaves lane group g of column tile c with {mean d, mean d+1, logvar d, logvar d+1} of one batch row in ONE
// accumulator: everything the sampling of those two dims needs (model.py:471-473), no LDS round trip.  -1 = zero padding.
__host__ __device__ __forceinline__ int head_pair_col(int p, int out_dim) {
    const int c = p >> 4, g = (p >> 2) & 3, i = p & 3;
    const int d = 8 * c + 2 * g + (i & 1);
    if (d >= out_dim) return -1;
    return i < 2 ? d : out_dim + d;
}

struct Extras {  // up to kMaxExtras leftover (column tile, row tile) units of one wave
    int c0, c1, c2, c3, r0, r1, r2, r3;
};

// The parametric closed forms of a model (include/hipets.h HIPETS_REW_TERMS / HIPETS_TERM_BOX), as hipets_set_model leaves them in
// engine-owned device memory: one block, read with plain loads at wave-uniform addresses by the one thread per row that evaluates
// reward and termination in the non-lean tail (closed_forms.hpp).  Never staged in LDS: the LDS layout does not know them.
struct FormTables {
    int n_terms, n_intervals, require_finite;
    float bias, alive_bonus;
    int grouped;  // HIPETS_REW_TERMS: some entry has a level, an op, a source or a function beyond the flat sum of ABI v9 (reward_eval picks its loop by it)
    int pad_[2];
    hipets_reward_term terms[HIPETS_MAX_REWARD_TERMS];
    hipets_term_interval intervals[HIPETS_MAX_TERM_INTERVALS];
};

struct ModelDev {
    int obs_dim, act_dim, in_dim, out_dim, out_total, hid, n_layers, M;
    int obs_in;  // width of obs_process_fn(obs) = in_dim - act_dim
    int activation;
    float slope;
    int propagation, deterministic, obs_process, reward_fn, term_fn, target_is_delta, learned_rewards, normalizer;
    const LayerMeta* layers;  // DEVICE [n_layers] (a table in memory: runtime-indexed kernargs would go to scratch), followed by the model's
                              // FormTables where reward_fn is HIPETS_REW_TERMS or term_fn HIPETS_TERM_BOX (form_tables below), and by its
                              // column table where obs_process is HIPETS_OBS_COLUMNS (obs_columns below)
    int Kp0;                  // padded input width of layer 0
    int hidC;                 // column tiles of a hidden layer (cost model; shape of the lean kernel instances)
    int outC;                 // column tiles of the output layer
    long long wmember;  // floats per member (packed weights)
    int bmember;        // floats per member (padded biases)
    int ld;             // LDS activation row stride in floats (== 8 mod 64)
    int ld_in;          // KSpec::WIDE instances: row stride of the model-input image (>= Kp0, == 8 mod 64); the hidden activations use KSpec::LD
    const float* w;
    const float* b;
    const double* norm_mean;
    const double* norm_std;
    const float* min_lv;  // [lv_rows][out_dim]
    const float* max_lv;
    int lv_rows;          // 1 (bounds shared by the members) or M (BasicEnsemble: one row per member)
    int iid_members;      // BasicEnsemble: members are drawn independently (no balanced shuffle, no batch % M rule)
    const unsigned char* no_delta;  // [obs_dim]
    int precision;            // HIPETS_PREC_*
    long long w3member;       // 16-byte units per member (bf16 planes: three in bf16x3, one in bf16)
    const uint4* w3;          // packed bf16 planes: [member][layer][col tile][k chunk of 32][plane 0..NP-1][lane][8 x bf16]
};

// The model's FormTables: hipets_set_model stores them right behind the layer table, in the same device block.  (No pointer of their own
// in ModelDev: the kernel-argument layout of every rollout-kernel instance stays what it was.)
__host__ __device__ __forceinline__ const FormTables* form_tables(const ModelDev& md) {
    return reinterpret_cast<const FormTables*>(md.layers + md.n_layers);
}

// The column table of a HIPETS_OBS_COLUMNS model ([obs_in] entries: column k of obs_process_fn(obs) is fn_k(obs[dim_k])):
// hipets_set_model_columns stores it behind the FormTables, in the same device block, for the same reason.  Read with plain global
// loads by build_input_impl (at most 4 KB, hot in cache); never staged in LDS: the LDS layout does not know it.
__host__ __device__ __forceinline__ const hipets_obs_column* obs_columns(const ModelDev& md) {
    return reinterpret_cast<const hipets_obs_column*>(form_tables(md) + 1);
}

struct RolloutArgs {
    int pop, P, H, B;
    int whole_horizon;  // the kernel form: 1 = FAST (one launch for the horizon, rows tiled from s0, state in LDS); 0 = step-synchronous
                        //   (rows by identity / permutation, state in HBM around the launch, or handed over in the persistent form)
    int t_begin, t_end;
    int groups;           // FAST: candidate groups per particle; EXACT: workgroups per member domain
    int rows_per_domain;  // EXACT: B / M (or B for expectation)
    const float* actions;  // [pop,H,A]
    const float* s0;       // [obs]
    float* state;          // EXACT: [B,obs] in/out
    float* totals;         // [B] (EXACT in/out; FAST out)
    unsigned char* term;   // EXACT: [B] in/out
    const long long* perm; // EXACT: [H,B] / [B] / null
    long long perm_step;   // stride between steps (0 for fixed_model)
    unsigned perm_n, perm_a, perm_b;  // DEVICE mode: row of slot j = perm_apply(j) over [0, perm_n), radices a x b (perm_n = 0: none)
    PermKeys perm_keys;    // DEVICE mode: round keys of THIS launch's permutation (perm_round_keys(perm_key(seed, stream, step)), host side)
    const float* eps;      // [H,B,out] or null
    int use_philox;        // FAST without eps override
    unsigned long long seed, stream_id;
    const int* schedule;   // FAST: [H, nWG] member slot per (step, workgroup), injected by the caller; null = every workgroup draws its own
                           //   entries in its prologue (common.hpp fast_member, radices fm_a x fm_b = perm_radices(gridDim.x))
    unsigned fm_a, fm_b;
    int fast_members;      // the step-synchronous form (whole_horizon = 0) with the workgroup's member chosen as in FAST mode (`schedule`,
                           //   or the in-kernel draw for step t_begin): hipets_step in FAST mode -- for one step that form IS the FAST form,
                           //   and it exists in every shape-specialised instance
    float* trace_next_obs;
    float* trace_rewards;
    long long* phase_cycles;  // optional [kWaves][16 phases] cycle counters of workgroup 0 (profiling aid)
    int pop_env;               // FAST batched planning: candidates per environment (candidate c starts from s0[c / pop_env]); 0 = one env
    int generic_only;          // hipets_rollout_opts.generic_kernel: 1 = only the fully generic kernel instance; 2 = no shape-specialised
                               // (lean) instance, but the hidden-static one (KSpec::HID_STATIC) where the model has its width
    int wide_lds;              // the host sized the LDS (and chose R) for the KSpec::WIDE layout: the launcher runs that instance or fails
    // DEVICE mode, persistent form (all workgroups co-resident, ONE launch for the horizon): rows change workgroups every step
    // through `exchange`, a [B][obs_dim + 2] table of 8-byte {value bits, step tag} granules (state dims, running total,
    // terminated flag).  A granule is written by ONE write-through (sc1) 8-byte store and polled with sc1 loads until its
    // tag is the awaited step: self-validating, so no fence, flag or grid barrier is involved (MI355X_MICROARCH.md R2).
    unsigned long long* exchange;  // null: per-step launches
    unsigned tag_base;             // step t's hand-over carries tag tag_base + t + 1 (the engine advances it by H per launch: no clearing)
    int resident_heads;            // HOST only (launch.hpp resident_heads_call; no kernel reads it): the call is a straight persistent launch -- as
                                   // many launched as logical workgroups -- and asks for the KSpec::RES instance of its shape
    int layout_pad_unused[2];      // never read or written: keeps the later fields at their kernarg offsets (profiles/one_launch_path.json)
    int n_logical;                 // persistent form: logical workgroups (member domain x row group); a launched workgroup serves the
                                   // logical ones wg, wg + gridDim.x, ... one after the other within every step (batches larger than the chip)
    int ragged_last_turn;          // persistent form, KSpec::WIDE two-tile instances: when the row tiles the LAST turn of a step would serve
                                   // fit one per launched workgroup, that turn is dealt in ONE-tile logical workgroups (rollout_kernel:
                                   // "ragged last turn"); 0 = always two-tile turns (A/B measurements: HIPETS_RAGGED_LAST_TURN=0)
    const PermKeys* step_keys;     // DEVICE [H]: round keys of every step's permutation
    int* error_flag;               // HOST-mapped: set to 1 when a poll exceeds its bound (another workgroup was not resident); once it is
                                   // set every later poll of the launch gives up after <= 64 spins, so a stranded grid drains in
                                   // milliseconds instead of waiting out the bound at every step and turn
    long long poll_ticks;          // bound of one hand-over poll in 100 MHz wall-clock ticks (hipets_set_handover_timeout; default 0.2 s)
    unsigned lds_bytes;            // the dynamic LDS size the launch was given (debug builds check every LDS section against it: HIPETS_DEBUG_BOUNDS)
    int* census;                   // DEVICE [2], launcher only: when set the launch is the co-residency SELF-TEST of this kernel instance at
                                   // this grid, not a rollout -- every workgroup arrives at census[0] and waits (bounded by poll_ticks)
                                   // until all gridDim.x have; those that saw everybody count themselves in census[1]
};

}  // namespace hipets
