// rollout_smem.hpp -- the dynamic-LDS layout of the rollout kernel, written once (HIPETS_ROLLOUT_SECTIONS): the kernel's section
// pointers (RolloutSmem), its carving of the launch's LDS and the size the host gives the launch (rollout_smem_bytes) all expand it.
// Replaces nothing in the reference: these are the tensors ModelEnv.evaluate_action_sequences (mbrl/models/model_env.py:145-191)
// keeps in HBM between its ATen launches, held on chip for the rows of one workgroup.
#pragma once
#include "common.hpp"
#include "rollout_types.hpp"

namespace hipets {

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// one activation buffer of `rows` rows of stride ld floats; buf0 + buf1 are contiguous (the bf16 instances clear both at once, the WIDE
// ones stage hand-over pairs in them)
__host__ __device__ inline size_t act_buf_bytes(int rows, int ld) { return align16((size_t)rows * ld * 4); }
__host__ __device__ inline size_t act_bytes(int rows, int ld0, int ld) { return act_buf_bytes(rows, ld0) + act_buf_bytes(rows, ld); }
// KSpec::WIDE instances collect a turn's rows by LDS-DMA (rollout_kernel, "dma_collect"): rows x pairs 16-byte hand-over pairs staged
// in 1 KiB chunks of 64.  The two activation buffers are idle then and hold most of them; what does not fit gets a section of its own.
__host__ __device__ inline size_t stage_extra_bytes(int rows, int ld0, int ld, int obs_dim) {
    const size_t nvp = (size_t)(obs_dim + 1) / 2 + 1;            // pairs per row
    const size_t need = (size_t)rows * ((nvp + 63) / 64) * 1024;  // every row's pairs in whole chunks of 64 (dma_collect)
    const size_t have = act_bytes(rows, ld0, ld);
    return need > have ? need - have : 0;
}

// THE layout: X(element type, name, bytes) for every section, in order.  The kernel's pointers, its carving and the host's launch size
// are expansions of this one table, so they cannot disagree.  Its other arguments are the expressions the sizes depend on -- rows per
// workgroup; ld0 / ld, the row strides of buf0 / buf1 in floats (they differ in the KSpec::WIDE layout only: buf0 holds the model-input
// image); the model's dimensions; the horizon; expectation propagation (generic instances); wide, the KSpec::WIDE layout -- and are
// evaluated where a size uses them (the kernel's loads of the model's dimensions stay where the carving needs them).
// Every size is a multiple of 16 bytes.  Sections whose size follows from the row count and the row strides come first: in a
// shape-specialised instance (compile-time stride) their addresses are constants -- immediate offsets in the LDS instructions instead
// of a live SGPR each (the DEVICE instance of cfg2 spills > 200 scalars); the sections sized by the model's run-time dimensions follow.
#define HIPETS_ROLLOUT_SECTIONS(X, rows, ld0, ld, obs_dim, act_dim, in_dim, lv_rows, out_dim, out_total, horizon, expectation, wide)                  \
    X(float, buf0, act_buf_bytes((rows), (ld0)))                                    /* [rows][ld0] activations (WIDE: the model-input image) */       \
    X(float, buf1, act_buf_bytes((rows), (ld)))                                     /* [rows][ld] activations */                                      \
    X(float, tot, align16((size_t)(rows) * 4))                                      /* [rows] running totals */                                       \
    X(float, lrew, align16((size_t)(rows) * 4))                                     /* [rows] learned reward of the current step */                   \
    X(int, term, align16((size_t)(rows) * 4))                                       /* [rows] terminated flags */                                     \
    X(int, rowid, align16((size_t)(rows) * 4))                                      /* [rows] global row id (candidate*P + particle) or -1 */         \
    X(int, pend, align16((size_t)2 * (rows) * 4))                                   /* [2][rows] persistent DEVICE form: running total / flag granule of the row not yet collected */\
    X(LayerMeta, lmeta, align16(sizeof(LayerMeta) * HIPETS_MAX_LAYERS))             /* [HIPETS_MAX_LAYERS] */                                         \
    X(long long, prof, align16((size_t)kWaves * 16 * 8))                            /* [kWaves][16] phase-cycle accumulators (profiling aid) */       \
    X(float, dump, 16)                                                              /* [4] sink of the fused tail's masked-off LDS stores (branch-free: an inactive lane stores here) */\
    X(float, part, (rows) == kTile ? (size_t)2 * kWaves * 64 * 16 : 0)              /* one-tile workgroups: [2][kWaves][64][4] k-split partial sums (KsArgs) */\
    X(float, state, align16((size_t)(rows) * (obs_dim) * 4))                        /* [rows][obs_dim] */                                             \
    X(float, actn, align16((size_t)2 * (rows) * (act_dim) * 4))                     /* [2][rows][act_dim] (double buffered: reward(t) reads while input(t+1) is built) */\
    X(double, nmean, align16((size_t)(in_dim) * 8))                                 /* [in_dim] normaliser stats (f64 like the reference) */          \
    X(double, nstd, align16((size_t)(in_dim) * 8))                                  /* [in_dim] (f64 normaliser: holds 1 / std) */                    \
    X(float, minlv, align16((size_t)(lv_rows) * (out_dim) * 4))                     /* [lv_rows][out_dim] */                                          \
    X(float, maxlv, align16((size_t)(lv_rows) * (out_dim) * 4))                     /* [lv_rows][out_dim] */                                          \
    X(int, nodelta, align16((size_t)(obs_dim) * 4))                                 /* [obs_dim] */                                                   \
    X(int, sched, align16((size_t)(horizon) * 4))                                   /* [H] member slot of this workgroup per step (FAST) */           \
    X(float, expacc, (expectation) ? align16((size_t)(rows) * (out_total) * 4) : 0) /* [rows][out_total] (expectation propagation only) */            \
    X(char, stage_x, (wide) ? stage_extra_bytes((rows), (ld0), (ld), (obs_dim)) : 0)/* KSpec::WIDE: the chunks of the hand-over staging area that do not fit buf0 + buf1 */

// (expansions that use the names only, not the sizes)
#define HIPETS_ROLLOUT_SECTION_NAMES(X) HIPETS_ROLLOUT_SECTIONS(X, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)

struct RolloutSmem {
#define HIPETS_SECTION_POINTER(T, name, bytes) T* name;
    HIPETS_ROLLOUT_SECTION_NAMES(HIPETS_SECTION_POINTER)
#undef HIPETS_SECTION_POINTER
};

// expacc and stage_x MUST stay the last two rows of the table.  No kernel has both (expectation propagation: generic instances; the
// staging chunks: WIDE ones) and nothing follows them, so the kernel's carving starts both at the same address and never sizes them
// (rollout_kernel); a section appended behind them would be misplaced there.
enum RolloutSection {
#define HIPETS_SECTION_INDEX(T, name, bytes) SEC_##name,
    HIPETS_ROLLOUT_SECTION_NAMES(HIPETS_SECTION_INDEX)
#undef HIPETS_SECTION_INDEX
    kRolloutSections
};
static_assert(SEC_expacc == kRolloutSections - 2 && SEC_stage_x == kRolloutSections - 1, "expacc and stage_x are the last two sections");

// dynamic LDS of a launch with `rows` rows per workgroup.  ld0 > 0: the KSpec::WIDE layout, buf0 with its own row stride ld0
__host__ __device__ inline size_t rollout_smem_bytes(int rows, int ld, int obs_dim, int act_dim, int in_dim, int out_dim,
                                                     int out_total, int horizon, bool expectation, int lv_rows = 1, int ld0 = 0) {
    size_t n = 0;
#define HIPETS_SECTION_SIZE(T, name, bytes) n += (bytes);
    HIPETS_ROLLOUT_SECTIONS(HIPETS_SECTION_SIZE, rows, (ld0 > 0 ? ld0 : ld), ld, obs_dim, act_dim, in_dim, lv_rows, out_dim, out_total, horizon, expectation, ld0 > 0)
#undef HIPETS_SECTION_SIZE
    return n;
}

}  // namespace hipets
