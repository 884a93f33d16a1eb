// launch.hpp -- host entry points of the kernels that live in their own translation units (rollout_r<R>.hip, planet.hip):
// the rollout kernel is instantiated per row-tile count R and activation, and the instantiations compile in parallel.
#pragma once
#include <hip/hip_runtime.h>

#include "kspec.hpp"
#include "lds_optin.hpp"
#include "planet_types.hpp"
#include "residency_rule.hpp"
#include "rollout_types.hpp"

namespace hipets {

// One instance of rollout_kernel<R, ...> as the host sees it: the address hipLaunchKernel takes and the instance's LDS opt-in flags
// (residency.hpp launches it and keeps what is known about its residency), and per row-tile count R the resolver that hands out the record
// of the instance pick_rollout_instance (below) names: nullptr with *why = hipErrorNotSupported / hipErrorInvalidConfiguration for a refusal.
struct KernelRec {
    const void* fn;
    LdsOptIn lds;
};
constexpr int kMaxR = 4;  // row-tile counts 1..kMaxR
KernelRec* rollout_instance_r1(const ModelDev& md, const RolloutArgs& ra, hipError_t* why);
KernelRec* rollout_instance_r2(const ModelDev& md, const RolloutArgs& ra, hipError_t* why);
KernelRec* rollout_instance_r3(const ModelDev& md, const RolloutArgs& ra, hipError_t* why);
KernelRec* rollout_instance_r4(const ModelDev& md, const RolloutArgs& ra, hipError_t* why);

// Hidden widths with a KSpec::HID_STATIC instance (hidden layers shape-specialised, everything else generic): X(hidden column tiles).
// 13 tiles = hidden widths 193..208: the reference's default of 200 (conf/dynamics_model/gaussian_mlp_ensemble.yaml:8), which every
// configuration it ships uses.  (Rounds 4-5 also instantiated 8 and 16 tiles -- hid 113..128, 241..256: + 2-10 % over the generic
// instance, profiles/r4_hidden_widths.json -- for widths no shipped configuration or BASELINE config has; round 6 dropped those eight
// instances from the build: other widths run the generic instance, same bits.)
#define HIPETS_HID_STATIC_SHAPES(X) X(13)

// Shape-specialised ("lean") fp32 instances per row-tile count R: X(hidden column tiles, output column tiles, reward fn, termination
// fn, obs preprocessing); all of them SiLU, f64 normaliser, stochastic GaussianMLP with in-kernel sampling.  R follows the cost
// model's choice for the configuration (rollout.hip choose_R, which in turn knows this table: lean_shape_exists):
//   BASELINE.json: cfg1 cartpole R = 1, cfg2 / cfg3 R = 3 (a rank's shard of a strong-scaled plan: 1, 2), cfg4 R = 3 at its first
//   iteration and 2 / 4 as the iCEM population decays, cfg4' Humanoid-v4 R = 2 (small batches 1; KSpec::WIDE), cfg5 (2500 row tiles) 2;
//   the workloads the reference ships (round 4): pets_halfcheetah (conf/overrides/pets_halfcheetah.yaml: obs 18 through
//   HalfCheetahEnv.preprocess_fn, pop 400 x 20) R = 2 in DEVICE mode, 1 in FAST mode; pets_cartpole (pop 350 x 20) R = 1, 2;
//   pets_cartpole_paper_version (cartpole_pets reward + CartPoleEnv.preprocess_fn, pop 500 x 20) R = 3.
//   learned rewards + no_termination (pets_pusher 20 / 7, pets_reacher 17 / 7: pop 350 x 20; pets_mppi_halfcheetah: obs 18 through
//   preprocess_fn, MPPI 350 x 20): output layers of 3 column tiles like cfg2's, R = 2 in DEVICE mode, 1 in FAST mode.
#define HIPETS_LEAN_SHAPES_R1(X)                                                                                                               \
    X(13, 1, HIPETS_REW_CARTPOLE, HIPETS_TERM_CARTPOLE, HIPETS_OBS_NONE) X(13, 47, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_HUMANOID, HIPETS_OBS_NONE) \
    X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE, HIPETS_OBS_NONE) X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE, HIPETS_OBS_HALFCHEETAH) \
    X(13, 3, HIPETS_REW_LEARNED, HIPETS_TERM_NONE, HIPETS_OBS_NONE) X(13, 3, HIPETS_REW_LEARNED, HIPETS_TERM_NONE, HIPETS_OBS_HALFCHEETAH) \
    X(13, 2, HIPETS_REW_LEARNED, HIPETS_TERM_HOPPER, HIPETS_OBS_NONE)
#define HIPETS_LEAN_SHAPES_R2(X)                                                                                                               \
    X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE, HIPETS_OBS_NONE) X(13, 47, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_HUMANOID, HIPETS_OBS_NONE) \
    X(13, 6, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_HUMANOID, HIPETS_OBS_NONE) X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE, HIPETS_OBS_HALFCHEETAH) \
    X(13, 1, HIPETS_REW_CARTPOLE, HIPETS_TERM_CARTPOLE, HIPETS_OBS_NONE)                                                                        \
    X(13, 3, HIPETS_REW_LEARNED, HIPETS_TERM_NONE, HIPETS_OBS_NONE) X(13, 3, HIPETS_REW_LEARNED, HIPETS_TERM_NONE, HIPETS_OBS_HALFCHEETAH) \
    X(13, 2, HIPETS_REW_LEARNED, HIPETS_TERM_HOPPER, HIPETS_OBS_NONE)
//   pets_inv_pendulum (learned reward + the inverted_pendulum termination function, obs 4 / act 1, pop 480 x 20): R = 3.
#define HIPETS_LEAN_SHAPES_R3(X)                                                                                                               \
    X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE, HIPETS_OBS_NONE) X(13, 6, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_HUMANOID, HIPETS_OBS_NONE) \
    X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE, HIPETS_OBS_HALFCHEETAH) X(13, 1, HIPETS_REW_CARTPOLE_PETS, HIPETS_TERM_NONE, HIPETS_OBS_CARTPOLE_PETS) \
    X(13, 1, HIPETS_REW_LEARNED, HIPETS_TERM_INVERTED_PENDULUM, HIPETS_OBS_NONE)
#define HIPETS_LEAN_SHAPES_R4(X) X(13, 6, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_HUMANOID, HIPETS_OBS_NONE)
// (every shape of these tables is instantiated in both launch modes: the FAST instances -- rollout_r<R>_fast.hip -- and the
// step-synchronous ones cover the same shapes)

// bf16x3 precision instances per R: X(hidden column tiles, output column tiles, reward fn, termination fn); no obs preprocessing
// (round 6: the R = 1 instances -- cfg1, and a rank's shard of a strong-scaled cfg2 plan, in an arithmetic mode that is reported
// separately and parked -- are gone from the build too: four instances; the mode runs R = 3 instances or raises)
#define HIPETS_B3_SHAPES_R1(X)
// (round 5: the R = 2 instances are gone -- two workgroups per CU cap a wave at 256 registers, the three-piece fragments did not fit and
// the two instances spilt 6 / 41 VGPRs to scratch, the only rollout kernels that did; the row-tile rule chooses among R = 1 and 3 for
// this arithmetic mode, rollout.hip choose_R)
#define HIPETS_B3_SHAPES_R2(X)
#define HIPETS_B3_SHAPES_R3(X) X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE) X(13, 6, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_HUMANOID)
#define HIPETS_B3_SHAPES_R4(X)

// bf16 precision instances per R (HIPETS_PREC_BF16: one bf16 piece per operand, one MFMA per block), same row format; the two shapes
// bf16x3 has, at R = 3.  (One-plane rows make R = 4 fit in LDS and R = 2 the register file: no such instance until a measurement asks for it.)
#define HIPETS_BF16_SHAPES_R1(X)
#define HIPETS_BF16_SHAPES_R2(X)
#define HIPETS_BF16_SHAPES_R3(X) X(13, 3, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_NONE) X(13, 6, HIPETS_REW_HALFCHEETAH, HIPETS_TERM_HUMANOID)
#define HIPETS_BF16_SHAPES_R4(X)

// what the fused tail's reward / termination lane can see of THIS model: termination functions that test every state dim need all of them
// among the four it holds; a learned reward next to a termination function comes from another lane of the same accumulator (column
// tile 0 holds output columns 0..7)
inline bool fused_term_ok(const ModelDev& md) {
    if (md.term_fn == HIPETS_TERM_INVERTED_PENDULUM && md.obs_dim > 4) return false;
    if (md.term_fn == HIPETS_TERM_HOPPER) return md.reward_fn == HIPETS_REW_LEARNED;  // every lane judges its own dims (FAST instances, KSpec)
    if (md.reward_fn == HIPETS_REW_LEARNED && md.term_fn != HIPETS_TERM_NONE && md.obs_dim >= 8) return false;
    return true;
}

// the model-side facts every shape-specialised instance (lean fp32, bf16x3 and bf16) was compiled for; the lean ones add fp32 arithmetic
// (lean_shape), the call adds its own (lean_call)
inline bool spec_model(const ModelDev& md) {
    return md.activation == HIPETS_ACT_SILU && md.normalizer == HIPETS_NORM_F64 && !md.deterministic && md.propagation != HIPETS_PROP_EXPECTATION &&
           md.lv_rows == 1 && fused_term_ok(md);
}

// does the call use nothing a shape-specialised instance compiled out? (KSpec in kspec.hpp lists what that is; the obs preprocessing
// is part of an instance's shape since round 4)
inline bool lean_call(const ModelDev& md, const RolloutArgs& ra) {
    return !ra.generic_only && spec_model(md) && !ra.eps && ra.use_philox &&
#if defined(HIPETS_STEP_TRACE) || (defined(HIPETS_LEAN_PROF) && HIPETS_LEAN_PROF)
           !ra.trace_next_obs && !ra.trace_rewards && ra.pop_env == 0;  // the stamps go to phase_cycles
#else
           !ra.trace_next_obs && !ra.trace_rewards && !ra.phase_cycles && ra.pop_env == 0;
#endif
}

// the lean fp32 instance X(hc, oc, rw, tm, ob) of the tables above, as rollout_inst.inc instantiates it for launch mode KMODE
template <int HC, int OC, int RW, int TM, int OB, int KMODE, int RES = 0>
using LeanSpec = KSpec<HIPETS_ACT_SILU, HC, OC, HIPETS_NORM_F64, OB, RW, TM, KMODE, HIPETS_PREC_F32, 1, RES>;

// does the model have the shape of the lean fp32 instance X(hc, oc, rw, tm, ob) of the tables above (the LDS row stride included)?
inline bool lean_shape_is(const ModelDev& md, const int hc, const int oc, const int rw, const int tm, const int ob) {
    return md.hidC == hc && md.outC == oc && md.reward_fn == rw && md.term_fn == tm && md.obs_process == ob && md.ld == lean_ld(hc, oc);
}
// ... of the bf16x3 or bf16 instance X(hc, oc, rw, tm)
inline bool b3_shape_is(const ModelDev& md, const int hc, const int oc, const int rw, const int tm) {
    return md.hidC == hc && md.outC == oc && md.reward_fn == rw && md.term_fn == tm && md.obs_process == HIPETS_OBS_NONE;
}
// ... of the hidden-static instance X(hc): the LDS row stride it was compiled for, i.e. no layer wider than the hidden ones
inline bool hid_static_is(const ModelDev& md, const int hc) { return md.hidC == hc && md.ld == lean_ld(hc, hc); }

// the lean fp32 instance of this model's shape for R row tiles: none, a plain one, or a KSpec::WIDE one
enum class LeanShape { none, plain, wide };
inline LeanShape lean_shape(const ModelDev& md, const int R) {
    if (md.precision != HIPETS_PREC_F32 || !spec_model(md)) return LeanShape::none;
#define HIPETS_HAS_SHAPE(HC, OC, RW, TM, OB) \
    if (lean_shape_is(md, HC, OC, RW, TM, OB)) return LeanSpec<HC, OC, RW, TM, OB, HIPETS_MODE_EXACT>::WIDE ? LeanShape::wide : LeanShape::plain;
    switch (R) {
        case 1: HIPETS_LEAN_SHAPES_R1(HIPETS_HAS_SHAPE) break;
        case 2: HIPETS_LEAN_SHAPES_R2(HIPETS_HAS_SHAPE) break;
        case 3: HIPETS_LEAN_SHAPES_R3(HIPETS_HAS_SHAPE) break;
        case 4: HIPETS_LEAN_SHAPES_R4(HIPETS_HAS_SHAPE) break;
        default: break;
    }
#undef HIPETS_HAS_SHAPE
    return LeanShape::none;
}

// is there a lean fp32 instance of this model's shape for R row tiles?  (the cost model prices a (shape, R) pair with an instance lower
// than one that runs the hidden-static or the generic kernel)
inline bool lean_shape_exists(const ModelDev& md, const int R) { return lean_shape(md, R) != LeanShape::none; }

// is the model one of the WIDE shapes?  (where the call is lean, rollout.hip rollout_geometry sizes the LDS and chooses R for that layout)
inline bool wide_model(const ModelDev& md) {
    for (int R = 1; R <= kMaxR; ++R)
        if (lean_shape(md, R) == LeanShape::wide) return true;
    return false;
}

// is there an instance of this model's shape for R row tiles in the model's own bf16x3 / bf16 arithmetic?  (fp32 models: no)
inline bool b3_shape_exists(const ModelDev& md, const int R) {
#define HIPETS_HAS_B3(HC, OC, RW, TM) \
    if (b3_shape_is(md, HC, OC, RW, TM)) return true;
    if (md.precision == HIPETS_PREC_BF16X3) {
        switch (R) {
            case 1: HIPETS_B3_SHAPES_R1(HIPETS_HAS_B3) break;
            case 2: HIPETS_B3_SHAPES_R2(HIPETS_HAS_B3) break;
            case 3: HIPETS_B3_SHAPES_R3(HIPETS_HAS_B3) break;
            case 4: HIPETS_B3_SHAPES_R4(HIPETS_HAS_B3) break;
            default: break;
        }
    } else if (md.precision == HIPETS_PREC_BF16) {
        switch (R) {
            case 1: HIPETS_BF16_SHAPES_R1(HIPETS_HAS_B3) break;
            case 2: HIPETS_BF16_SHAPES_R2(HIPETS_HAS_B3) break;
            case 3: HIPETS_BF16_SHAPES_R3(HIPETS_HAS_B3) break;
            case 4: HIPETS_BF16_SHAPES_R4(HIPETS_HAS_B3) break;
            default: break;
        }
    }
#undef HIPETS_HAS_B3
    return false;
}

// may this model / call run a hidden-static instance?  (SiLU, fp32 arithmetic, a hidden width of HIPETS_HID_STATIC_SHAPES;
// RolloutArgs::generic_only == 1 forbids it, 2 allows it)
inline bool hid_static_call(const ModelDev& md, const RolloutArgs& ra) {
    if (ra.generic_only == 1 || md.precision != HIPETS_PREC_F32 || md.activation != HIPETS_ACT_SILU) return false;
#define HIPETS_HAS_HID(HC) \
    if (hid_static_is(md, HC)) return true;
    HIPETS_HID_STATIC_SHAPES(HIPETS_HAS_HID)
#undef HIPETS_HAS_HID
    return false;
}

// The instance of rollout_kernel<R, ...> a call runs -- the one selection rule: the resolver of rollout_r<R>.hip dispatches on it,
// hipets_kernel_class reports it.  lean_wide: a KSpec::WIDE lean instance, which runs exactly where the host sized the LDS for its
// layout (RolloutArgs::wide_lds); generic_silu: the generic instance with the SiLU epilogue fixed.  Refusals: no_b3 / no_bf16 (bf16x3 and
// bf16 arithmetic exist in shape-specialised instances only: a model or call without one fails, it never runs another arithmetic),
// no_wide (LDS sized for a WIDE instance that does not exist for this R / call).
// lean_resident: the KSpec::RES twin of a plain lean instance (op heads resident in AccVGPRs), for the straight persistent form alone.
enum class RolloutInstance { lean, lean_resident, lean_wide, b3, bf16, hidden_static, generic_silu, generic, no_b3, no_bf16, no_wide };
// May a DEVICE rollout of `logical` workgroups of R row tiles ask for the resident-heads instance (RolloutArgs::resident_heads)?  Its
// premise: one wave per SIMD with the whole register file (R = 3: residency_rule.hpp), a model of kResLayers ops, and a persistent launch in which every
// launched workgroup serves exactly one logical workgroup for the whole horizon -- at most one per CU.  (A pure host rule; the caller
// still has to find that many workgroups co-resident: rollout.hip falls back to the plain instance where the capacity query says no.)
inline bool resident_heads_call(const ModelDev& md, const int R, const int logical, const int n_cu, const int horizon) {
    static_assert(kResLayers == kResHeadOps, "the host rule and the kernel count the same ops");
    return md.precision == HIPETS_PREC_F32 && resident_heads_wanted(R, md.n_layers, logical, n_cu, horizon);
}
inline RolloutInstance pick_rollout_instance(const ModelDev& md, const RolloutArgs& ra, const int R) {
    const bool lean = lean_call(md, ra);
    if (md.precision == HIPETS_PREC_BF16X3) return lean && b3_shape_exists(md, R) ? RolloutInstance::b3 : RolloutInstance::no_b3;
    if (md.precision == HIPETS_PREC_BF16) return lean && b3_shape_exists(md, R) ? RolloutInstance::bf16 : RolloutInstance::no_bf16;
    if (lean && lean_shape(md, R) == (ra.wide_lds ? LeanShape::wide : LeanShape::plain)) {
        if (ra.wide_lds) return RolloutInstance::lean_wide;
        return ra.resident_heads && !ra.whole_horizon && R == 3 && md.n_layers == kResLayers ? RolloutInstance::lean_resident : RolloutInstance::lean;
    }
    if (ra.wide_lds) return RolloutInstance::no_wide;
    if (hid_static_call(md, ra)) return RolloutInstance::hidden_static;
    return md.activation == HIPETS_ACT_SILU ? RolloutInstance::generic_silu : RolloutInstance::generic;
}

hipError_t launch_planet_rollout(int grid, unsigned lds, int lds_max, const PlanetDev& pd, const PlanetArgs& ra, hipStream_t st, bool static_shape);

}  // namespace hipets
