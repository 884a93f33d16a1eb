// rollout_inst.inc -- body of rollout_r<R>.hip: instantiates rollout_kernel<HIPETS_R, KSpec<...>> -- the generic instances
// (activation fixed to SiLU, or read at run time) and the shape-specialised "lean" instances of the BASELINE configurations --
// and defines rollout_instance_r<R> (launch.hpp), which RESOLVES the instance launch.hpp pick_rollout_instance names to its KernelRec (host
// address + LDS opt-in flags).  Nothing here launches: the one launcher, the occupancy estimate, the co-residency self-test and the table
// of validated grids live in residency.hpp (host only, compiled with rollout.hip).
// HIPETS_PART splits an R over four translation units, so that no compile job of the build is longer than its largest single kernel
// instance (round 6: the two fully generic instances take 40-60 s each, an R's whole set took 85-140 s as one unit):
//   1  rollout_r<R>.hip       the resolver, the reference-semantics (EXACT / DEVICE) shape-specialised instances, the hidden-static one
//   2  rollout_r<R>_fast.hip  the FAST-mode shape-specialised instances               behind HIPETS_FN(_fast)
//   3  rollout_r<R>_gen.hip   the fully generic instance (activation read at run time) behind HIPETS_FN(_gen)
//   4  rollout_r<R>_gens.hip  the fully generic instance with the SiLU epilogue fixed  behind HIPETS_FN(_gens)
#ifndef HIPETS_PART
#error "define HIPETS_PART (1..4) and HIPETS_R before including rollout_inst.inc"
#endif
#define HIPETS_CAT2_(a, b) a##b
#define HIPETS_CAT2(a, b) HIPETS_CAT2_(a, b)
#define HIPETS_FN(suffix) HIPETS_CAT2(HIPETS_CAT2(rollout_instance_r, HIPETS_R), suffix)
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "rollout.hpp"

// lean fp32, bf16x3 and bf16 shapes instantiated for this R: the per-R tables of launch.hpp
#define HIPETS_LEAN_SHAPES(X) HIPETS_CAT2(HIPETS_LEAN_SHAPES_R, HIPETS_R)(X)
#define HIPETS_B3_SHAPES(X) HIPETS_CAT2(HIPETS_B3_SHAPES_R, HIPETS_R)(X)
#define HIPETS_BF16_SHAPES(X) HIPETS_CAT2(HIPETS_BF16_SHAPES_R, HIPETS_R)(X)

// The launch mode of this unit's shape-specialised instances and the function that resolves them (HIPETS_SPEC_FN), and the record of
// the instance of a table row that matches the model: the lean fp32 instances run the output layer's accumulators straight into the
// step's tail (KSpec::FUSE = 1).
#if HIPETS_PART == 2
#define HIPETS_LEAN_MODE HIPETS_MODE_FAST
#define HIPETS_SPEC_FN HIPETS_FN(_fast)
#else
#define HIPETS_LEAN_MODE HIPETS_MODE_EXACT
#define HIPETS_SPEC_FN HIPETS_FN(_exact)
#endif
#define HIPETS_TRY_SHAPE(HC, OC, RW, TM, OB) \
    if (lean_shape_is(md, HC, OC, RW, TM, OB)) return &rec<LeanSpec<HC, OC, RW, TM, OB, HIPETS_LEAN_MODE>>();
#define HIPETS_TRY_RES_SHAPE(HC, OC, RW, TM, OB) \
    if (lean_shape_is(md, HC, OC, RW, TM, OB)) return &rec<LeanSpec<HC, OC, RW, TM, OB, HIPETS_LEAN_MODE, 1>>();
#define HIPETS_TRY_PREC(PREC, HC, OC, RW, TM) \
    if (b3_shape_is(md, HC, OC, RW, TM)) return &rec<KSpec<HIPETS_ACT_SILU, HC, OC, HIPETS_NORM_F64, HIPETS_OBS_NONE, RW, TM, HIPETS_LEAN_MODE, PREC>>();
#define HIPETS_TRY_B3(HC, OC, RW, TM) HIPETS_TRY_PREC(HIPETS_PREC_BF16X3, HC, OC, RW, TM)
#define HIPETS_TRY_BF16(HC, OC, RW, TM) HIPETS_TRY_PREC(HIPETS_PREC_BF16, HC, OC, RW, TM)
#define HIPETS_TRY_HID(HC) \
    if (hid_static_is(md, HC)) return &rec<KSpec<HIPETS_ACT_SILU, HC>>();

namespace hipets {

namespace {
// the record of ONE instance: its host address and per-device LDS opt-in flags (launch.hpp KernelRec; residency.hpp works on it)
template <class S>
KernelRec& rec() {
    static KernelRec r{reinterpret_cast<const void*>(&rollout_kernel<HIPETS_R, S>)};
    return r;
}
}  // namespace

// the other translation units of this R
KernelRec* HIPETS_FN(_fast)(RolloutInstance pick, const ModelDev& md);
KernelRec* HIPETS_FN(_gen)();
KernelRec* HIPETS_FN(_gens)();

#if HIPETS_PART == 3
KernelRec* HIPETS_FN(_gen)() { return &rec<KSpec<-1>>(); }
#endif
#if HIPETS_PART == 4
KernelRec* HIPETS_FN(_gens)() { return &rec<KSpec<HIPETS_ACT_SILU>>(); }  // the PETS default
#endif

#if HIPETS_PART <= 2
// the shape-specialised instance that the pick names, in this unit's launch mode: a bf16x3 one, a bf16 one, or a lean fp32 one (KSpec::WIDE or not)
KernelRec* HIPETS_SPEC_FN(const RolloutInstance pick, const ModelDev& md) {
    if (pick == RolloutInstance::b3) {
        HIPETS_B3_SHAPES(HIPETS_TRY_B3)
    } else if (pick == RolloutInstance::bf16) {
        HIPETS_BF16_SHAPES(HIPETS_TRY_BF16)
#if HIPETS_PART == 1 && HIPETS_R == 3
    } else if (pick == RolloutInstance::lean_resident) {  // (step-synchronous unit, one wave per SIMD: the only place these instances exist)
        HIPETS_LEAN_SHAPES(HIPETS_TRY_RES_SHAPE)
#endif
    } else {
        HIPETS_LEAN_SHAPES(HIPETS_TRY_SHAPE)
    }
    return nullptr;  // (not reached: the pick found the model's row in this table)
}
#endif

#if HIPETS_PART == 1
KernelRec* HIPETS_FN()(const ModelDev& md, const RolloutArgs& ra, hipError_t* why) {
    const RolloutInstance pick = pick_rollout_instance(md, ra, HIPETS_R);
    *why = hipErrorNotSupported;
    switch (pick) {
        case RolloutInstance::lean:
        case RolloutInstance::lean_resident:
        case RolloutInstance::lean_wide:
        case RolloutInstance::b3:
        case RolloutInstance::bf16: return (ra.whole_horizon ? HIPETS_FN(_fast) : HIPETS_FN(_exact))(pick, md);
        case RolloutInstance::hidden_static: HIPETS_HID_STATIC_SHAPES(HIPETS_TRY_HID) break;
        case RolloutInstance::generic_silu: return HIPETS_FN(_gens)();
        case RolloutInstance::generic: return HIPETS_FN(_gen)();
        case RolloutInstance::no_b3:
        case RolloutInstance::no_bf16: break;                                        // (rollout.hip launch_rollout reports it)
        case RolloutInstance::no_wide: *why = hipErrorInvalidConfiguration; break;  // never run another layout in LDS sized for a WIDE instance
    }
    return nullptr;
}
#endif  // HIPETS_PART == 1

}  // namespace hipets
