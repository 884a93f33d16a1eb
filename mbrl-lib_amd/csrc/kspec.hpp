// kspec.hpp -- the compile-time facts of a rollout-kernel instance (KSpec, lean_ld, kSplMaxTiles) and the per-layer dispatch they
// decide: which linear_op / linear_op_b3 instance runs layer l (mlp_layer, mlp_layer_b3, mlp_output_layer_fused).  Replaces the
// layer loop of GaussianMLP._default_forward (mbrl/models/gaussian_mlp.py:140-146: hidden_layers, then mean_and_logvar).
#pragma once
#include "gemm_bf16.hpp"
#include "gemm_f32.hpp"
#include "rollout_types.hpp"

namespace hipets {

// Compile-time facts of a rollout-kernel instance; -1 = decided at run time.  Instances with HIDC >= 0 are the
// SHAPE-SPECIALISED ("lean") kernels of the BASELINE configurations: hidden / output column-tile counts, normaliser kind,
// obs preprocessing, reward and termination functions and the launch mode are template arguments, and everything those
// shapes never use (expectation propagation, injected eps, traces, the phase profiler, batched / per-row initial states,
// per-member logvar bounds) is compiled out.  The host picks an instance only when the model and the call match ALL of its
// facts (launch.hpp pick_rollout_instance); anything else runs a generic one.  Same arithmetic, instruction for instruction, in
// the parts both execute: tests compare the two bit for bit.
// LDS row stride the host derives for a model whose widest layer has `tiles` column tiles (hipets_set_model: >= the widest
// activation, == 8 mod 64); a shape-specialised instance runs only when the model's stride is this one (launch.hpp lean_shape_is)
// Output layers of up to this many column tiles sum every unit's even / odd k-steps separately (wave_gemm SPL) and, in the
// shape-specialised fp32 instances, feed the fused tail (KSpec::FUSE).  Wider ones (cfg4': 47) keep the plain order: a wave's share
// is a dozen units there, and twice the accumulators (or a dozen inlined tails) do not fit the register file.
constexpr int kSplMaxTiles = 8;
constexpr int kResLayers = 5;  // ops of a model a KSpec::RES instance runs: input layer, three hidden-fed layers, output layer

constexpr int lean_ld(int hidc, int outc) {
    int m = (hidc > outc ? hidc : outc) * 16;
    while (m % 64 != 8) m += 4;
    return m;
}

template <int ACT_, int HIDC_ = -1, int OUTC_ = -1, int NORM_ = -1, int OBSP_ = -1, int REW_ = -1, int TERM_ = -1, int KMODE_ = -1, int PREC_ = 0,
          int FUSE_ = 0, int RES_ = 0>
struct KSpec {
    // WIDE (fused fp32 instances whose output layer is wider than kSplMaxTiles column tiles -- cfg4': 47): no LDS image of the outputs
    // exists at all, so the two activation buffers hold hidden activations only (row stride for HIDC tiles) and the model-input
    // image -- wider than a hidden layer there: 393 columns -- lives in buf0 with its own run-time stride (ModelDev::ld_in).
    // 4.4 KB of LDS per row instead of 7.6: two row tiles per workgroup fit where one did.
    static constexpr bool WIDE = FUSE_ != 0 && HIDC_ >= 0 && PREC_ == HIPETS_PREC_F32 && OUTC_ > kSplMaxTiles;
    static constexpr int LD = (HIDC_ >= 0 && PREC_ == HIPETS_PREC_F32) ? lean_ld(HIDC_, WIDE ? HIDC_ : OUTC_) : -1;  // compile-time LDS row stride (fp32 lean instances)
    static constexpr int ACT = ACT_, HIDC = HIDC_, OUTC = OUTC_, NORM = NORM_, OBSP = OBSP_, REW = REW_, TERM = TERM_, KMODE = KMODE_;
    static constexpr int PREC = PREC_;  // HIPETS_PREC_F32 (fp32 MFMA), or HIPETS_PREC_BF16X3 / HIPETS_PREC_BF16 (lean instances only)
    static constexpr int PIECES = PREC_ == HIPETS_PREC_BF16X3 ? 3 : (PREC_ == HIPETS_PREC_BF16 ? 1 : 0);  // bf16 pieces per operand on the bf16 matrix pipe
    static constexpr bool LEAN = HIDC_ >= 0 && OUTC_ >= 0;
    // HIDDEN-STATIC instances (HIDC_ >= 0, everything else decided at run time): what ANY model with that hidden width gets --
    // the reference's default is 200 = 13 column tiles (conf/dynamics_model/gaussian_mlp_ensemble.yaml:8), whatever its
    // environment's obs preprocessing, reward / termination functions, normaliser, output width or propagation method.  The ops
    // that carry > 90 % of a step's FLOPs (every op whose N is the hidden width) run exactly like in the shape-specialised
    // instances: per-wave (CT, EX) through one branch, compile-time LDS stride, interleaved fragment loads, unrolled k loops where
    // the register file allows; the output layer and every elementwise phase stay the generic kernel's.
    static constexpr bool HID_STATIC = HIDC_ >= 0 && OUTC_ < 0;
    // FUSE (lean fp32 instances): the output layer runs on the "head pair" pack and its accumulators go straight into the
    // step's tail -- sampling, delta, next state, hand-over publication, reward / termination / totals and the next step's
    // normalised model input happen in registers in the output layer's own barrier interval (5 barriers per step instead
    // of 7, no LDS round trip of the 2 x out_dim outputs).  Needs reward / termination forms that read state dims 0..3 only.
    // (output layers of up to 8 column tiles: beyond that -- cfg4' has 47 -- a wave's tail covers a dozen units and the instance spills)
    static constexpr bool FUSE = FUSE_ != 0 && LEAN && PREC_ == HIPETS_PREC_F32 && (OUTC_ <= kSplMaxTiles || WIDE);
    // RES (fused fp32 instances, not WIDE, R = 3: rollout_kernel asserts the R): the instance of the STRAIGHT PERSISTENT form only -- every
    // launched workgroup serves one logical workgroup, i.e. one member, for the whole launch -- with the op heads resident in AccVGPRs
    // (gemm_f32.hpp ResHead).  Models of kResLayers ops: the hidden-fed layers' heads are told apart by a switch over exactly three.
    static constexpr bool RES = RES_ != 0;
    static_assert(!RES || (FUSE && !WIDE), "resident op heads: fused fp32 instances");
    static constexpr bool SPL_OUT = OUTC_ >= 0 && OUTC_ <= kSplMaxTiles;  // the output layer sums even / odd k-steps separately (wave_gemm SPL)
    // K-split of the leftover hidden column tile (gemm_f32.hpp KsArgs): the fused fp32 instances whose hidden layers leave ONE column tile over
    // (13 = 3 x 4 + 1), used by the kernel for ONE-TILE workgroups only (R = 1: rollout_kernel's kKS)
    // (13 column tiles only: the consumer side, wave_gemm KSI inside KSO, rebuilds the last k chunk from slot kKsSlots - 1 of the last wave,
    // which is where a 13-chunk range -- 3 + 3 + 3 + 4 chunks -- ends; a 5- or 9-tile shape would end in another slot and read unwritten LDS)
    static constexpr bool KSPLIT = FUSE && !WIDE && kWaves == 4 && HIDC_ == 13;
    // termination functions that test EVERY state dim (inverted_pendulum: isfinite(next_obs).all(), termination_fns.py:47-55) are fused for
    // models with obs_dim <= 4 only -- then dims 0..3 ARE every dim (launch.hpp fused_term_ok checks the model)
    static_assert(!FUSE || ((REW_ == HIPETS_REW_HALFCHEETAH || REW_ == HIPETS_REW_CARTPOLE || REW_ == HIPETS_REW_CARTPOLE_PETS || REW_ == HIPETS_REW_LEARNED) &&
                            (TERM_ == HIPETS_TERM_NONE || TERM_ == HIPETS_TERM_CARTPOLE || TERM_ == HIPETS_TERM_HUMANOID || TERM_ == HIPETS_TERM_INVERTED_PENDULUM ||
                             TERM_ == HIPETS_TERM_HOPPER)),
                  "fused tail: the reward / termination lane sees dims 0..3 of its row");
    // hopper (termination_fns.py:12-26) tests EVERY state dim of a model whose dims span several column tiles, i.e. several waves: every
    // tail lane judges its own two dims and raises a per-row flag in LDS; the flag of step t is complete at the barrier that ends the
    // step and is folded into the row's `terminated` by the tail of step t + 1 -- which is when it first matters (model_env.py:186-188:
    // the reward of the terminating step itself still counts).  The row must still be HERE then: FAST instances only (in the persistent
    // DEVICE form it has moved to another workgroup, which would need the flag through the hand-over table); learned rewards only.
    // Round 5: DEVICE-mode instances too.  One launch per step: the flag of the launch's step is folded into `terminated` behind the
    // step loop, before the write-back.  Persistent form: the row has moved on -- and its NEXT owner holds every dim of the state it
    // receives: the threads that collect a pair of dims judge them exactly like the tail lanes would have and raise the flag in the
    // new owner's LDS (rollout_kernel hop_flags); nothing more travels through the hand-over table.
    static_assert(!FUSE || TERM_ != HIPETS_TERM_HOPPER || (REW_ == HIPETS_REW_LEARNED && !WIDE),
                  "fused tail with an all-dims termination function: instances with a learned reward");
    // learned rewards (round 4): the reward is the sampled LAST output column.  Without a termination function (pets_pusher / pets_reacher /
    // pets_mppi_halfcheetah) the lane that holds that column keeps the row's running total and needs no state dim at all; with one
    // (pets_inv_pendulum) the lane with dims 0, 1 keeps it and fetches the reward from the column's lane of the SAME accumulator, i.e. the
    // column must sit in column tile 0: obs_dim < 8 (fused_term_ok)
    static_assert(!FUSE || REW_ != HIPETS_REW_LEARNED || !WIDE, "fused tail with learned rewards: no WIDE instance");
    // obs preprocessing in the fused tail (round 4): the lane that holds the trig dim writes its sin and cos columns (ObsMap)
    static_assert(!FUSE || (NORM_ == HIPETS_NORM_F64 && (OBSP_ == HIPETS_OBS_NONE || !WIDE)), "fused tail: f64 normaliser; WIDE instances: no obs preprocessing");
    static_assert(!FUSE || OBSP_ == HIPETS_OBS_NONE || OBSP_ == HIPETS_OBS_HALFCHEETAH || OBSP_ == HIPETS_OBS_CARTPOLE_PETS, "unknown obs preprocessing");
};

// Layer l in bf16x3 / bf16 arithmetic
template <int R, class S>
__device__ __forceinline__ void mlp_layer_b3(const ModelDev& md, const LayerMeta* lmeta, const int l, const int member, const float* in, float* out,
                                             const int wave, const int lane) {
    const LayerMeta lm = lmeta[l];
    const uint4* W3 = md.w3 + (size_t)member * md.w3member + lm.woff3;
    const float* bias = md.b + (size_t)member * md.bmember + lm.boff;
    const char* inb = reinterpret_cast<const char*>(in);
    char* outb = reinterpret_cast<char*>(out);
    if (l < md.n_layers - 1) linear_op_b3<R, S::ACT, S::HIDC, S::PIECES>(W3, bias, lm.Kp32 / 32, md.ld * 4, false, inb, outb, wave, lane);
    else linear_op_b3<R, S::ACT, S::OUTC, S::PIECES>(W3, bias, lm.Kp32 / 32, md.ld * 4, true, inb, outb, wave, lane);
}

// Layer l of the ensemble MLP with member `member`'s weights.
// part: the two k-split partial-sum buffers of a KSpec::KSPLIT one-tile workgroup ([2][kWaves][64][4] floats, alternating by layer)
template <int R, class S>
__device__ __forceinline__ void mlp_layer(const ModelDev& md, const LayerMeta* lmeta, const int l, const int member,
                                          const float* in, float* out, const int wave, const int lane, Prof& prof, float* part = nullptr,
                                          const ResHead* heads = nullptr) {
    const LayerMeta lm = lmeta[l];  // staged in LDS once per launch (a global scalar load here cost ~400 cycles per layer)
    const float* W = md.w + (size_t)member * md.wmember + lm.woff;
    const float* bias = md.b + (size_t)member * md.bmember + lm.boff;
    if constexpr (S::KSPLIT && R == 1) {
        // hidden ops of a one-tile workgroup: every wave 3 column tiles + its quarter of the 13th tile's k range (wave_gemm KSO); ops fed
        // by a hidden layer rebuild their last k chunk from the previous op's partial sums (KSI)
        float* const po = part + (l & 1) * (kWaves * 64 * 4);
        const float* const pi = part + ((l & 1) ^ 1) * (kWaves * 64 * 4);
        if (l == 0) linear_op<R, S::ACT, S::HIDC, NoTail, S::LD, false, -1, 2>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof, nullptr, 0, nullptr, po);
        else linear_op<R, S::ACT, S::HIDC, NoTail, S::LD, false, S::HIDC, 3>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof, nullptr, 0, pi, po);
    } else if constexpr (S::LEAN) {
        // ops fed by a hidden layer have K = hid: HIDC chunks, a compile-time count (the input layer's K is the model's input width)
        // Unrolled only where the register file is not the constraint (R >= 3: one workgroup per CU, 512 registers per lane).  At R = 2
        // (two workgroups per CU, 256-register cap) the allocator splits accumulator live ranges inside the unrolled stream and
        // puts v_mov copies straight behind asm MFMAs -- which it believes complete at once (wave_gemm, "drain_all") -- and the
        // interleaved + unrolled build returned wrong sums (caught by the cfg5 parity tests); R = 1 measured 1 % slower unrolled.
        constexpr int kHidChunks = MinWavesOf<R>::value == 1 ? S::HIDC : -1;
        if constexpr (S::RES) {  // (never an output layer here: the fused instances run it through mlp_output_layer_fused)
            if (l == 0) linear_op<R, S::ACT, S::HIDC, NoTail, S::LD, false, -1, 0, 1>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof, nullptr, 0, nullptr, nullptr, heads);
            else linear_op<R, S::ACT, S::HIDC, NoTail, S::LD, false, kHidChunks, 0, 3>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof, nullptr, 0, nullptr, nullptr, heads + 1, l - 1);
        } else
        if (l == 0) linear_op<R, S::ACT, S::HIDC, NoTail, S::LD>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof, nullptr, S::WIDE ? md.ld_in : 0);
        else if (l < md.n_layers - 1) linear_op<R, S::ACT, S::HIDC, NoTail, S::LD, false, kHidChunks>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof);
        else linear_op<R, S::ACT, S::OUTC, NoTail, S::LD, (S::OUTC <= kSplMaxTiles), kHidChunks>(W, bias, lm, md.ld, false, md.activation, md.slope, in, out, wave, lane, prof);
    } else if constexpr (S::HID_STATIC) {
        // (unrolled up to 13 MFMA units per wave -- the widest the shape-specialised instances run: at 16 units, hid 256 with R = 4,
        // the allocator splits accumulator live ranges inside the unrolled stream again and the build's ISA scan finds a v_mov of an
        // accumulator behind an MFMA still in flight; the rolled loop ends every block with drain_all)
        constexpr int kHidChunks = (MinWavesOf<R>::value == 1 && ((S::HIDC + kWaves - 1) / kWaves) * R <= 13) ? S::HIDC : -1;
        if (l == 0) linear_op<R, S::ACT, S::HIDC, NoTail, S::LD>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof);
        else if (l < md.n_layers - 1) linear_op<R, S::ACT, S::HIDC, NoTail, S::LD, false, kHidChunks>(W, bias, lm, md.ld, true, md.activation, md.slope, in, out, wave, lane, prof);
        else if (lm.Np / kTile <= kSplMaxTiles)  // the output layer: the generic instance's dispatch, the SAME summation rule (SPL)
            linear_op<R, S::ACT, -1, NoTail, -1, true>(W, bias, lm, md.ld, false, md.activation, md.slope, in, out, wave, lane, prof);
        else linear_op<R, S::ACT>(W, bias, lm, md.ld, false, md.activation, md.slope, in, out, wave, lane, prof);
    } else {
        // the output layer of up to kSplMaxTiles column tiles: SPL (the SAME rule in the shape-specialised branch above)
        if (l == md.n_layers - 1 && lm.Np / kTile <= kSplMaxTiles)
            linear_op<R, S::ACT, -1, NoTail, -1, true>(W, bias, lm, md.ld, false, md.activation, md.slope, in, out, wave, lane, prof);
        else linear_op<R, S::ACT>(W, bias, lm, md.ld, l < md.n_layers - 1, md.activation, md.slope, in, out, wave, lane, prof);
    }
}

// The OUTPUT layer of a KSpec::FUSE instance: the "head pair" pack, accumulators handed to `tl` (no LDS image of the outputs)
template <int R, class S, class TL>
__device__ __forceinline__ void mlp_output_layer_fused(const ModelDev& md, const LayerMeta* lmeta, const int member, const float* in,
                                                       const int wave, const int lane, Prof& prof, const TL& tl, const float* part = nullptr,
                                                       const ResHead* heads = nullptr) {
    const LayerMeta lm = lmeta[md.n_layers - 1];
    const float* W = md.w + (size_t)member * md.wmember + lm.woff_pairs;
    const float* bias = md.b + (size_t)member * md.bmember + lm.boff_pairs;
    if constexpr (S::KSPLIT && R == 1) {  // the last hidden layer (index n_layers - 2) left its 13th tile as partial sums
        const float* const pi = part + ((md.n_layers - 2) & 1) * (kWaves * 64 * 4);
        linear_op<R, S::ACT, S::OUTC, TL, S::LD, S::SPL_OUT, S::HIDC, 1>(W, bias, lm, md.ld, false, md.activation, md.slope, in, nullptr, wave, lane, prof, &tl, 0, pi);
    } else if constexpr (S::RES) {
        linear_op<R, S::ACT, S::OUTC, TL, S::LD, S::SPL_OUT, S::HIDC, 0, 1>(W, bias, lm, md.ld, false, md.activation, md.slope, in, nullptr, wave, lane, prof, &tl, 0, nullptr, nullptr, heads + kResLayers - 1);
    } else {
        linear_op<R, S::ACT, S::OUTC, TL, S::LD, S::SPL_OUT, MinWavesOf<R>::value == 1 ? S::HIDC : -1>(W, bias, lm, md.ld, false, md.activation, md.slope, in, nullptr, wave, lane, prof, &tl);
    }
}

// a RES instance's heads, one per op; nothing in every other instance
template <bool RES> struct ResHeadStore {
    ResHead h[kResLayers];
    __device__ __forceinline__ ResHead* get() { return h; }
};
template <> struct ResHeadStore<false> {
    __device__ __forceinline__ ResHead* get() { return nullptr; }
};

// The heads of all kResLayers ops of member `member` for this wave, requested into AccVGPRs (the caller waits once and pins them)
template <int R, class S>
__device__ __forceinline__ void res_load_heads(ResHead* const heads, const ModelDev& md, const LayerMeta* lmeta, const int member, const int wave, const int lane) {
    const float* const Wm = md.w + (size_t)member * md.wmember;
    const float* const bm = md.b + (size_t)member * md.bmember;
#pragma unroll
    for (int l = 0; l < kResLayers - 1; ++l) res_load_op<R, S::HIDC>(heads[l], Wm + lmeta[l].woff, bm + lmeta[l].boff, lmeta[l].Kp / kKChunk, wave, lane);
    const LayerMeta lo = lmeta[kResLayers - 1];
    res_load_op<R, S::OUTC>(heads[kResLayers - 1], Wm + lo.woff_pairs, bm + lo.boff_pairs, lo.Kp / kKChunk, wave, lane);
}
template <int R, class S>
__device__ __forceinline__ void res_pin_heads(ResHead* const heads) {
#pragma unroll
    for (int l = 0; l < kResLayers - 1; ++l) res_pin_op<R, S::HIDC>(heads[l]);
    res_pin_op<R, S::OUTC>(heads[kResLayers - 1]);
}

}  // namespace hipets
