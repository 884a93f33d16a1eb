// gemm_f32.hpp -- the fp32 MFMA GEMM of a workgroup's row tiles: the MFMA / LDS primitives, the phase profiler (Prof), the bound
// checks of the debug build (HIPETS_BOUND), the fused-tail hooks (NoTail / FusedSlot / TailStages), one wave's share of a linear op
// (wave_gemm, wave_gemm_ex) and the op itself (linear_op).  Replaces EnsembleLinearLayer.forward (mbrl/models/util.py:53-65:
// xw = x.matmul(weight) + bias per member) and the activation behind it (gaussian_mlp.py:89-112); the PlaNet kernel runs its
// nn.Linear ops (mbrl/models/planet.py:83-101, :229-234, :260-266) through the same code.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "rollout_types.hpp"

namespace hipets {

// D = A(16x4) * B(4x16) + C, exact f32.  Issued through inline asm with the accumulator tied in place
// ("+v"): with the builtin, hipcc's register allocator rotates the accumulators through fresh registers in
// the unrolled k loop and pays ~45 v_accvgpr_mov/read/write per iteration to undo it at the back edge.
// Hazards: A/B come from loads (the compiler's s_waitcnt covers asm inputs); back-to-back MFMAs that take
// the previous D whole as C need no wait states; the first non-MFMA reader of D is fenced by mfma_drain().
__device__ __forceinline__ void mfma16x16x4(const float a, const float b, f32x4& c) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// ... with the weight operand read from an AccVGPR (gfx950 MFMAs take A / B from either file): the resident op heads below
__device__ __forceinline__ void mfma16x16x4_ra(const float a, const float b, f32x4& c) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(c) : "a"(a), "v"(b));
}
// >= 12 wait states between the last 8-pass MFMA and a VALU read of its result (cdna4 ISA, XDL write -> VALU read)
__device__ __forceinline__ void mfma_drain() { asm volatile("s_nop 15" ::: "memory"); }

// Column c of an activation row lives at LDS position lds_col(c): inside every 16-wide k chunk the 4x4 block
// (k-step s, lane group g) is stored transposed, so the lane group g of the A fragment reads its 4 k-steps
// {16kk + 4s + g : s = 0..3} with ONE ds_read_b128 at [16kk + 4g, +3].
__device__ __forceinline__ int lds_col(int c) { return (c & ~15) | ((c & 3) << 2) | ((c >> 2) & 3); }

// phase profiler: lane 0 of every wave of workgroup 0 accumulates s_memtime deltas per phase in LDS (a mark is one LDS
// read-modify-write on one lane, ~100 cycles; accumulating straight into global memory cost a ~800-cycle round trip per
// mark and dominated the short phases it measured) and flushes them into RolloutArgs::phase_cycles[wave][phase] at the end
// of the launch (a profiling aid, off unless the caller passes a buffer).  An accumulator holds the cycles in its low 44 bits and
// the NUMBER of marks that fed it above them (round 6): a reader divides both by the step count and can subtract what the marks
// themselves cost (profiles/one_tile_phase_profile.py calibrates that against the unprofiled launch duration).
constexpr int kProfCountShift = 44;
struct Prof {
    long long* slot;  // LDS: this wave's 16 accumulators
    long long t;
    bool on;
    __device__ __forceinline__ void mark(int phase) {
        if (on) {
            const long long now = clock64();
            slot[phase] += (now - t) + (1ll << kProfCountShift);
            t = now;
        }
    }
};

#ifndef HIPETS_LEAN_PROF
#define HIPETS_LEAN_PROF 0  // profiling builds: the phase profiler also in the shape-specialised instances (profiles/kernel_variants.py)
#endif

// One wave's share of a layer: CT strided column tiles (c_first + kWaves*ct) for all R row tiles, plus EX
// "extra" (column tile, row tile) units taken from the C % 4 leftover column tiles, all accumulated
// in the same k loop so the MFMA pipe always has >= 2 independent accumulators in flight.
// The k loop is software pipelined by hand with two register buffers: the B fragments (global, L2
// resident) and A fragments (LDS) of chunk kk+1 are in flight while the 4*(CT*R+EX) MFMAs of chunk kk
// issue (one wave per SIMD, so nothing else hides the load latency).
template <int R, int CT, int EX>
struct GemmFrags {
    f32x4 b[CT > 0 ? CT : 1];
    f32x4 bx[EX > 0 ? EX : 1];
    f32x4 a[R];
    f32x4 ax[EX > 0 ? EX : 1];
};

using u32x4g = __attribute__((ext_vector_type(4))) unsigned;  // 16 bytes as four words: a raw buffer load, a pair of hand-over granules

// Minimum waves per SIMD the register allocation must leave room for (= workgroups of 4 waves per CU).  R <= 2 keeps two
// workgroups per CU resident (their barrier / latency phases overlap); R = 3, 4 need the registers.
template <int R> struct MinWavesOf { static constexpr int value = R <= 2 ? 2 : 1; };

// Debug build (__graft_entry__.build_debug: -O1 -g -DHIPETS_DEBUG_BOUNDS=1, host side under AddressSanitizer): every LDS section of
// the rollout kernel is checked against the dynamic LDS size of the launch, and the indexed LDS accesses of the elementwise phases
// against their section.  A violated bound aborts the kernel (device assert -> the next HIP call reports it).  Off in the shipped
// library: the checks cost registers in kernels that sit at the limit.
#ifndef HIPETS_DEBUG_BOUNDS
#define HIPETS_DEBUG_BOUNDS 0
#endif
#if HIPETS_DEBUG_BOUNDS
// (not <cassert>'s assert: the generic lambdas of wave_gemm are implicitly __host__ __device__, where the host's __assert_fail is not callable)
__host__ __device__ inline void hipets_bound_fail(const int line) {
#if defined(__HIP_DEVICE_COMPILE__)
    // (the line is one of gemm_f32.hpp -- wave_gemm's checks -- or of rollout.hpp: a HIPETS_BOUND sits on it in one of the two)
    printf("hipets: bound violated at gemm_f32.hpp / rollout.hpp line %d (workgroup %d, thread %d)\n", line, (int)blockIdx.x, (int)threadIdx.x);
    __builtin_trap();
#else
    (void)line;
#endif
}
#define HIPETS_BOUND(cond) do { if (!(cond)) hipets_bound_fail(__LINE__); } while (0)
#else
#define HIPETS_BOUND(cond) ((void)0)
#endif

// RESIDENT OP HEADS (KSpec::RES; the straight persistent form of the fused fp32 instances with one wave per SIMD, R = 3).  There a
// workgroup is bound to ONE member for the whole launch, so what a wave needs before the first MFMA of an op -- its biases and the
// chunk-0 weight fragments of its column tiles -- are the same bits at every step.  They are loaded ONCE per launch, straight into
// AccVGPRs (these instances leave ~200 of the 256 idle), and every step's op starts from them: accumulators from the resident
// bias, the chunk-0 MFMAs with their weight operand in the AccVGPR file; the only loads in front of the first MFMA are the
// activation fragments from LDS.  From chunk 1 on the k loop is the ordinary one (same operands, same order: same bits).
// One head = at most kMaxCT = 3 strided column tiles + 3 extra units of a wave: 6 fragments + 6 bias quads, of which a wave's
// (CT, EX) uses CT + EX each; the others are never loaded or read (no register).
struct ResHead {
    f32x4 b[3], bx[3], bv[3], bvx[3];
};
__device__ __forceinline__ void res_load(f32x4& dst, const float* const p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(dst) : "v"(p) : "memory"); }
__device__ __forceinline__ void res_pin(f32x4& v) { asm volatile("" : "+a"(v)); }

// CONDITIONAL K-STEPS (shape-specialised ops with one wave per SIMD, R >= 3: wave_gemm's kStraight).  Whether a k-step of an op runs is
// a wave-uniform RUN-TIME fact in two places -- the last chunk holds 1..4 real k-steps, the input layer has 1.. chunks -- and written as
// C++ control flow around the asm MFMAs it costs what the k loop otherwise avoids: where the arms begin and meet, the register
// allocator copies EVERY accumulator of the wave (clumps of ~20 v_mov_b64 between two MFMAs), and every arm must end in a pipe drain
// so that those copies read finished results.  Here the choice stays out of the compiler's sight: one k-step of up to NC column tiles x
// R row tiles + NE extra units is ONE asm statement that jumps over its own MFMAs when n <= S (n in an SGPR, S the k-step's number).
// The compiler sees straight-line code with the accumulators tied in place: no phis, no copies, no drains per arm.  The k-step's s_nop 1
// guard (hazard (1) of wave_gemm) sits inside the statement, behind the branch.  An asm statement takes at most 30 operands, an
// accumulator ("+v") counts twice: the wave's share goes through in as few statements as that allows (kstep_if in wave_gemm).
// WC: the register file of the weight operands, "v" or "a" (resident heads).
#define HIPETS_KT_MF(C, B, A) "v_mfma_f32_16x16x4_f32 %[" #C "], %[" #B "], %[" #A "], %[" #C "]\n\t"
#define HIPETS_KT_COL3(ct) HIPETS_KT_MF(c##ct##0, b##ct, a0) HIPETS_KT_MF(c##ct##1, b##ct, a1) HIPETS_KT_MF(c##ct##2, b##ct, a2)
#define HIPETS_KT_COL4(ct) HIPETS_KT_COL3(ct) HIPETS_KT_MF(c##ct##3, b##ct, a3)
#define HIPETS_KT_EX(e) HIPETS_KT_MF(x##e, bx##e, ax##e)
#define HIPETS_KT_ACC3(ct) [c##ct##0] "+v"(*c[ct][0]), [c##ct##1] "+v"(*c[ct][1]), [c##ct##2] "+v"(*c[ct][2])
#define HIPETS_KT_ACC4(ct) HIPETS_KT_ACC3(ct), [c##ct##3] "+v"(*c[ct][3])
#define HIPETS_KT_XACC(e) [x##e] "+v"(*x[e])
#define HIPETS_KT_A3 [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2])
#define HIPETS_KT_A4 HIPETS_KT_A3, [a3] "v"(a[3])
#define HIPETS_KT_B(WC, ct) [b##ct] WC(b[ct])
#define HIPETS_KT_XIN(WC, e) [bx##e] WC(bx[e]), [ax##e] "v"(ax[e])
#define HIPETS_KT_ASM(BODY, OUTS, INS)                                                                                        \
    asm volatile("s_cmp_le_i32 %[n], %[s]\n\ts_cbranch_scc1 .Lhipets_kt%=\n\ts_nop 1\n\t" BODY ".Lhipets_kt%=:" \
                 : OUTS : INS, [n] "s"(n), [s] "n"(S) : "scc")
#define HIPETS_KT_COMMA ,
#define HIPETS_KT_SHAPES(WC)                                                                                                                        \
    if constexpr (R == 3 && NC == 3 && NE == 1)                                                                                                     \
        HIPETS_KT_ASM(HIPETS_KT_COL3(0) HIPETS_KT_COL3(1) HIPETS_KT_COL3(2) HIPETS_KT_EX(0),                                                        \
                      HIPETS_KT_ACC3(0) HIPETS_KT_COMMA HIPETS_KT_ACC3(1) HIPETS_KT_COMMA HIPETS_KT_ACC3(2) HIPETS_KT_COMMA HIPETS_KT_XACC(0),      \
                      HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_B(WC, 1) HIPETS_KT_COMMA HIPETS_KT_B(WC, 2) HIPETS_KT_COMMA HIPETS_KT_A3         \
                          HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 0));                                                                                    \
    else if constexpr (R == 3 && NC == 3 && NE == 0)                                                                                                \
        HIPETS_KT_ASM(HIPETS_KT_COL3(0) HIPETS_KT_COL3(1) HIPETS_KT_COL3(2),                                                                        \
                      HIPETS_KT_ACC3(0) HIPETS_KT_COMMA HIPETS_KT_ACC3(1) HIPETS_KT_COMMA HIPETS_KT_ACC3(2),                                        \
                      HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_B(WC, 1) HIPETS_KT_COMMA HIPETS_KT_B(WC, 2) HIPETS_KT_COMMA HIPETS_KT_A3);       \
    else if constexpr (R == 3 && NC == 1 && NE == 1)                                                                                                \
        HIPETS_KT_ASM(HIPETS_KT_COL3(0) HIPETS_KT_EX(0), HIPETS_KT_ACC3(0) HIPETS_KT_COMMA HIPETS_KT_XACC(0),                                       \
                      HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_A3 HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 0));                                        \
    else if constexpr (R == 3 && NC == 1 && NE == 2)                                                                                                \
        HIPETS_KT_ASM(HIPETS_KT_COL3(0) HIPETS_KT_EX(0) HIPETS_KT_EX(1), HIPETS_KT_ACC3(0) HIPETS_KT_COMMA HIPETS_KT_XACC(0) HIPETS_KT_COMMA HIPETS_KT_XACC(1), \
                      HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_A3 HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 0) HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 1));   \
    else if constexpr (R == 4 && NC == 2 && NE == 0)                                                                                                \
        HIPETS_KT_ASM(HIPETS_KT_COL4(0) HIPETS_KT_COL4(1), HIPETS_KT_ACC4(0) HIPETS_KT_COMMA HIPETS_KT_ACC4(1),                                     \
                      HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_B(WC, 1) HIPETS_KT_COMMA HIPETS_KT_A4);                                          \
    else if constexpr (R == 4 && NC == 1 && NE == 0)                                                                                                \
        HIPETS_KT_ASM(HIPETS_KT_COL4(0), HIPETS_KT_ACC4(0), HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_A4);                                       \
    else if constexpr (R == 4 && NC == 1 && NE == 1)                                                                                                \
        HIPETS_KT_ASM(HIPETS_KT_COL4(0) HIPETS_KT_EX(0), HIPETS_KT_ACC4(0) HIPETS_KT_COMMA HIPETS_KT_XACC(0),                                       \
                      HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_A4 HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 0));                                        \
    else if constexpr (R == 4 && NC == 1 && NE == 2)                                                                                                \
        HIPETS_KT_ASM(HIPETS_KT_COL4(0) HIPETS_KT_EX(0) HIPETS_KT_EX(1), HIPETS_KT_ACC4(0) HIPETS_KT_COMMA HIPETS_KT_XACC(0) HIPETS_KT_COMMA HIPETS_KT_XACC(1), \
                      HIPETS_KT_B(WC, 0) HIPETS_KT_COMMA HIPETS_KT_A4 HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 0) HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 1));   \
    else if constexpr (NC == 0 && NE == 1)                                                                                                          \
        HIPETS_KT_ASM(HIPETS_KT_EX(0), HIPETS_KT_XACC(0), HIPETS_KT_XIN(WC, 0));                                                                    \
    else if constexpr (NC == 0 && NE == 2)                                                                                                          \
        HIPETS_KT_ASM(HIPETS_KT_EX(0) HIPETS_KT_EX(1), HIPETS_KT_XACC(0) HIPETS_KT_COMMA HIPETS_KT_XACC(1),                                         \
                      HIPETS_KT_XIN(WC, 0) HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 1));                                                                   \
    else if constexpr (NC == 0 && NE == 3)                                                                                                          \
        HIPETS_KT_ASM(HIPETS_KT_EX(0) HIPETS_KT_EX(1) HIPETS_KT_EX(2), HIPETS_KT_XACC(0) HIPETS_KT_COMMA HIPETS_KT_XACC(1) HIPETS_KT_COMMA HIPETS_KT_XACC(2), \
                      HIPETS_KT_XIN(WC, 0) HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 1) HIPETS_KT_COMMA HIPETS_KT_XIN(WC, 2));                              \
    else                                                                                                                                            \
        static_assert(R < 0, "conditional k-step: a (row tiles, column tiles, extras) share the shape tables do not produce")
// c[ct][r] / x[e]: the accumulators of the k-step's parity; b / bx, a / ax: element S of the weight and activation fragments
template <int R, int NC, int NE, int S, bool WA>
__device__ __forceinline__ void mfma_kstep_if(const int n, f32x4* const (&c)[NC > 0 ? NC : 1][R], f32x4* const (&x)[NE > 0 ? NE : 1],
                                              const float (&b)[NC > 0 ? NC : 1], const float (&a)[R], const float (&bx)[NE > 0 ? NE : 1],
                                              const float (&ax)[NE > 0 ? NE : 1]) {
    if constexpr (WA) {
        HIPETS_KT_SHAPES("a");
    } else {
        HIPETS_KT_SHAPES("v");
    }
}

struct NoTail {};  // wave_gemm's TL: the ordinary epilogue (activation, store as the next op's LDS image)
// A fused tail = four stages over the accumulators (units) a wave finished: prep(slot, c, r) for EVERY unit of a group first -- it
// only loads (LDS) what the unit will need into its slot, so the round trips of all units overlap --, then draw(slot a, slot b, c_a,
// c_b, two) for every PAIR of units (the pair's standard normals: one Philox block per lane for the two units together, see
// rollout_kernel's tail_draw), then unit(slot, acc, c, r) for every unit (arithmetic + stores), then finish() once per wave.
struct FusedSlot {  // what one unit's lane reads from LDS (rollout_kernel, KSpec::FUSE)
    float mxA, mxB, mnA, mnB, pA, pB;
    double nmA, nmB, nsA, nsB;
    int rid, ndA, ndB;
    float n0, n1;  // the two standard normals of the lane's dims (draw stage)
};
template <class P, class D, class F, class G>
struct TailStages {
    P prep;
    D draw;
    F unit;
    G finish;
};
template <class P, class D, class F, class G>
__device__ __forceinline__ TailStages<P, D, F, G> make_tail(P p, D d, F f, G g) { return TailStages<P, D, F, G>{p, d, f, g}; }

// ACT >= 0: the activation is a compile-time fact (one epilogue in the code); ACT < 0: `act` selects it at run time.
// TL != NoTail: instead of the epilogue every finished accumulator is handed to (*tl)(acc, column tile, row tile) -- the fused
// per-step tail of the output layer (KSpec::FUSE: sampling, next state, reward, next input straight from the registers).
// LD > 0: the LDS row stride is a compile-time fact (shape-specialised instances): the A-fragment reads of the R row tiles become
// ONE base register + immediate offsets (ds_read_b128 ... offset:r * 16 * LD * 4), no per-row address arithmetic in the k loop.
// SPL: every unit sums its even and its odd k-steps in two accumulators and adds them at the end -- the order a wave whose whole
// share is ONE unit uses anyway (hazard (2) below).  The OUTPUT layer runs with SPL in every instance: its columns are dealt to
// the waves differently by the natural and the head-pair packs, and with SPL a column's sum does not depend on whether its wave
// holds one unit or several -- shape-specialised and generic instances keep returning the same bits.
// KCS > 0: the number of k chunks is a compile-time fact (ops whose K is the hidden width of a shape-specialised instance): the
// k loop is fully unrolled -- straight-line code, no loop control, no accumulator copies where blocks meet.
// x * rcp(1 + exp2(-x log2 e)) on the 4 accumulator values of a lane: the two multiplies and the add as packed 2 x f32 ops
__device__ __forceinline__ f32x4 silu4(const f32x4 a) {
    using f32x2 = __attribute__((ext_vector_type(2))) float;
    const f32x2 k = {-1.44269504088896340736f, -1.44269504088896340736f}, one = {1.0f, 1.0f};
    const f32x2 lo = {a[0], a[1]}, hi = {a[2], a[3]};
    f32x2 tl = lo * k, th = hi * k;
    tl[0] = __builtin_amdgcn_exp2f(tl[0]); tl[1] = __builtin_amdgcn_exp2f(tl[1]);
    th[0] = __builtin_amdgcn_exp2f(th[0]); th[1] = __builtin_amdgcn_exp2f(th[1]);
    tl = tl + one; th = th + one;
    tl[0] = __builtin_amdgcn_rcpf(tl[0]); tl[1] = __builtin_amdgcn_rcpf(tl[1]);
    th[0] = __builtin_amdgcn_rcpf(th[0]); th[1] = __builtin_amdgcn_rcpf(th[1]);
    const f32x2 yl = lo * tl, yh = hi * th;
    return f32x4{yl[0], yl[1], yh[0], yh[1]};
}

// K-SPLIT of the leftover column tile (one-tile workgroups, round 5; KSpec::KSPLIT).  A hidden layer of 13 column tiles deals 4-3-3-3
// tiles to the four waves: the wave with four sets the pace of every layer (200 of its 4 x 50 MFMA k-steps against 150 of the
// others), and at R = 1 nothing else runs on the CU.  Instead the 13th tile's K RANGE is dealt to the waves -- wave w takes the k
// chunks [w KC / 4, (w + 1) KC / 4) of it, at most kKsSlots -- so every wave issues 3 x 50 + 16 k-steps, and the four partial sums
// meet LAZILY: a wave leaves its partial (pre-activation; wave 0's starts at the bias) in LDS as the f32x4 its lanes hold -- which,
// formed transposed, is exactly the B-operand fragment layout of the NEXT op's last k chunk (`lds_col`) -- and after the layer's
// ordinary barrier every wave of the next op reads the four partials of its lane, adds them in one fixed order ((P0 + P1) + (P2 + P3))
// and applies the activation: that IS its fragment of the last chunk.  No extra barrier, no extra pass; 4 ds_read_b128 + ~20 VALU
// instructions per wave and layer against 34 k-steps (~1.1 k cycles) fewer on the critical wave.  The hidden columns 192..207 are
// summed in another order than in the other instances: KSPLIT instances agree with them to rounding (tests: T2 against the oracle),
// not bit for bit.  Two partial buffers alternate by layer parity (a fast wave may finish layer l + 1 while a slow one still reads
// layer l's partials).
constexpr int kKsSlots = 4;  // k chunks of the split tile per wave (KC <= 16: hidden widths up to 256, inputs up to 256 columns)
struct KsArgs {
    const float* part_in;  // KSI: [kWaves][64][4] the producer's partial sums of this op's LAST k chunk
    float* part_out;       // KSO: [kWaves][64][4] this op's partial sums of its split column tile
    int tile;              // KSO: the split column tile (the op's last)
    int k0, n;             // KSO: this wave's chunks [k0, k0 + n) of it
    int wave;
};

// KS bit 0 (KSI): the input image's last k chunk is NOT in LDS -- it is rebuilt from ks->part_in; bit 1 (KSO): see above;
// bit 2: no k-split, only the one-tile k loop that fetches two chunks ahead (kTriple: ops with a static chunk count, planet.hpp)
// RES: 1 = the op's head is *rh (resident, see ResHead); 3 = one of rh[0..2], chosen by the wave-uniform rsel (the hidden-fed layers share
// one code body: only the head -- bias init + chunk-0 MFMAs -- exists per layer, behind a switch; the rest of the k loop once)
template <int R, int CT, int EX, int ACT, class TL = NoTail, int LD = -1, bool SPL = false, int KCS = -1, int KS = 0, int RES = 0>
__device__ __forceinline__ void wave_gemm(const float* __restrict__ in, float* __restrict__ out, const int ld_rt,
                                          const float* __restrict__ W, const float* __restrict__ bias, const int KC_rt,
                                          const int tail_steps, const int c_first, const Extras ex,
                                          const bool apply_act, const int act, const float slope, const int lane,
                                          Prof& prof, const TL* tl = nullptr, const int ldi_rt = 0, const KsArgs* ks = nullptr,
                                          const ResHead* rh = nullptr, const int rsel = 0) {
    static_assert(!RES || (LD > 0 && KS == 0 && R >= 3 && CT <= 3 && EX <= 3), "resident heads: shape-specialised one-wave-per-SIMD instances");
    constexpr int CTn = CT > 0 ? CT : 1;
    constexpr int EXn = EX > 0 ? EX : 1;
    constexpr bool KSI = (KS & 1) != 0, KSO = (KS & 2) != 0;
    static_assert(!KS || (R == 1 && LD > 0), "k-split: one-tile shape-specialised instances, rolled k loop");
    static_assert(!KSO || (std::is_same<TL, NoTail>::value && EX == 0 && !SPL), "k-split producer: a hidden op");
    f32x4 acc[CTn][R];
    f32x4 accx[EXn];
    const int ld = LD > 0 ? LD : ld_rt;
    const int ldi = ldi_rt > 0 ? ldi_rt : ld;  // row stride of `in` when it differs from the output's (KSpec::WIDE: the model-input image)
    const int KC = KCS > 0 ? KCS : KC_rt;
    // one wave per SIMD, shape-specialised, no k-split: the ops whose run-time choices are conditional k-steps (mfma_kstep_if), not branches
    constexpr bool kStraight = LD > 0 && MinWavesOf<R>::value == 1 && KS == 0;
    const int tail_sgpr = kStraight ? __builtin_amdgcn_readfirstlane(tail_steps) : tail_steps;

    const int exc[kMaxExtras] = {ex.c0, ex.c1, ex.c2, ex.c3};
    const int exr[kMaxExtras] = {ex.r0, ex.r1, ex.r2, ex.r3};
    // per-lane BYTE offsets from the (wave-uniform) chunk base W + 256 kk floats: loop invariant, unsigned 32 bit, so the
    // loads take the scalar-base form (global_load v, v_off, s[base]) and the k loop carries no 64-bit address VALU work
    // (a wave's own VALU instructions do not overlap its MFMAs, profiles/microbench)
    unsigned woff[CTn], wxoff[EXn];
    int axoff[EXn];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) woff[ct] = (unsigned)(((c_first + kWaves * ct) * KC * 64 + lane) * 16);
#pragma unroll
    for (int e = 0; e < EX; ++e) {
        wxoff[e] = (unsigned)((exc[e] * KC * 64 + lane) * 16);
        axoff[e] = exr[e] * 16 * ldi;
    }
    const float* ap = in + (lane & 15) * ldi + 4 * (lane >> 4);
    // biases of this lane's columns: loaded before the k loop so their latency hides behind it
    f32x4 bv[CTn], bvx[EXn];
    if constexpr (!RES) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) bv[ct] = *reinterpret_cast<const f32x4*>(bias + (c_first + kWaves * ct) * 16 + 4 * (lane >> 4));
#pragma unroll
    for (int e = 0; e < EX; ++e) bvx[e] = *reinterpret_cast<const f32x4*>(bias + exc[e] * 16 + 4 * (lane >> 4));
    }
    // The weight block of this op as a raw buffer (base = W, wave-uniform): a fragment load is buffer_load_dwordx4 v, v_off, s[rsrc],
    // s_chunk offen -- the loop-invariant per-lane offset in a VGPR, the chunk offset (kk KiB) in an SGPR, NO address VALU work in
    // the k loop (fp32 MFMAs and VALU instructions exclude each other on a SIMD: every v_lshl_add_u64 there is MFMA-pipe idle time)
    // (W is wave-uniform by construction -- member and layer are -- but parts of it came through LDS, which the compiler's divergence
    // analysis cannot see: without the readfirstlane it wraps every buffer_load in a waterfall loop)
    const unsigned long long wbits = reinterpret_cast<unsigned long long>(W);
    const unsigned long long wuni = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(wbits >> 32)) << 32) |
                                    (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)wbits);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(wuni), 0, 0x7FFFFFFF, 0x00020000);
    auto wload = [&](const unsigned voff, const int kk) __attribute__((always_inline)) {
        const u32x4g v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)voff, kk * 1024, 0);
        f32x4 r;
        __builtin_memcpy(&r, &v, 16);
        return r;
    };
    auto load = [&](GemmFrags<R, CT, EX>& f, const int kk) __attribute__((always_inline)) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) f.b[ct] = wload(woff[ct], kk);
#pragma unroll
        for (int e = 0; e < EX; ++e) f.bx[e] = wload(wxoff[e], kk);
#pragma unroll
        for (int r = 0; r < R; ++r) f.a[r] = *reinterpret_cast<const f32x4*>(ap + r * 16 * ldi + kk * 16);
#pragma unroll
        for (int e = 0; e < EX; ++e) f.ax[e] = *reinterpret_cast<const f32x4*>(ap + axoff[e] + kk * 16);
    };
    // Hazards the compiler cannot see inside asm: (1) a VALU write (e.g. a phi copy of an accumulator) must be
    // >= 2 wait states ahead of the MFMA that reads it -> s_nop 1 opens every k-step; (2) an MFMA that takes the
    // previous MFMA's D as C back-to-back (issue interval 32 < dependent latency 40 cycles) reads a stale C on
    // VGPR accumulators -> a wave whose whole share is ONE unit alternates two accumulators (even / odd k-steps).
    constexpr bool kSplit = (CT * R + EX) == 1;
    constexpr bool kSplitAll = SPL && !kSplit;
    f32x4 acc_odd = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acco[CTn][R], accxo[EXn];  // kSplitAll: the odd k-steps of every unit
#pragma unroll
    for (int ct = 0; ct < CTn; ++ct)
#pragma unroll
        for (int r = 0; r < R; ++r) acco[ct][r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < EXn; ++e) accxo[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto kstep = [&](const GemmFrags<R, CT, EX>& f, const int s) __attribute__((always_inline)) {
        asm volatile("s_nop 1");
        if constexpr (kSplit) {
            f32x4& dst = (s & 1) ? acc_odd : (CT ? acc[0][0] : accx[0]);
            if constexpr (CT) mfma16x16x4(f.b[0][s], f.a[0][s], dst);
            else mfma16x16x4(f.bx[0][s], f.ax[0][s], dst);
        } else if constexpr (kSplitAll) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < R; ++r) mfma16x16x4(f.b[ct][s], f.a[r][s], (s & 1) ? acco[ct][r] : acc[ct][r]);
#pragma unroll
            for (int e = 0; e < EX; ++e) mfma16x16x4(f.bx[e][s], f.ax[e][s], (s & 1) ? accxo[e] : accx[e]);
        } else {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < R; ++r) mfma16x16x4(f.b[ct][s], f.a[r][s], acc[ct][r]);
#pragma unroll
            for (int e = 0; e < EX; ++e) mfma16x16x4(f.bx[e][s], f.ax[e][s], accx[e]);
        }
    };
    auto compute = [&](const GemmFrags<R, CT, EX>& f) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s) kstep(f, s);
    };
    // Interleaved form of "load the next chunk, then compute this one": the kNL fragment loads of chunk
    // kk_next are issued ONE AT A TIME, evenly spread behind the MFMAs of the current chunk, instead of as a clump in front of it.
    // Measured stand-alone (profiles/microbench/kloop_probe.hip, this wave's 3 x 3 + 1 tiling, 220 workgroups): a VMEM / LDS
    // instruction issued while no MFMA is executing costs ~12 cycles of matrix-pipe idle time (8 per 40 MFMAs: 34.46 cycles per
    // MFMA); issued inside an MFMA's 32-cycle shadow it is free (32.98).  Weight fragments first: they have the L2 round trip
    // ahead of them and are needed >= 30 MFMAs (~1 000 cycles) later; the LDS fragments follow in the order the next chunk's first
    // MFMAs consume them.  sched_barrier(0) on both sides pins each load where it is written.
    constexpr bool kIL = LD > 0;  // shape-specialised instances only: in the generic ones (every shape x activation in one kernel, at the
                                  // 256-VGPR limit) the longer live ranges spill 16-20 VGPRs to scratch
    constexpr int kNU = CT * R + EX;                              // MFMA units of this wave
    constexpr int kNL = CT + EX + (CT > 0 ? R : 0) + EX;          // fragment loads per chunk
    static_assert(4 * kNU >= kNL + 1, "every load needs its own slot behind an MFMA");
    auto load_one = [&](GemmFrags<R, CT, EX>& g, const int kk, const int i) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        if (i < CT) g.b[i < CT ? i : 0] = wload(woff[i < CT ? i : 0], kk);
        else if (i < CT + EX) g.bx[i - CT] = wload(wxoff[i - CT], kk);
        else if (CT > 0 && i < CT + EX + R) g.a[i - CT - EX] = *reinterpret_cast<const f32x4*>(ap + (i - CT - EX) * 16 * ldi + kk * 16);
        else {
            const int e = i - CT - EX - (CT > 0 ? R : 0);
            g.ax[e] = *reinterpret_cast<const f32x4*>(ap + axoff[e] + kk * 16);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mfma_unit = [&](const GemmFrags<R, CT, EX>& f, const int s, const int u) __attribute__((always_inline)) {
        if constexpr (kSplit) {
            f32x4& dst = (s & 1) ? acc_odd : (CT ? acc[0][0] : accx[0]);
            if constexpr (CT) mfma16x16x4(f.b[0][s], f.a[0][s], dst);
            else mfma16x16x4(f.bx[0][s], f.ax[0][s], dst);
        } else if (u < CT * R) {
            const int ct = u / R, r = u - ct * R;
            if constexpr (kSplitAll) mfma16x16x4(f.b[ct][s], f.a[r][s], (s & 1) ? acco[ct][r] : acc[ct][r]);
            else mfma16x16x4(f.b[ct][s], f.a[r][s], acc[ct][r]);
        } else {
            const int e = u - CT * R;
            if constexpr (kSplitAll) mfma16x16x4(f.bx[e][s], f.ax[e][s], (s & 1) ? accxo[e] : accx[e]);
            else mfma16x16x4(f.bx[e][s], f.ax[e][s], accx[e]);
        }
    };
    // after MFMA number m1 (1-based) of the chunk: the loads whose slot this is.  Load j goes behind MFMA (j + 1) * total / (kNL + 1):
    // evenly spread, the last one still several MFMAs ahead of the chunk's end (the next chunk's first MFMAs want its data).
    // Plain nested loops with compile-time bounds and an explicit `#pragma unroll` each: every array index must be a constant
    // after unrolling (a dynamically indexed fragment array is demoted to scratch memory -- measured: 28 ms per rollout).
    auto loads_behind = [&](GemmFrags<R, CT, EX>& g, const int kk_next, const int m1) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kNL; ++j)
            if (((j + 1) * 4 * kNU) / (kNL + 1) == m1) load_one(g, kk_next, j);
    };
    auto compute_il = [&](const GemmFrags<R, CT, EX>& f, GemmFrags<R, CT, EX>& g, const int kk_next) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            asm volatile("s_nop 1");  // hazard guard of kstep above
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    mfma_unit(f, ks, ct * R + r);
                    loads_behind(g, kk_next, ks * kNU + ct * R + r + 1);
                }
#pragma unroll
            for (int e = 0; e < EX; ++e) {
                mfma_unit(f, ks, CT * R + e);
                loads_behind(g, kk_next, ks * kNU + CT * R + e + 1);
            }
        }
    };
    // The compiler models an asm MFMA as an ordinary instruction whose result is ready immediately, so any VALU
    // copy of an accumulator it places right behind one (phi copies where control flow merges) would read the
    // register before the matrix pipe has written it.  drain_all() = wait out the pipe, then re-define every
    // accumulator through an empty asm so such copies can only be scheduled after the wait.  It ends every
    // conditional arm below and follows the main loop; the loop body itself is branch-free and in place.
    auto drain_all = [&]() __attribute__((always_inline)) {
        mfma_drain();
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acc[ct][r]));
#pragma unroll
        for (int e = 0; e < EX; ++e) asm volatile("" : "+v"(accx[e]));
        asm volatile("" : "+v"(acc_odd));
        if constexpr (kSplitAll) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int r = 0; r < R; ++r) asm volatile("" : "+v"(acco[ct][r]));
#pragma unroll
            for (int e = 0; e < EX; ++e) asm volatile("" : "+v"(accxo[e]));
        }
    };
    // k-step S of `f` if n > S (mfma_kstep_if above; n wave-uniform): the wave's units in as few statements as the operand limit allows --
    // one, but for the 13 units of an R = 4 wave (two column tiles, then the third with the extra unit).  WA: weights from a resident head.
    auto kstep_if = [&](const auto& wb, const auto& wbx, const GemmFrags<R, CT, EX>& f, auto sc, auto wa, const int n) __attribute__((always_inline)) {
        constexpr int S = decltype(sc)::value;
        constexpr bool WA = decltype(wa)::value;
        constexpr bool odd = (S & 1) != 0;
        float ea[R] = {}, eax[EXn] = {}, ebx[EXn] = {};
        f32x4* px[EXn] = {};
#pragma unroll
        for (int r = 0; r < (CT > 0 ? R : 0); ++r) ea[r] = f.a[r][S];
#pragma unroll
        for (int e = 0; e < EX; ++e) {
            eax[e] = f.ax[e][S];
            ebx[e] = wbx[e][S];
            px[e] = (kSplitAll && odd) ? &accxo[e] : ((kSplit && odd) ? &acc_odd : &accx[e]);
        }
        if constexpr (kSplit && CT > 0) {  // (not produced by the shape tables: a lone strided tile at R = 1 only)
            static_assert(R < 0, "conditional k-step: one strided unit");
        } else if constexpr (2 * (CT * R + EX) + CT + (CT > 0 ? R : 0) + 2 * EX + 1 <= 30) {
            f32x4* pc[CTn][R] = {};
            float eb[CTn] = {};
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                eb[ct] = wb[ct][S];
#pragma unroll
                for (int r = 0; r < R; ++r) pc[ct][r] = (kSplitAll && odd) ? &acco[ct][r] : &acc[ct][r];
            }
            mfma_kstep_if<R, CT, EX, S, WA>(n, pc, px, eb, ea, ebx, eax);
        } else {
            static_assert(CT == 3, "two statements: the widest share is three column tiles and the extra units");
            f32x4* p01[2][R];
            f32x4* p2[1][R];
            float e01[2], e2[1];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                e01[ct] = wb[ct][S];
#pragma unroll
                for (int r = 0; r < R; ++r) p01[ct][r] = (kSplitAll && odd) ? &acco[ct][r] : &acc[ct][r];
            }
            e2[0] = wb[2][S];
#pragma unroll
            for (int r = 0; r < R; ++r) p2[0][r] = (kSplitAll && odd) ? &acco[2][r] : &acc[2][r];
            f32x4* pnone[1] = {nullptr};
            const float enone[1] = {0.f};
            mfma_kstep_if<R, 2, 0, S, WA>(n, p01, pnone, e01, ea, enone, enone);
            mfma_kstep_if<R, 1, EX, S, WA>(n, p2, px, e2, ea, ebx, eax);
        }
    };
    // last chunk: only the k-steps that hold real (non-padding) weights, e.g. 2 of 4 for K = 200
    auto compute_tail = [&](const GemmFrags<R, CT, EX>& f) __attribute__((always_inline)) {
        if constexpr (kStraight) {  // k-step 0 always runs; 1..3 skip themselves inside their asm statement: nothing here for the compiler to merge
            kstep(f, 0);
            kstep_if(f.b, f.bx, f, std::integral_constant<int, 1>{}, std::false_type{}, tail_sgpr);
            kstep_if(f.b, f.bx, f, std::integral_constant<int, 2>{}, std::false_type{}, tail_sgpr);
            kstep_if(f.b, f.bx, f, std::integral_constant<int, 3>{}, std::false_type{}, tail_sgpr);
            return;
        }
        switch (tail_steps) {
            case 1: kstep(f, 0); drain_all(); break;
            case 2: kstep(f, 0); kstep(f, 1); drain_all(); break;
            case 3: kstep(f, 0); kstep(f, 1); kstep(f, 2); drain_all(); break;
            default: kstep(f, 0); kstep(f, 1); kstep(f, 2); kstep(f, 3); drain_all(); break;
        }
    };

    // sched_barrier(0) pins "issue the next chunk's loads, THEN this chunk's MFMAs": without it the machine
    // scheduler sinks each load group down to its first use and the pipeline degenerates to load->wait->compute.
    // k-split: the partials of the input's last chunk (KSI) and this wave's share of the split tile (KSO: its weight and activation
    // fragments, ALL requested up front -- unused slots read chunk 0 and are zeroed below: straight-line code, no branch around an MFMA)
    f32x4 ks_p[kWaves], ks_b[kKsSlots], ks_a[kKsSlots], ks_bias = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (KSI) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) ks_p[w] = *reinterpret_cast<const f32x4*>(ks->part_in + (w * 64 + lane) * 4);
    }
    if constexpr (KSO) {
        const unsigned xoff = (unsigned)((ks->tile * KC * 64 + lane) * 16);
        ks_bias = *reinterpret_cast<const f32x4*>(bias + ks->tile * 16 + 4 * (lane >> 4));
#pragma unroll
        for (int j = 0; j < kKsSlots; ++j) {
            const int c = j < ks->n ? ks->k0 + j : 0;
            ks_b[j] = wload(xoff, c);
            ks_a[j] = *reinterpret_cast<const f32x4*>(ap + c * 16);
        }
    }
    GemmFrags<R, CT, EX> f0, f1;
    if constexpr (RES) {  // chunk 0: the weight fragments are resident, only the activation fragments (LDS) are fetched
#pragma unroll
        for (int r = 0; r < (CT > 0 ? R : 0); ++r) f0.a[r] = *reinterpret_cast<const f32x4*>(ap + r * 16 * ldi);
#pragma unroll
        for (int e = 0; e < EX; ++e) f0.ax[e] = *reinterpret_cast<const f32x4*>(ap + axoff[e]);
    } else {
        load(f0, 0);
    }
    // One-tile k-split instances fetch TWO chunks ahead (kTriple below): a wave's 12 MFMAs per chunk (384 cycles) are no cover for an
    // L2 round trip issued somewhere inside the previous chunk
    // (ops whose chunk count is a compile-time fact -- KCS: everything fed by a hidden layer -- so that the loop's remainder is no run-time
    // branch: the allocator copies accumulators where such arms begin and sinks the copies to just in front of their first MFMA)
    constexpr bool kTriple = KS != 0 && KCS > 0 && LD > 0;
    static_assert(!KS || KCS <= 0 || kTriple, "k-split ops with a static chunk count run the three-set loop");
    if constexpr (kTriple) load(f1, KCS > 1 ? 1 : 0);
    // accumulators start at the bias (C input of the first MFMA) instead of zero: no add in the epilogue.  Initialised AFTER
    // chunk 0's fragment loads were issued: the bias loads are older, so waiting for them leaves the fragments in flight
    // (initialising first serialised two L2 round trips per layer: ~1.2k cycles of "set-up" per layer in the phase profile)
    // Pin every accumulator's initial value HERE: to the compiler an asm MFMA is an ordinary reader of its C operand, so it may
    // sink the (VALU) initialisation -- a copy of the bias, the zeros of the odd-k-step accumulators -- down to just in front of
    // the first MFMA that uses the register, inside a k-step, behind that k-step's s_nop: a VALU write followed at once by an MFMA
    // reading it as SrcC (hazard (1) below; found in the ISA of the cfg4 instances by __graft_entry__.scan_isa_hazards (tests/test_abi.py), where it returned
    // wrong sums).  An empty asm that "modifies" the register makes the value opaque: it must be complete before this point.
    auto pin = [](f32x4& v) __attribute__((always_inline)) { asm volatile("" : "+v"(v)); };
    // ... and the same with the number of the forked body it stands in (kForked below) as an asm comment: identical statements in every
    // body are hoisted back in front of the fork, and each body then begins by copying the accumulators it was to initialise itself
    auto pin_in = [](f32x4& v, auto body) __attribute__((always_inline)) {
        if constexpr (decltype(body)::value == 0) asm volatile("" : "+v"(v));
        else asm volatile("; body %1" : "+v"(v) : "n"(decltype(body)::value));
    };
    auto acc_from_bias = [&](auto body) __attribute__((always_inline)) {
#pragma unroll
        for (int ct = 0; ct < CTn; ++ct)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[ct][r] = CT > 0 ? bv[ct] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < EXn; ++e) accx[e] = EX > 0 ? bvx[e] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ct = 0; ct < CTn; ++ct)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if constexpr (CT > 0) pin_in(acc[ct][r], body);
                if constexpr (CT > 0 && kSplitAll) pin_in(acco[ct][r], body);
            }
#pragma unroll
        for (int e = 0; e < EXn; ++e) {
            if constexpr (EX > 0) pin_in(accx[e], body);
            if constexpr (EX > 0 && kSplitAll) pin_in(accxo[e], body);
        }
        if constexpr (kSplit) pin_in(acc_odd, body);
        prof.mark(14);
    };
    // (an op that forks into whole bodies -- kStraight with a run-time chunk count, below -- initialises inside each body)
    constexpr bool kForked = kStraight && KCS <= 0;
    if constexpr (!RES && !kForked) acc_from_bias(std::integral_constant<int, 0>{});
    f32x4 a_last = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (KSI) {  // this lane's fragment of the input's last chunk: the activation of the four partial sums, in ONE fixed order
        static_assert(ACT == HIPETS_ACT_SILU, "k-split instances are SiLU instances");
        a_last = silu4((ks_p[0] + ks_p[1]) + (ks_p[2] + ks_p[3]));
    }
    f32x4 ks_e = f32x4{0.f, 0.f, 0.f, 0.f}, ks_o = f32x4{0.f, 0.f, 0.f, 0.f};  // even / odd k-steps of the split tile (hazard (2) above)
    if constexpr (KSO) {
        // Wave-uniform choices as ARITHMETIC (a multiply by 1.0f or 0.0f from an SGPR: exact on finite values), never as control flow:
        // written as `if`s the compiler built a web of ~40 scalar branches around these 20 register writes
        ks_e = ks_bias * (ks->wave == 0 ? 1.0f : 0.0f);  // the sum of the four partials carries the bias once
#pragma unroll
        for (int j = 0; j < kKsSlots; ++j) ks_b[j] = ks_b[j] * (j < ks->n ? 1.0f : 0.0f);  // unused slot: 0 x (a valid activation of chunk 0)
        if constexpr (KSI) {
            // the input's last chunk lives in registers (a_last), not in LDS.  In an op fed by a hidden layer it is the LAST slot of the
            // LAST wave (KC = 13 .. 16: wave 3 holds chunks [3 KC / 4, KC), four of them); on the other waves that slot is unused (zero
            // weights), so it may hold the same finite values there: no selection at all
            HIPETS_BOUND(KC >= 13 && KC <= 16);
            ks_a[kKsSlots - 1] = a_last;
        }
        pin(ks_e);
        pin(ks_o);
#pragma unroll
        for (int j = 0; j < kKsSlots; ++j) {
            pin(ks_b[j]);
            pin(ks_a[j]);
        }
#pragma unroll
        for (int j = 0; j < kKsSlots; ++j)
#pragma unroll
            for (int s_ = 0; s_ < 4; ++s_) {
                asm volatile("s_nop 1");
                mfma16x16x4(ks_b[j][s_], ks_a[j][s_], (s_ & 1) ? ks_o : ks_e);
            }
        prof.mark(7);  // (profiling builds) the k-split share: its loads' round trip + 16 MFMAs
    }
    if constexpr (RES != 0) {
        auto acc_init = [&](const f32x4* const b, const f32x4* const bx) __attribute__((always_inline)) {
#pragma unroll
            for (int ct = 0; ct < CTn; ++ct)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[ct][r] = CT > 0 ? b[ct] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < EXn; ++e) accx[e] = EX > 0 ? bx[e] : f32x4{0.f, 0.f, 0.f, 0.f};
        };
        auto pin_acc = [&](auto body) __attribute__((always_inline)) {
#pragma unroll
            for (int ct = 0; ct < CTn; ++ct)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if constexpr (CT > 0) pin_in(acc[ct][r], body);
                    if constexpr (CT > 0 && kSplitAll) pin_in(acco[ct][r], body);
                }
#pragma unroll
            for (int e = 0; e < EXn; ++e) {
                if constexpr (EX > 0) pin_in(accx[e], body);
                if constexpr (EX > 0 && kSplitAll) pin_in(accxo[e], body);
            }
            if constexpr (kSplit) pin_in(acc_odd, body);
        };
        // Resident head (RES): the accumulators start from the resident bias (v_accvgpr_read: VALU writes, pinned ahead of the k-step's
        // s_nop like every initial value), then chunk 0 with the weight operand in AccVGPRs; chunk 1's fragment loads ride behind its
        // MFMAs exactly as compute_il places them.  An op of ONE chunk runs its tail steps from the head.  Every arm ends drained.
        auto mfma_unit_h = [&](const ResHead& h, const GemmFrags<R, CT, EX>& f, const int s, const int u) __attribute__((always_inline)) {
            if constexpr (kSplit) {
                f32x4& dst = (s & 1) ? acc_odd : (CT ? acc[0][0] : accx[0]);
                if constexpr (CT) mfma16x16x4_ra(h.b[0][s], f.a[0][s], dst);
                else mfma16x16x4_ra(h.bx[0][s], f.ax[0][s], dst);
            } else if (u < CT * R) {
                const int ct = u / R, r = u - ct * R;
                if constexpr (kSplitAll) mfma16x16x4_ra(h.b[ct][s], f.a[r][s], (s & 1) ? acco[ct][r] : acc[ct][r]);
                else mfma16x16x4_ra(h.b[ct][s], f.a[r][s], acc[ct][r]);
            } else {
                const int e = u - CT * R;
                if constexpr (kSplitAll) mfma16x16x4_ra(h.bx[e][s], f.ax[e][s], (s & 1) ? accxo[e] : accx[e]);
                else mfma16x16x4_ra(h.bx[e][s], f.ax[e][s], accx[e]);
            }
        };
        auto head_init = [&](const ResHead& h, auto body) __attribute__((always_inline)) {
            acc_init(h.bv, h.bvx);
            pin_acc(body);
            prof.mark(14);
        };
        auto head_full = [&](const ResHead& h) __attribute__((always_inline)) {  // chunk 0, chunk 1's fragments on their way into f1
#pragma unroll
            for (int ks_ = 0; ks_ < 4; ++ks_) {
                asm volatile("s_nop 1");
#pragma unroll
                for (int u = 0; u < kNU; ++u) {
                    mfma_unit_h(h, f0, ks_, u);
                    loads_behind(f1, 1, ks_ * kNU + u + 1);
                }
            }
        };
        if constexpr (KCS > 0) {
            // ops fed by a hidden layer: straight-line code behind the head (the only choice left is WHICH head: the arms of the layer switch)
            static_assert(KCS >= 2, "a hidden width of more than one chunk");
            auto head = [&](const ResHead& h) __attribute__((always_inline)) {
                head_init(h, std::integral_constant<int, 0>{});
                head_full(h);
                if constexpr (RES == 3) drain_all();  // (an arm of the layer switch)
            };
            if constexpr (RES == 1) {
                head(rh[0]);
            } else {
                switch (rsel) {
                    case 0: head(rh[0]); break;
                    case 1: head(rh[1]); break;
                    default: head(rh[2]); break;
                }
            }
            // chunks 1 .. KCS - 1: the two-set loop with the sets' roles swapped (chunk 1 is in f1)
#pragma unroll
            for (int k2 = 1; k2 + 2 < KCS; k2 += 2) {
                compute_il(f1, f0, k2 + 1);
                compute_il(f0, f1, k2 + 2);
            }
            constexpr int kEndR = KCS >= 3 ? 1 + ((KCS - 2) / 2) * 2 : 1;  // where that loop leaves k2: the largest odd number <= KCS - 1
            if constexpr (kEndR + 1 < KCS) {
                compute_il(f1, f0, kEndR + 1);
                compute_tail(f0);
            } else {
                compute_tail(f1);
            }
        } else {
            // The input layer (run-time chunk count): the op forks ONCE, before its first MFMA, into a whole body per case -- one chunk /
            // an even / an odd number of them -- and the bodies meet in front of the epilogue.  Inside a body the fragment set the tail
            // reads is fixed, so nothing merges between MFMAs (forking behind the loop, "one chunk left or two", cost a copy of every
            // accumulator where the arms began and met, and a drain each).  Every body ends drained: the epilogue's own wait is dropped.
            // The accumulators are initialised INSIDE each body (pin_in): initialised in front of the fork, every body began by copying them.
            static_assert(RES == 1, "one head");
            const ResHead& h = rh[0];
            if (KC < 2) {  // the head IS the tail chunk
                head_init(h, std::integral_constant<int, 1>{});
                asm volatile("s_nop 1");
#pragma unroll
                for (int u = 0; u < kNU; ++u) mfma_unit_h(h, f0, 0, u);
                kstep_if(h.b, h.bx, f0, std::integral_constant<int, 1>{}, std::true_type{}, tail_sgpr);
                kstep_if(h.b, h.bx, f0, std::integral_constant<int, 2>{}, std::true_type{}, tail_sgpr);
                kstep_if(h.b, h.bx, f0, std::integral_constant<int, 3>{}, std::true_type{}, tail_sgpr);
                drain_all();
            } else if ((KC & 1) == 0) {  // chunks 1 .. KC - 1 are an odd number: pairs, then the tail from f1
                head_init(h, std::integral_constant<int, 2>{});
                head_full(h);
                for (int kk = 1; kk + 2 < KC; kk += 2) {
                    compute_il(f1, f0, kk + 1);
                    compute_il(f0, f1, kk + 2);
                }
                compute_tail(f1);
                drain_all();
            } else {  // an even number: pairs, one more full chunk, the tail from f0
                head_init(h, std::integral_constant<int, 3>{});
                head_full(h);
                int kk = 1;
                for (; kk + 2 < KC; kk += 2) {
                    compute_il(f1, f0, kk + 1);
                    compute_il(f0, f1, kk + 2);
                }
                compute_il(f1, f0, kk + 1);
                compute_tail(f0);
                drain_all();
            }
        }
    } else if constexpr (KCS > 0 && !kTriple) {
        constexpr int kEnd = KCS >= 2 ? ((KCS - 1) / 2) * 2 : 0;  // the loop below leaves kk at the smallest even number >= KCS - 2
#pragma unroll
        for (int kk = 0; kk + 2 < KCS; kk += 2) {
            if constexpr (kIL) {
                compute_il(f0, f1, kk + 1);
                compute_il(f1, f0, kk + 2);
            } else {
                load(f1, kk + 1);
                __builtin_amdgcn_sched_barrier(0);
                compute(f0);
                __builtin_amdgcn_sched_barrier(0);
                load(f0, kk + 2);
                __builtin_amdgcn_sched_barrier(0);
                compute(f1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (kEnd + 1 < KCS) {
            if constexpr (kIL) {
                compute_il(f0, f1, kEnd + 1);
            } else {
                load(f1, kEnd + 1);
                __builtin_amdgcn_sched_barrier(0);
                compute(f0);
                __builtin_amdgcn_sched_barrier(0);
            }
            compute_tail(f1);
        } else {
            compute_tail(f0);
        }
    } else if constexpr (kTriple) {
        // three fragment sets in rotation: chunk kk is computed from one while chunk kk + 2 is being fetched into another (measured
        // on MI355X, one-tile workgroups, round 5: with one chunk of lead the k loop of a wave with 3 column tiles ran at the pace of
        // the L2 round trips, not of its MFMAs -- profiles/r5_small_batches.json)
        GemmFrags<R, CT, EX> f2;
        auto last_frag = [&](GemmFrags<R, CT, EX>& f) __attribute__((always_inline)) {  // KSI: see the two-set loop below
            if constexpr (KSI) {
                if constexpr (CT > 0) f.a[0] = a_last;
#pragma unroll
                for (int e = 0; e < EX; ++e) f.ax[e] = a_last;
                if constexpr (CT > 0) pin(f.a[0]);
#pragma unroll
                for (int e = 0; e < EX; ++e) pin(f.ax[e]);
            }
        };
        constexpr int kEnd3 = KCS >= 3 ? ((KCS - 1) / 3) * 3 : 0;  // where the loop below leaves kk
        constexpr int kRem = KCS - kEnd3;                          // 1 .. 3 chunks left then, the last of them the tail chunk
#pragma nounroll
        for (int kk = 0; kk + 3 < KCS; kk += 3) {  // chunks kk .. kk + 2 are full ones; f0 = chunk kk, f1 = chunk kk + 1 on entry
            compute_il(f0, f2, kk + 2);
            compute_il(f1, f0, kk + 3);
            compute_il(f2, f1, min(kk + 4, KCS - 1));  // (past the end: the last chunk once more, never used)
        }
        drain_all();
        if constexpr (kRem == 1) {
            last_frag(f0);
            compute_tail(f0);
        } else if constexpr (kRem == 2) {
            compute(f0);
            drain_all();
            last_frag(f1);
            compute_tail(f1);
        } else {
            compute_il(f0, f2, kEnd3 + 2);
            compute(f1);
            drain_all();
            last_frag(f2);
            compute_tail(f2);
        }
    } else if constexpr (kStraight) {
        // The input layer (run-time chunk count): forked ONCE on the parity of the count, before the first MFMA, into two whole bodies
        // in which the tail's fragment set is fixed (see the resident twin of this code above); both initialise their accumulators themselves and end drained
        if (KC & 1) {
            acc_from_bias(std::integral_constant<int, 1>{});
            int kk = 0;
            for (; kk + 2 < KC; kk += 2) {
                compute_il(f0, f1, kk + 1);
                compute_il(f1, f0, kk + 2);
            }
            compute_tail(f0);
            drain_all();
        } else {
            acc_from_bias(std::integral_constant<int, 2>{});
            compute_il(f0, f1, 1);
            for (int kk = 1; kk + 2 < KC; kk += 2) {
                compute_il(f1, f0, kk + 1);
                compute_il(f0, f1, kk + 2);
            }
            compute_tail(f1);
            drain_all();
        }
    } else {
        int kk = 0;
        for (; kk + 2 < KC; kk += 2) {  // chunks kk, kk+1 are not the last one
            if constexpr (kIL) {
                compute_il(f0, f1, kk + 1);
                compute_il(f1, f0, kk + 2);
            } else {
                load(f1, kk + 1);
                __builtin_amdgcn_sched_barrier(0);
                compute(f0);
                __builtin_amdgcn_sched_barrier(0);
                load(f0, kk + 2);
                __builtin_amdgcn_sched_barrier(0);
                compute(f1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // (k-split instances drain unconditionally: their register allocation copies the accumulators where the tail's arms begin, and
        // the build's ISA scan cannot know that the path "loop left with results in flight AND kk == 0" does not exist)
        if (KS != 0 || kk > 0) drain_all();
        // KSI: the last chunk's activation fragment is a_last (what the loads above fetched from that LDS position is unwritten space)
        auto last_frag = [&](GemmFrags<R, CT, EX>& f) __attribute__((always_inline)) {
            if constexpr (KSI) {
                if constexpr (CT > 0) f.a[0] = a_last;
#pragma unroll
                for (int e = 0; e < EX; ++e) f.ax[e] = a_last;
                if constexpr (CT > 0) pin(f.a[0]);
#pragma unroll
                for (int e = 0; e < EX; ++e) pin(f.ax[e]);
            }
        };
        if (kk + 1 < KC) {  // two chunks left: kk (full) and kk+1 (tail)
            if constexpr (kIL) {
                compute_il(f0, f1, kk + 1);
            } else {
                load(f1, kk + 1);
                __builtin_amdgcn_sched_barrier(0);
                compute(f0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (KS != 0) drain_all();  // (the allocator copies the accumulators where the tail's arms begin: see above)
            last_frag(f1);
            compute_tail(f1);
        } else {  // one chunk left
            last_frag(f0);
            compute_tail(f0);
        }
    }
    // the fused tail runs over the wave's units in groups of at most kTailGroup: within a group the LDS loads of ALL its units are
    // issued first (prep), then the arithmetic (unit); the slots of one group are dead before the next starts (a wave of a
    // 47-tile output layer holds 6-8 units per pass: all their slots at once would not fit the arch VGPRs)
    constexpr int kNUt = CT * R + EX;
    constexpr int kTailGroup = 4;
    FusedSlot slots[kTailGroup];
    auto unit_c = [&](const int u) __attribute__((always_inline)) { return u < CT * R ? c_first + kWaves * (u / R) : exc[(u >= CT * R && u < kNUt) ? u - CT * R : 0]; };
    auto unit_r = [&](const int u) __attribute__((always_inline)) { return u < CT * R ? u % R : exr[(u >= CT * R && u < kNUt) ? u - CT * R : 0]; };
    if constexpr (!std::is_same<TL, NoTail>::value) {  // the first group's LDS loads: in flight while the matrix pipe drains
#pragma unroll
        for (int k = 0; k < kTailGroup; ++k)
            if (k < kNUt) tl->prep(slots[k < kNUt ? k : 0], unit_c(k), unit_r(k));
    }
    if constexpr (kSplit) {
        mfma_drain();
        if constexpr (CT) acc[0][0] += acc_odd;
        else accx[0] += acc_odd;
    }
    if constexpr (kSplitAll) {
        drain_all();
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[ct][r] += acco[ct][r];
#pragma unroll
        for (int e = 0; e < EX; ++e) accx[e] += accxo[e];
    }
    if constexpr (!kForked) mfma_drain();  // (the bodies of a run-time chunk count end drained)
    __builtin_amdgcn_sched_barrier(0);
    prof.mark(11);
    if constexpr (!std::is_same<TL, NoTail>::value) {
        // (constant trip counts on both levels: every slot / accumulator index must be a constant after unrolling)
#pragma unroll
        for (int g = 0; g < (kNUt + kTailGroup - 1) / kTailGroup; ++g) {
            if (g > 0) {
#pragma unroll
                for (int k = 0; k < kTailGroup; ++k) {
                    const int u = g * kTailGroup + k;
                    if (u < kNUt) tl->prep(slots[k], unit_c(u), unit_r(u));
                }
            }
            static_assert(kTailGroup % 2 == 0, "the draw stage pairs the units of a group");
            // (pair by pair -- draw, unit, unit -- so that only one pair's normals are live at a time: with the whole group's drawn up front
            // three two-workgroups-per-CU instances spilt to scratch memory)
#pragma unroll
            for (int k = 0; k < kTailGroup; k += 2) {
                const int u = g * kTailGroup + k;
                if (u + 1 < kNUt) tl->draw(slots[k], slots[k + 1], unit_c(u), unit_c(u + 1), true);
                else if (u < kNUt) tl->draw(slots[k], slots[k], unit_c(u), unit_c(u), false);
#pragma unroll
                for (int kk = k; kk < k + 2; ++kk) {
                    const int uu = g * kTailGroup + kk;
                    if (uu < CT * R) tl->unit(slots[kk], acc[(uu < CT * R ? uu : 0) / R][(uu < CT * R ? uu : 0) % R], unit_c(uu), unit_r(uu));
                    else if (uu < kNUt) tl->unit(slots[kk], accx[(uu >= CT * R && uu < kNUt) ? uu - CT * R : 0], unit_c(uu), unit_r(uu));
                }
            }
        }
        tl->finish();
        prof.mark(9);  // the fused tail is booked as the "sample" phase
        return;
    }

    if constexpr (KSO) {
        // this wave's partial sum of the split tile -> LDS, as the f32x4 the lane holds (= the next op's fragment layout).  The two
        // accumulators are re-defined behind the drain above: to the compiler an asm MFMA's result is ready at once, and it would
        // otherwise be free to form this sum right behind the mini-loop, while the matrix pipe still writes the registers
        asm volatile("" : "+v"(ks_e));
        asm volatile("" : "+v"(ks_o));
        *reinterpret_cast<f32x4*>(ks->part_out + (ks->wave * 64 + lane) * 4) = ks_e + ks_o;
    }
    // epilogue: D[row = 4*(lane>>4)+i][col = lane&15] -> bias, activation, next layer's A image.
    // The activation switch is hoisted OUT of the element loops: one compact straight-line body per
    // activation (a per-element switch made the hot path stream ~12 KB of mostly-skipped code per layer
    // through the instruction cache: 11k cycles per epilogue instead of ~2k).
    // The product is formed transposed (weights are the MFMA A operand, activations the B operand), so a lane's
    // accumulator holds 4 CONSECUTIVE LDS columns (16c + 4g .. +3; the weight / bias packing pre-permutes the real
    // columns so that this holds in the chunk-transposed layout too) of batch row 16r + (lane & 15): one
    // ds_write_b128 per accumulator instead of four ds_write_b32.
    // actfn maps the 4 accumulator values of a lane at once (lets an activation use packed 2 x f32 VALU instructions:
    // a wave's VALU work is not hidden behind anything here, so the instruction count is the cost)
    auto store = [&](auto actfn) __attribute__((always_inline)) {
        const int j = lane & 15, g4 = 4 * (lane >> 4);
        HIPETS_BOUND(c_first >= 0 && (CT == 0 || (c_first + kWaves * (CT - 1)) * 16 + g4 + 3 < ld) && KC >= 1 && KC * 16 <= ldi);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int col = (c_first + kWaves * ct) * 16 + g4;
#pragma unroll
            for (int r = 0; r < R; ++r) *reinterpret_cast<f32x4*>(out + (r * 16 + j) * ld + col) = actfn(acc[ct][r]);
        }
#pragma unroll
        for (int e = 0; e < EX; ++e) *reinterpret_cast<f32x4*>(out + (exr[e] * 16 + j) * ld + exc[e] * 16 + g4) = actfn(accx[e]);
    };
    auto each = [](auto f) {  // lift a scalar activation to the 4 values
        return [f](const f32x4 a) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = f(a[i]);
            return v;
        };
    };
    if (!apply_act) {
        store([](const f32x4 a) { return a; });
    } else {
        switch (ACT >= 0 ? ACT : act) {
            case HIPETS_ACT_SILU: store([](const f32x4 a) { return silu4(a); }); break;
            case HIPETS_ACT_RELU: store(each([](float x) { return x < 0.0f ? 0.0f : x; })); break;  // NOT fmaxf: v_max_f32 returns 0 for a NaN input, torch.relu returns NaN
            case HIPETS_ACT_LEAKY_RELU: store(each([slope](float x) { return x > 0.0f ? x : slope * x; })); break;
            case HIPETS_ACT_TANH: store(each([](float x) { return tanhf(x); })); break;
            default: store(each([](float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896340736f)); })); break;
        }
    }
    prof.mark(13);
}

template <int R, int CT, int ACT, bool SPL = false>
__device__ __forceinline__ void wave_gemm_ex(int nex, const float* in, float* out, int ld, const float* W,
                                             const float* bias, int KC, int tail_steps, int c_first, const Extras ex,
                                             bool apply_act, int act, float slope, int lane, Prof& prof) {
    // a wave holds at most ceil(3 R / 4) leftover units (C % 4 <= 3 leftover column tiles x R row tiles dealt to 4 waves): only those
    // counts are instantiated (every instance adds to the kernel's register maximum, and the generic kernels sit at the limit)
    constexpr int kMaxEx = (3 * R + kWaves - 1) / kWaves;
    switch (nex) {
        case 0:
            if constexpr (CT > 0) wave_gemm<R, CT, 0, ACT, NoTail, -1, SPL>(in, out, ld, W, bias, KC, tail_steps, c_first, ex, apply_act, act, slope, lane, prof);
            break;
        case 1: wave_gemm<R, CT, 1, ACT, NoTail, -1, SPL>(in, out, ld, W, bias, KC, tail_steps, c_first, ex, apply_act, act, slope, lane, prof); break;
        case 2:
            if constexpr (kMaxEx >= 2) wave_gemm<R, CT, 2, ACT, NoTail, -1, SPL>(in, out, ld, W, bias, KC, tail_steps, c_first, ex, apply_act, act, slope, lane, prof);
            break;
        default:
            if constexpr (kMaxEx >= 3) wave_gemm<R, CT, 3, ACT, NoTail, -1, SPL>(in, out, ld, W, bias, KC, tail_steps, c_first, ex, apply_act, act, slope, lane, prof);
            break;
    }
}

// One linear op (+activation) for the workgroup's 16*R rows: in (LDS) -> out (LDS), both with row stride ld.
// W / bias point at the packed fragments / padded biases of this op (pack_weights_kernel / pack_bias_kernel).
// CS >= 0: the number of column tiles is a compile-time fact (shape-specialised kernels): every wave's (CT, EX) follows
// from it and the wave index through ONE branch, and only the two wave_gemm instances the shape needs are compiled;
// CS < 0: it is read from the layer table and dispatched through the (full, nex) switches.
// KS (shape-specialised ops of one-tile workgroups): wave_gemm's k-split bits; part_in / part_out: the partial-sum buffers (KsArgs)
// RES / rh / rsel: wave_gemm's resident head (shape-specialised ops whose strided tiles go through in one pass)
template <int R, int ACT = -1, int CS = -1, class TL = NoTail, int LD = -1, bool SPL = false, int KCS = -1, int KS = 0, int RES = 0>
__device__ __forceinline__ void linear_op(const float* W, const float* bias, const LayerMeta lm, const int ld, const bool apply_act,
                                          const int activation, const float slope, const float* in, float* out, const int wave,
                                          const int lane, Prof& prof, const TL* tl = nullptr, const int ldi = 0,
                                          const float* part_in = nullptr, float* part_out = nullptr, const ResHead* rh = nullptr, const int rsel = 0) {
    static_assert(std::is_same<TL, NoTail>::value || CS >= 0, "a fused tail needs a shape-specialised op");
    static_assert(!RES || (CS >= 0 && CS / kWaves <= 3 && KS == 0), "resident heads: one pass of a shape-specialised op");
    static_assert(!KS || CS >= 0, "k-split needs a shape-specialised op");
    const int KC = lm.Kp / kKChunk;
    if constexpr ((KS & 2) != 0) {
        // k-split producer: the CS - 1 strided tiles as usual (CS / 4 per wave, no leftover units), the last tile's k range dealt to the waves
        static_assert(CS % kWaves == 1 && CS / kWaves >= 1 && CS / kWaves <= 3, "k-split: one leftover column tile");
        KsArgs ks;
        ks.part_in = part_in; ks.part_out = part_out; ks.tile = CS - 1; ks.wave = wave;
        ks.k0 = (wave * KC) / kWaves;
        ks.n = ((wave + 1) * KC) / kWaves - ks.k0;
        Extras ex0;
        ex0.c0 = ex0.c1 = ex0.c2 = ex0.c3 = 0; ex0.r0 = ex0.r1 = ex0.r2 = ex0.r3 = 0;
        wave_gemm<R, CS / kWaves, 0, ACT, NoTail, LD, false, KCS, KS>(in, out, ld, W, bias, KC, lm.tail_steps, wave, ex0, apply_act, activation, slope, lane, prof,
                                                                     nullptr, ldi, &ks);
    } else {
    KsArgs ks;  // (KS == 1: a consumer only -- the output layer)
    ks.part_in = part_in; ks.part_out = nullptr; ks.tile = 0; ks.k0 = 0; ks.n = 0; ks.wave = wave;
    // a wave's strided column tiles go through in passes of at most kMaxCT tiles (accumulator + double-buffered
    // fragment registers must fit the 256 VGPRs two waves per SIMD leave each wave)
    constexpr int kMaxCT = kWaves >= 8 ? 2 : 3;
    if constexpr (CS >= 0) {
        constexpr int full = CS / kWaves, rem = CS % kWaves, nu = rem * R;
        Extras ex;
        ex.c0 = kWaves * full + wave / R;                ex.r0 = wave % R;
        ex.c1 = kWaves * full + (wave + kWaves) / R;     ex.r1 = (wave + kWaves) % R;
        ex.c2 = kWaves * full + (wave + 2 * kWaves) / R; ex.r2 = (wave + 2 * kWaves) % R;
        ex.c3 = kWaves * full + (wave + 3 * kWaves) / R; ex.r3 = (wave + 3 * kWaves) % R;
        constexpr int passes = full > kMaxCT ? (full - 1) / kMaxCT : 0;  // whole passes of kMaxCT tiles before the last one
        constexpr int last = full - passes * kMaxCT;                      // 0 .. kMaxCT column tiles ride with the extras
        if constexpr (std::is_same<TL, NoTail>::value) {
#pragma unroll
            for (int p = 0; p < passes; ++p)
                wave_gemm<R, kMaxCT, 0, ACT, TL, LD, SPL, KCS, (KS & 4)>(in, out, ld, W, bias, KC, lm.tail_steps, wave + kWaves * kMaxCT * p, ex, apply_act, activation, slope, lane, prof, tl, ldi);
        } else {  // with a fused tail inlined per unit the body is large: ONE copy, a real loop over the passes
#pragma nounroll
            for (int p = 0; p < passes; ++p)
                wave_gemm<R, kMaxCT, 0, ACT, TL, LD, SPL, KCS, (KS & 4)>(in, out, ld, W, bias, KC, lm.tail_steps, wave + kWaves * kMaxCT * p, ex, apply_act, activation, slope, lane, prof, tl, ldi);
        }
        const int c_first = wave + kWaves * kMaxCT * passes;
        // the nu leftover units are dealt round-robin: waves below nu % kWaves hold one more than the others
        constexpr int lo = nu / kWaves, hi = (nu + kWaves - 1) / kWaves;
        if constexpr (lo == hi) {
            if constexpr (last > 0 || lo > 0)
                wave_gemm<R, last, lo, ACT, TL, LD, SPL, KCS, KS, RES>(in, out, ld, W, bias, KC, lm.tail_steps, c_first, ex, apply_act, activation, slope, lane, prof, tl, ldi, &ks, rh, rsel);
        } else {
            if (wave < nu % kWaves) {
                wave_gemm<R, last, hi, ACT, TL, LD, SPL, KCS, KS, RES>(in, out, ld, W, bias, KC, lm.tail_steps, c_first, ex, apply_act, activation, slope, lane, prof, tl, ldi, &ks, rh, rsel);
            } else {
                if constexpr (last > 0 || lo > 0)
                    wave_gemm<R, last, lo, ACT, TL, LD, SPL, KCS, KS, RES>(in, out, ld, W, bias, KC, lm.tail_steps, c_first, ex, apply_act, activation, slope, lane, prof, tl, ldi, &ks, rh, rsel);
            }
        }
    } else {
        const int C = lm.Np / kTile;
        const int full = C / kWaves, rem = C % kWaves;
        // leftover units u = (column tile kWaves*full + u / R, row tile u % R), dealt round-robin to waves
        const int nu = rem * R;
        Extras ex;
        ex.c0 = kWaves * full + wave / R;                ex.r0 = wave % R;
        ex.c1 = kWaves * full + (wave + kWaves) / R;     ex.r1 = (wave + kWaves) % R;
        ex.c2 = kWaves * full + (wave + 2 * kWaves) / R; ex.r2 = (wave + 2 * kWaves) % R;
        ex.c3 = kWaves * full + (wave + 3 * kWaves) / R; ex.r3 = (wave + 3 * kWaves) % R;
        const int nex = wave < nu ? (nu - wave + kWaves - 1) / kWaves : 0;  // <= kMaxExtras since rem < kWaves, R <= 4
        int done = 0;
        while (full - done > kMaxCT) {
            wave_gemm<R, kMaxCT, 0, ACT, NoTail, -1, SPL>(in, out, ld, W, bias, KC, lm.tail_steps, wave + kWaves * done, ex, apply_act, activation, slope, lane, prof);
            done += kMaxCT;
        }
        const int c_first = wave + kWaves * done;
        switch (full - done) {
            case 0: wave_gemm_ex<R, 0, ACT, SPL>(nex, in, out, ld, W, bias, KC, lm.tail_steps, c_first, ex, apply_act, activation, slope, lane, prof); break;
            case 1: wave_gemm_ex<R, 1, ACT, SPL>(nex, in, out, ld, W, bias, KC, lm.tail_steps, c_first, ex, apply_act, activation, slope, lane, prof); break;
            case 2: wave_gemm_ex<R, 2, ACT, SPL>(nex, in, out, ld, W, bias, KC, lm.tail_steps, c_first, ex, apply_act, activation, slope, lane, prof); break;
            default:
                // (SPL ops have at most 8 column tiles, i.e. at most 2 strided tiles per wave: mlp_layer)
                if constexpr (kMaxCT >= 3 && !SPL)
                    wave_gemm_ex<R, 3, ACT, SPL>(nex, in, out, ld, W, bias, KC, lm.tail_steps, c_first, ex, apply_act, activation, slope, lane, prof);
                break;
        }
    }
    }  // (not a k-split producer)
}

// The head of one shape-specialised op (CS column tiles) as THIS wave's share of it needs it -- linear_op's dealing: strided tiles
// wave + kWaves ct, leftover unit e = (tile kWaves full + (wave + kWaves e) / R, ...) -- requested into AccVGPRs; the caller waits
// (s_waitcnt vmcnt(0)) once for all ops.  A wave with one leftover unit fewer than `hi` requests its unit 0 again for the slot it
// never reads: branch-free, every address a valid one.
template <int R, int CS>
__device__ __forceinline__ void res_load_op(ResHead& h, const float* const W, const float* const bias, const int KC, const int wave, const int lane) {
    constexpr int full = CS / kWaves, rem = CS % kWaves, nu = rem * R;
    constexpr int lo = nu / kWaves, hi = (nu + kWaves - 1) / kWaves;
    static_assert(full <= 3 && hi <= 3, "one pass, at most three leftover units");
#pragma unroll
    for (int ct = 0; ct < full; ++ct) {
        const int c = wave + kWaves * ct;
        res_load(h.b[ct], W + ((size_t)c * KC * 64 + lane) * 4);
        res_load(h.bv[ct], bias + c * 16 + 4 * (lane >> 4));
    }
#pragma unroll
    for (int e = 0; e < hi; ++e) {
        const int u = wave + kWaves * e;  // (units nu and up do not exist: unit 0's tile, a valid one, for the slot nobody reads)
        const int c = kWaves * full + (u < nu ? u : 0) / R;
        res_load(h.bx[e], W + ((size_t)c * KC * 64 + lane) * 4);
        res_load(h.bvx[e], bias + c * 16 + 4 * (lane >> 4));
    }
}
// ... and the same registers re-defined in place (empty asm, "+a"): behind the wait for the loads, and wherever the allocator must not
// be free to move the resident set to other registers (the step loop's back edge)
template <int R, int CS>
__device__ __forceinline__ void res_pin_op(ResHead& h) {
    constexpr int full = CS / kWaves, hi = ((CS % kWaves) * R + kWaves - 1) / kWaves;
#pragma unroll
    for (int ct = 0; ct < full; ++ct) { res_pin(h.b[ct]); res_pin(h.bv[ct]); }
#pragma unroll
    for (int e = 0; e < hi; ++e) { res_pin(h.bx[e]); res_pin(h.bvx[e]); }
}

}  // namespace hipets
