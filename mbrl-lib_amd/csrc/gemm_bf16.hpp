// gemm_bf16.hpp -- the bf16x3 / bf16 GEMM of a workgroup's row tiles on the bf16 matrix pipe: the split of an fp32 value into bf16
// pieces (host and device: the weight packer states the same arithmetic), the LDS row format of the pieces, one wave's share of a
// linear op (wave_gemm_b3) and the op itself (linear_op_b3).  Replaces the same reference code as gemm_f32.hpp --
// EnsembleLinearLayer.forward (mbrl/models/util.py:53-65) and the SiLU behind it (gaussian_mlp.py:89-112) -- in another arithmetic.
#pragma once
#include "common.hpp"
#include "gemm_f32.hpp"
#include "rollout_types.hpp"

namespace hipets {

// ---------------------------------------------------------------------------------------------------------------------
// bf16x3 precision mode ("f32 on the bf16 matrix pipe").  An fp32 operand x is carried as three bf16 pieces x0 + x1 + x2
// (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1): |x - x0 - x1 - x2| <= 2^-24 |x|), and a product a b is formed from
// the six partial products of weight <= 2^-16: a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0), each EXACT in fp32
// (8 x 8 significand bits), accumulated in fp32 by v_mfma_f32_16x16x32_bf16.  The dropped terms (a1 b2, a2 b1, a2 b2) are
// <= 2^-23 |a b|: the result is fp32-accurate to a few ulps of the products, at 6 x 17 cycles per 16x16x32 block instead of
// 8 x 32 cycles for the fp32 MFMAs -- and the bf16 matrix pipe, unlike the fp32 one, runs beside the VALU.
// Layouts: weights packed per (column tile, 32-wide k chunk, piece) as one A-operand fragment (lane l: output column
// l & 15, k = 8 (l >> 4) .. + 7); activations in LDS per row as [k chunk][piece][4 groups][8 x bf16] so that a lane's
// B-operand fragment of a piece is ONE ds_read_b128.  The last layer's results stay fp32 (sampling reads them).
// Precision bf16 (HIPETS_PREC_BF16) is the one-piece form of the same code (template parameter NP = 1): piece 0 alone, i.e. both
// operands rounded to bf16 (nearest-even), exact products, fp32 accumulation, ONE MFMA per block; bias and SiLU in fp32.
// ---------------------------------------------------------------------------------------------------------------------
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// round-to-nearest-even bf16 of x as the upper 16 bits of a word (finite x)
__host__ __device__ __forceinline__ unsigned bf16_rne_bits(float x) {
    unsigned u;
    __builtin_memcpy(&u, &x, 4);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
}
__host__ __device__ __forceinline__ float bits_to_float(unsigned u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// the three pieces of x as bf16 bit patterns (in the UPPER halves of h[0..2])
__host__ __device__ __forceinline__ void split3(float x, unsigned (&h)[3]) {
    h[0] = bf16_rne_bits(x);
    const float r1 = x - bits_to_float(h[0]);
    h[1] = bf16_rne_bits(r1);
    const float r2 = r1 - bits_to_float(h[1]);
    h[2] = bf16_rne_bits(r2);
}
// four consecutive values -> per piece one 8-byte word pair (4 x bf16, little endian: value 0 in the low half of word 0).
// v_cvt_pk_bf16_f32 rounds two floats to nearest-even and packs them in exactly that order: one conversion, two bit
// operations and one packed subtract per pair and piece (the host-side split3 above states the same arithmetic bit by bit).
// NP = 1 keeps piece 0 alone: the plain bf16 rounding of precision bf16 (HIPETS_PREC_BF16).
template <int NP>
__device__ __forceinline__ void split_x4(const f32x4 v, u32x2 (&out)[NP]) {
    using f32p = __attribute__((ext_vector_type(2))) float;
    using bf16p = __attribute__((ext_vector_type(2))) __bf16;
    f32p lo = {v[0], v[1]}, hi = {v[2], v[3]};
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const bf16p hl = __builtin_convertvector(lo, bf16p), hh = __builtin_convertvector(hi, bf16p);
        unsigned ul, uh;
        __builtin_memcpy(&ul, &hl, 4);
        __builtin_memcpy(&uh, &hh, 4);
        out[p][0] = ul;
        out[p][1] = uh;
        if (p + 1 < NP) {
            lo = lo - f32p{bits_to_float(ul << 16), bits_to_float(ul & 0xFFFF0000u)};
            hi = hi - f32p{bits_to_float(uh << 16), bits_to_float(uh & 0xFFFF0000u)};
        }
    }
}
__device__ __forceinline__ bf16x8 as_bf16x8(const u32x4 v) {
    bf16x8 r;
    __builtin_memcpy(&r, &v, 16);
    return r;
}
// byte offset inside an activation row of the 4 consecutive columns k0 .. k0 + 3 (k0 % 4 == 0) of piece p of NP
template <int NP>
__device__ __forceinline__ int b3_offset(int k0, int p) { return (k0 >> 5) * (64 * NP) + p * 64 + ((k0 & 31) >> 3) * 16 + (k0 & 7) * 2; }

template <int R, int CT, int EX, int NP>
struct GemmFragsB3 {
    u32x4 w[CT > 0 ? CT : 1][NP];   // weight pieces (A operand) of the strided column tiles
    u32x4 wx[EX > 0 ? EX : 1][NP];  // ... of the extra units
    u32x4 a[R][NP];                 // activation pieces (B operand) of the row tiles
    u32x4 ax[EX > 0 ? EX : 1][NP];
};

// One wave's share of a linear op in bf16x3 arithmetic: same unit decomposition as wave_gemm (CT strided column tiles x R row
// tiles + EX extra units).  `in`: LDS activation pieces (byte stride ldb); hidden ops write the activated result as pieces into
// `out`, the last op writes fp32 (float stride ldb / 4) for the sampling phase.
// NP = 3: precision bf16x3.  NP = 1: precision bf16 -- one weight and one activation fragment per unit, ONE MFMA per unit and k
// chunk, activation rows of 64 bytes per chunk; the bf16 store of a hidden layer's activated result IS the rounding of the next
// layer's operand.  Its k loop is paced by the fragment loads, not by the MFMAs: fragments are requested kBf16Ahead chunks ahead
// (measured per cfg2 rollout, DEVICE / FAST: 2 ahead 0.443 / 0.362 ms, 4 ahead 0.437 / 0.356 ms, all 7 chunks of a hidden layer
// 0.450 / 0.375 ms -- profiles/bf16_rollout.json).
constexpr int kBf16Ahead = 4;
template <int R, int CT, int EX, int ACT, int NP>
__device__ __forceinline__ void wave_gemm_b3(const char* __restrict__ in, char* __restrict__ out, const int ldb, const uint4* __restrict__ W3,
                                             const float* __restrict__ bias, const int KC32, const int c_first, const Extras ex,
                                             const bool last_op, const int lane) {
    constexpr int CTn = CT > 0 ? CT : 1;
    constexpr int EXn = EX > 0 ? EX : 1;
    f32x4 acc[CTn][R];
    f32x4 accx[EXn];
    const int exc[kMaxExtras] = {ex.c0, ex.c1, ex.c2, ex.c3};
    const int exr[kMaxExtras] = {ex.r0, ex.r1, ex.r2, ex.r3};
    // weights: 16-byte units; (column tile c, chunk kk, piece p, lane) -> ((c * KC32 + kk) * NP + p) * 64 + lane
    constexpr int kCh = 64 * NP;  // 16-byte weight units per (column tile, chunk) -- and bytes per chunk of an activation row
    unsigned woff[CTn], wxoff[EXn];
    int axoff[EXn];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) woff[ct] = (unsigned)((c_first + kWaves * ct) * KC32 * kCh + lane);
#pragma unroll
    for (int e = 0; e < EX; ++e) {
        wxoff[e] = (unsigned)(exc[e] * KC32 * kCh + lane);
        axoff[e] = exr[e] * 16 * ldb;
    }
    const char* ap = in + (lane & 15) * ldb + (lane >> 4) * 16;
    // biases: the packed bias arrays serve the fp32 kernels, where hidden layers keep their columns permuted inside every group
    // of 16 (position lds_col(n) holds column n; lds_col is an involution); here columns are natural
    auto bias4 = [&](const int c) __attribute__((always_inline)) {
        const int g = lane >> 4;
        if (last_op) return *reinterpret_cast<const f32x4*>(bias + c * 16 + 4 * g);
        const float* bp = bias + c * 16 + g;  // natural column 4 g + i sits at position 4 i + g
        return f32x4{bp[0], bp[4], bp[8], bp[12]};
    };
#pragma unroll
    for (int ct = 0; ct < CTn; ++ct) {
        const f32x4 b = CT > 0 ? bias4(c_first + kWaves * ct) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < R; ++r) acc[ct][r] = b;
    }
#pragma unroll
    for (int e = 0; e < EXn; ++e) accx[e] = EX > 0 ? bias4(exc[e]) : f32x4{0.f, 0.f, 0.f, 0.f};

    auto load = [&](GemmFragsB3<R, CT, EX, NP>& f, const int kk) __attribute__((always_inline)) {
        const uint4* Wk = W3 + (size_t)kk * kCh;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int p = 0; p < NP; ++p) f.w[ct][p] = *reinterpret_cast<const u32x4*>(Wk + woff[ct] + p * 64);
#pragma unroll
        for (int e = 0; e < EX; ++e)
#pragma unroll
            for (int p = 0; p < NP; ++p) f.wx[e][p] = *reinterpret_cast<const u32x4*>(Wk + wxoff[e] + p * 64);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int p = 0; p < NP; ++p) f.a[r][p] = *reinterpret_cast<const u32x4*>(ap + r * 16 * ldb + kk * kCh + p * 64);
#pragma unroll
        for (int e = 0; e < EX; ++e)
#pragma unroll
            for (int p = 0; p < NP; ++p) f.ax[e][p] = *reinterpret_cast<const u32x4*>(ap + axoff[e] + kk * kCh + p * 64);
    };
    // the six partial products of one unit, smallest weights first (NP = 1: the one product)
    auto unit = [&](const u32x4 (&w)[NP], const u32x4 (&a)[NP], f32x4& c) __attribute__((always_inline)) {
        if constexpr (NP == 3) {
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w[2]), as_bf16x8(a[0]), c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w[1]), as_bf16x8(a[1]), c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w[0]), as_bf16x8(a[2]), c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w[1]), as_bf16x8(a[0]), c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w[0]), as_bf16x8(a[1]), c, 0, 0, 0);
        }
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w[0]), as_bf16x8(a[0]), c, 0, 0, 0);
    };
    auto compute = [&](const GemmFragsB3<R, CT, EX, NP>& f) __attribute__((always_inline)) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < R; ++r) unit(f.w[ct], f.a[r], acc[ct][r]);
#pragma unroll
        for (int e = 0; e < EX; ++e) unit(f.wx[e], f.ax[e], accx[e]);
    };
    if constexpr (NP == 1) {
        // a ring of kBf16Ahead fragment sets (32 registers each at R = 3): slot i holds chunks i, i + kBf16Ahead, ...; a slot is
        // refilled as soon as its MFMAs are issued, so kBf16Ahead - 1 chunks of loads are in flight behind every compute
        GemmFragsB3<R, CT, EX, NP> f[kBf16Ahead];
#pragma unroll
        for (int i = 0; i < kBf16Ahead; ++i)
            if (i < KC32) load(f[i], i);
        for (int kk = 0; kk < KC32; kk += kBf16Ahead) {
#pragma unroll
            for (int i = 0; i < kBf16Ahead; ++i) {
                if (kk + i < KC32) {
                    __builtin_amdgcn_sched_barrier(0);
                    compute(f[i]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (kk + i + kBf16Ahead < KC32) load(f[i], kk + i + kBf16Ahead);
                }
            }
        }
    } else {
        GemmFragsB3<R, CT, EX, NP> f0, f1;
        load(f0, 0);
        int kk = 0;
        for (; kk + 1 < KC32; kk += 2) {
            load(f1, kk + 1);
            __builtin_amdgcn_sched_barrier(0);
            compute(f0);
            __builtin_amdgcn_sched_barrier(0);
            if (kk + 2 < KC32) load(f0, kk + 2);
            __builtin_amdgcn_sched_barrier(0);
            compute(f1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (kk < KC32) compute(f0);
    }

    const int j = lane & 15, g4 = 4 * (lane >> 4);
    static_assert(ACT == HIPETS_ACT_SILU, "bf16x3 / bf16 instances exist for SiLU models");
    auto store = [&](const f32x4 v, const int row, const int col0) __attribute__((always_inline)) {
        if (last_op) {
            *reinterpret_cast<f32x4*>(out + (size_t)row * ldb + col0 * 4) = v;  // fp32, natural columns (float stride ldb / 4)
        } else {
            u32x2 pc[NP];
            split_x4<NP>(silu4(v), pc);
#pragma unroll
            for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x2*>(out + (size_t)row * ldb + b3_offset<NP>(col0, p)) = pc[p];
        }
    };
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < R; ++r) store(acc[ct][r], r * 16 + j, (c_first + kWaves * ct) * 16 + g4);
#pragma unroll
    for (int e = 0; e < EX; ++e) store(accx[e], exr[e] * 16 + j, exc[e] * 16 + g4);
}

// linear op with CS column tiles in bf16x3 (NP = 3) or bf16 (NP = 1) arithmetic (static shapes only: the lean instances)
template <int R, int ACT, int CS, int NP>
__device__ __forceinline__ void linear_op_b3(const uint4* W3, const float* bias, const int KC32, const int ldb, const bool last_op, const char* in,
                                             char* out, const int wave, const int lane) {
    constexpr int kMaxCT = 3;
    constexpr int full = CS / kWaves, rem = CS % kWaves, nu = rem * R;
    static_assert(full <= kMaxCT, "bf16x3 / bf16 instances cover ops of at most 15 column tiles");
    Extras ex;
    ex.c0 = kWaves * full + wave / R;                ex.r0 = wave % R;
    ex.c1 = kWaves * full + (wave + kWaves) / R;     ex.r1 = (wave + kWaves) % R;
    ex.c2 = kWaves * full + (wave + 2 * kWaves) / R; ex.r2 = (wave + 2 * kWaves) % R;
    ex.c3 = kWaves * full + (wave + 3 * kWaves) / R; ex.r3 = (wave + 3 * kWaves) % R;
    constexpr int lo = nu / kWaves, hi = (nu + kWaves - 1) / kWaves;
    if constexpr (lo == hi) {
        if constexpr (full > 0 || lo > 0) wave_gemm_b3<R, full, lo, ACT, NP>(in, out, ldb, W3, bias, KC32, wave, ex, last_op, lane);
    } else {
        if (wave < nu % kWaves) {
            wave_gemm_b3<R, full, hi, ACT, NP>(in, out, ldb, W3, bias, KC32, wave, ex, last_op, lane);
        } else {
            if constexpr (full > 0 || lo > 0) wave_gemm_b3<R, full, lo, ACT, NP>(in, out, ldb, W3, bias, KC32, wave, ex, last_op, lane);
        }
    }
}

}  // namespace hipets
