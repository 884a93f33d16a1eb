"""The operand split of precision='bf16x3' (csrc/gemm_bf16.hpp split3), restated in numpy: three bf16 pieces reproduce an fp32 value to
2^-24 relative, and the six kept partial products reproduce an fp32 product to a few 2^-24."""
import numpy as np


def bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def split3(x):
    x = x.astype(np.float32)
    h0 = bf16_rne(x)
    r1 = (x - h0).astype(np.float32)
    h1 = bf16_rne(r1)
    r2 = (r1 - h1).astype(np.float32)
    h2 = bf16_rne(r2)
    return h0, h1, h2


def test_three_pieces_carry_24_bits_and_six_products_an_fp32_product():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(200000) * np.exp(rng.uniform(-8, 8, 200000))).astype(np.float32)
    b = (rng.standard_normal(200000) * np.exp(rng.uniform(-8, 8, 200000))).astype(np.float32)
    a0, a1, a2 = split3(a)
    b0, b1, b2 = split3(b)
    assert (np.abs(a.astype(np.float64) - (a0.astype(np.float64) + a1 + a2)) <= 2.0 ** -24 * np.abs(a)).all()
    exact = a.astype(np.float64) * b.astype(np.float64)
    six = (a0.astype(np.float64) * b0 + (a0.astype(np.float64) * b1 + a1.astype(np.float64) * b0)
           + (a0.astype(np.float64) * b2 + a1.astype(np.float64) * b1 + a2.astype(np.float64) * b0))
    rel = np.abs(six - exact) / np.abs(exact)
    assert rel.max() <= 2.0 ** -22  # dropped terms a1 b2 + a2 b1 + a2 b2 and the piece residuals
    assert np.median(rel) <= 2.0 ** -25
    # every kept partial product is exact in fp32 (8 x 8 significand bits)
    p = (a1.astype(np.float64) * b1.astype(np.float64))
    assert (p.astype(np.float32).astype(np.float64) == p).all()


def test_dot_product_error_bound_of_the_six_product_scheme():
    """The bound DESIGN.md section 4 states for a K-term dot product in precision='bf16x3': with the three cross terms
    a1 b2, a2 b1, a2 b2 dropped and every operand carried to 2^-24 relative,

        | sum_k six(a_k, b_k)  -  sum_k a_k b_k |  <=  2^-22 sum_k |a_k b_k|          (operand split, exact arithmetic)

    and the fp32 accumulation of the 6 K exact partial products adds what any fp32 accumulation of that many terms adds,
    <= 6 K 2^-24 sum |a_k b_k| in the worst case, ~sqrt(6 K) 2^-24 typically.  Checked on K = 200 (the hidden width) with the
    kernel's accumulation order (per 32-wide chunk: the six piece products, smallest weights first), against fp64, next to
    a plain fp32 chain of the same dot products: the bf16x3 error stays within the bound and within a small multiple of the
    fp32 chain's own error."""
    rng = np.random.default_rng(1)
    n, K = 4000, 200
    a = (rng.standard_normal((n, K)) * np.exp(rng.uniform(-3, 3, (n, K)))).astype(np.float32)
    b = (rng.standard_normal((n, K)) * 0.07).astype(np.float32)  # weights of the reference initialiser's scale
    exact = (a.astype(np.float64) * b.astype(np.float64)).sum(1)
    mag = np.abs(a.astype(np.float64) * b.astype(np.float64)).sum(1)
    a3, b3 = split3(a), split3(b)
    order = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]  # (weight piece, activation piece) as wave_gemm_b3's `unit` issues them
    acc = np.zeros(n, np.float32)
    for k0 in range(0, K, 32):  # one v_mfma_f32_16x16x32_bf16 per piece pair and chunk; inside an MFMA the 32 products add in fp32
        for (pw, pa) in order:
            prod = (b3[pw][:, k0:k0 + 32].astype(np.float32) * a3[pa][:, k0:k0 + 32].astype(np.float32))  # exact in fp32
            acc = (acc + prod.sum(1, dtype=np.float32)).astype(np.float32)
    chain = np.zeros(n, np.float32)
    for k in range(K):
        chain = (chain + a[:, k] * b[:, k]).astype(np.float32)  # fp32 multiply-add chain (products rounded: an upper bound for fmaf)
    err_b3, err_f32 = np.abs(acc - exact), np.abs(chain - exact)
    assert (err_b3 <= (2.0 ** -22 + 6 * K * 2.0 ** -24) * mag).all()          # the worst-case bound
    assert np.median(err_b3 / mag) <= 2.0 ** -22                              # typically: the operand-split term alone
    assert np.percentile(err_b3 / mag, 99) <= 4 * np.percentile(err_f32 / mag, 99) + 2.0 ** -22  # same league as the fp32 chain
