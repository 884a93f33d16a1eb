"""precision='bf16' (include/hipets.h HIPETS_PREC_BF16), the host side: spec validation, the rounding rule, and the power of the
GPU parity tests (tests/test_gpu_bf16.py) to tell bf16 from fp32.

Packing: the weight packer (csrc/rollout_helpers.hpp pack_weights_b3_kernel, pieces = 1) is a device kernel and is not reachable
from a host build; the plane it writes is piece 0 of split3, i.e. bf16_rne_bits of the weight -- the rounding this file restates and
checks against torch.  The packed layout itself is covered on the GPU: a misplaced or mis-rounded weight fails the replay tests."""
import json
import os

import numpy as np
import pytest
import torch

from bf16_restatement import (CASES_OF, CFG2, EDGE_CASES, EDGE_CASES_B3, MUTATIONS, T1_ATOL, T2_REL, bf16_rne_bits, edge_figures, emulated_rollout,
                               scaled_case)
from conftest import ROOT, to_spec
from oracle import pets_oracle as po


def test_spec_accepts_bf16_and_still_refuses_unknown_names():
    from hipets import _lib

    om = po.make_synthetic_model(17, 6, ensemble_size=5, hid=200, seed=0)
    with pytest.raises(ValueError, match="precision"):
        to_spec(om, 17, 6, precision="fp8").validate()
    for name in ("f32", "bf16x3", "bf16"):
        to_spec(om, 17, 6, precision=name).validate()
    assert _lib.PREC["bf16"] == 2 and _lib.PREC["bf16x3"] == 1 and _lib.PREC["f32"] == 0
    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    assert "HIPETS_PREC_BF16 = 2" in header
    assert _lib.KERNEL_CLASSES[4] == "bf16" and "HIPETS_KERNEL_BF16 = 4" in header


def test_rounding_restatement_equals_torch_bfloat16():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(400000) * np.exp(rng.uniform(-30, 30, 400000))).astype(np.float32)
    # exact ties (the 16 dropped bits are 0x8000: to the even neighbour, up and down), in both signs
    hi = rng.integers(0x0080, 0x7F7F, 20000).astype(np.uint32)
    ties = ((hi << 16) | 0x8000).view(np.float32)
    # the largest finite inputs that stay finite: bf16 max itself and everything below its rounding boundary
    top = np.array([0x7F7F0000, 0x7F7F7FFF, 0x7F7F0001, 0x7F7E8000, 0x7F7EFFFF], np.uint32).view(np.float32)
    edge = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)
    for v in (x, ties, -ties, top, -top, edge):
        want = torch.from_numpy(v.copy()).to(torch.bfloat16).float().numpy()
        got = bf16_rne_bits(v)
        assert np.isfinite(want).all()
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (bf16_rne_bits(ties).view(np.uint32) & 0x10000 == 0).all()  # ties land on the even bf16


@pytest.mark.parametrize("H,bound", [(1, T1_ATOL), (30, T2_REL)], ids=["H1_T1", "H30_T2"])
def test_scaled_case_tells_bf16_from_fp32(monkeypatch, H, bound):
    """The power check: on the scaled cfg2 case (pop 500 x 20) the emulated bf16 rollout differs from the fp32 oracle by at least
    ten times the fp32 mode's own tolerance (T1 atol at H = 1; T2, relative to max(1, |v|), at H = 30) -- so an fp32 kernel in
    disguise cannot pass the GPU tests' 'really bf16' check, and D there is far above fp32 noise."""
    obs, act, pop, P, mkw = CFG2
    om, actions, s0, perms, eps = scaled_case(obs, act, pop, P, H, **mkw)
    f32 = po.rollout(om, actions, s0, P, perms=perms, eps=eps)
    emu = emulated_rollout(monkeypatch, om, actions, s0, P, perms=perms, eps=eps)
    assert torch.isfinite(emu).all() and torch.isfinite(f32).all()
    d = (emu - f32).abs()
    fig = d.max().item() if H == 1 else (d / torch.clamp(f32.abs(), min=1.0)).max().item()
    print(f"H {H}: max|emu - f32| = {d.max().item():.3e}, figure {fig:.3e}, {fig / bound:.0f} x the bound {bound:g}")
    assert fig >= 10 * bound, fig
    # the restatement is no longer installed: the oracle is the fp32 one again
    assert torch.equal(po.rollout(om, actions, s0, P, perms=perms, eps=eps), f32)


# ---------------------------------------------------------------------------------------------------------------------
# The edge probes of the two instance families (tests/bf16_restatement.py EDGE_CASES): what the GPU tests of every case can see,
# measured on the CPU before a GPU is touched
# ---------------------------------------------------------------------------------------------------------------------
_EDGE = [(prec, c) for prec in ("bf16", "bf16x3") for c in CASES_OF[prec]]


@pytest.mark.parametrize("mode", ["device", "fast"])
@pytest.mark.parametrize("prec,case", _EDGE, ids=[f"{p}-{c.name}" for p, c in _EDGE])
def test_edge_case_cpu_conditions(monkeypatch, prec, case, mode):
    """Against the reference of `prec` (bf16: the emulation, tol_i = max(T2_i, D / 4); bf16x3: the fp32 oracle, T2), on the CPU
    restatement of the draws the GPU test replays:
    (a) power: zeroing the last input row of layer 0, the last hidden row of layer 1 (where a hidden -> hidden layer exists), the last
        mean column or the last log-variance column moves some candidate's reference return by >= 4 x its tolerance (the device may
        itself use up to 1 x);
    (b) spread: the same restatement accumulated in f64 stays within tol / 4 of the reference for every candidate -- the kernel's own
        fp32 summation order, which neither restates, has four times the room the reference's needs;
    (c) the reference returns are finite, and no row's height is within 1e-4 of the humanoid thresholds 1.0 / 2.0;
    (d) bf16: some candidate's |emu - f32| is >= 4 x its T2 tolerance: the mode is told apart from fp32;
    (e) bf16, flip room: with every activation moved by -2, -1, 1 or 2 fp32 ulps before its rounding to bf16 the emulation stays within
        tol / 2 of itself for every candidate.  The device's elementwise functions are not torch's (its SiLU, x rcp(1 + exp2(-x log2 e)),
        is off by 0.3 ulp on average and <= 2.6 on [-3, 10]), so some activations land on the other side of a bf16 boundary there: a
        case in which one such flip is worth a tolerance tests the draw of the flips, not the kernel.  (b) and (e) together leave the
        device a quarter of the tolerance."""
    f = edge_figures(monkeypatch, case, prec, mode)
    print("EDGE_CPU " + json.dumps({"case": case.name, "precision": prec, "mode": mode, **f}))
    assert f["finite"]
    want = [m for m in MUTATIONS if m != "hid_row" or case.mkw.get("num_layers", 4) > 1]
    assert sorted(f["power"]) == sorted(want)
    assert min(f["power"].values()) >= 4.0, f["power"]
    assert f["spread"] <= 0.25, f["spread"]
    assert f["margin"] >= 1e-4, f["margin"]
    if prec == "bf16":
        assert f["told"] >= 4.0, f["told"]
        assert sorted(f["flip"]) == [-2, -1, 1, 2] and max(f["flip"].values()) <= 0.5, f["flip"]


def test_edge_case_table_covers_the_family_edges():
    """Every edge the table claims, stated on the shapes: input widths on both sides of the 32-wide k chunks up to the first ring
    refill (kBf16Ahead = 4 chunks), full and nearly empty last output tiles, both hidden-width limits, both depths, a non-prefix
    member subset and single-tile batches; bf16x3 runs the same table up to the widest input its three-plane rows leave LDS for."""
    ins = {c.name: c.obs + c.act for c in EDGE_CASES}
    assert [ins[n] for n in ("A_in18", "A_in32", "A_in33", "A_in64", "A_in65", "A_in97", "A_in129")] == [18, 32, 33, 64, 65, 97, 129]
    assert [ins[n] for n in ("B_in42", "B_in64", "B_in65", "B_in97")] == [42, 64, 65, 97]
    assert {-(-i // 32) for i in ins.values()} >= {1, 2, 3, 4, 5}
    for cases in (EDGE_CASES, EDGE_CASES_B3):
        fam_a = [c for c in cases if c.mkw.get("termination") is None]
        fam_b = [c for c in cases if c.mkw.get("termination") == "humanoid"]
        assert {c.obs for c in fam_a} >= {17, 24} and all(17 <= c.obs <= 24 for c in fam_a)
        assert {c.obs for c in fam_b} >= {41, 48} and all(41 <= c.obs <= 48 for c in fam_b)
        assert {c.mkw["hid"] for c in cases} == {193, 200, 208}
        assert {c.mkw.get("num_layers", 4) for c in cases} == {1, 4, 7}
        assert any(c.mkw.get("elite") == [0, 2, 3, 5, 6] for c in cases) and {c.pop for c in cases} == {1, 7, 40}
        assert all((c.P, c.H) == (5, 4) for c in cases)
    assert [c.name for c in EDGE_CASES_B3 if c not in EDGE_CASES] == ["A_in88", "B_in96"] and len(EDGE_CASES_B3) == len(EDGE_CASES) - 1
