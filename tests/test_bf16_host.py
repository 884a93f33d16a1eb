"""precision='bf16' (include/hipets.h HIPETS_PREC_BF16), the host side: spec validation, the rounding rule, and the power of the
GPU parity tests (tests/test_gpu_bf16.py) to tell bf16 from fp32.

Packing: the weight packer (csrc/rollout_helpers.hpp pack_weights_b3_kernel, pieces = 1) is a device kernel and is not reachable
from a host build; the plane it writes is piece 0 of split3, i.e. bf16_rne_bits of the weight -- the rounding this file restates and
checks against torch.  The packed layout itself is covered on the GPU: a misplaced or mis-rounded weight fails the replay tests."""
import os

import numpy as np
import pytest
import torch

from bf16_restatement import CFG2, T1_ATOL, T2_REL, bf16_rne_bits, emulated_rollout, scaled_case
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
