"""The bf16 ensemble kernel's host-side rules, without a device: the name rule, the constant against the header, the geometry rule
restated in hipets.ensemble (csrc/ensemble_bf16.hpp) against hand-computed values, and the numpy bf16 rounding the GPU test's
restatement uses against torch's own cast."""
import os
import re

import numpy as np
import pytest
import torch

from bf16_restatement import bf16_rne_bits
from hipets import _lib
from hipets.ensemble import ENSEMBLE_KERNELS, ensemble_bf16_geometry, ensemble_kernel_for


def test_bf16_is_asked_for_by_name_only():
    assert "bf16" in ENSEMBLE_KERNELS
    for out_dim, det in ((1, False), (18, False), (377, False), (377, True), (512, False)):
        assert ensemble_kernel_for("bf16", out_dim, det) == "bf16"
        assert ensemble_kernel_for("auto", out_dim, det) in ("tile", "wide")
    with pytest.raises(ValueError, match="kernel"):
        ensemble_kernel_for("fp8", 18)


def test_constant_agrees_with_the_header():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "hipets.h")).read()
    defines = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define HIPETS_ENSEMBLE_KERNEL_(\w+) (\d+)", header)}
    assert defines == _lib.ENSEMBLE_KERNEL and defines["bf16"] == 2


@pytest.mark.parametrize("shape,want", [
    ((23, 200, 18), (4, 1, 2, 64 * (64 + 16 + 7 * 64 + 16 + 64))),         # mbpo_halfcheetah: 38 912 B, several workgroups per CU
    ((393, 200, 377), (2, 3, 2, 32 * (13 * 64 + 16 + 7 * 64 + 16 + 64))),  # Humanoid: three mean tiles per wave need R = 2 (44 032 B)
    ((512, 1024, 128), (2, 1, 8, 32 * (16 * 64 + 16 + 32 * 64 + 16 + 64))),  # the widest accepted: 101 376 B
    ((33, 33, 31), (4, 1, 1, 64 * (2 * 64 + 16 + 2 * 64 + 16 + 64))),      # one column in a second k chunk of both kinds
    ((23, 1024, 129), None),                                               # eight hidden tiles beside two mean tiles: refused
    ((23, 257, 18), (2, 1, 3, 32 * (64 + 16 + 9 * 64 + 16 + 64))),         # a third hidden tile per wave: R = 2
])
def test_geometry_rule(shape, want):
    assert ensemble_bf16_geometry(*shape) == want


def test_numpy_rounding_is_torchs_bfloat16_cast():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.uniform(-6, 6, 4096), [0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895314e38]]).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(np.asarray(bf16_rne_bits(x), np.float32).view(np.uint32), want.view(np.uint32))
