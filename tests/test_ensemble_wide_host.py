"""The wide ensemble kernel's host-side rules, without a device: the geometry rule restated in hipets.ensemble (csrc/ensemble_wide.hpp)
against hand-computed values, and kernel="auto" as a function of the model's shape alone."""
import pytest

from hipets.ensemble import ENSEMBLE_WIDE_MIN_OUT_COLS, ensemble_kernel_for, ensemble_wide_geometry


@pytest.mark.parametrize("shape,want", [
    ((23, 200, 18), (4, 1, 2, 64 * 4 * (32 + 4 + 208 + 4 + 16))),       # stock: 67 584 B
    ((393, 200, 377), (4, 3, 2, 161792)),                               # Humanoid: X 103 424 + H 54 272 + partials 4 096
    ((448, 200, 441), (2, 4, 2, 32 * 4 * (448 + 4 + 208 + 4 + 16))),    # 64 rows of the input do not fit (174 080 B); four mean tiles need R = 2 too
    ((512, 200, 377), (2, 3, 2, 95232)),                                # the in_dim limit
    ((23, 200, 400), (2, 4, 2, 33792)),                                 # LDS would allow R = 4, the registers of four mean tiles do not
    ((23, 1024, 18), (2, 1, 8, 32 * 4 * (32 + 4 + 1024 + 4 + 16))),     # eight hidden tiles per wave: R = 2
    ((248, 1024, 9), None),                                             # 32 rows x (260 + 1028 + 16) floats = 166 912 B: the tile form
    ((23, 1024, 300), None),                                            # eight hidden tiles beside three mean tiles: the tile form
])
def test_geometry_rule(shape, want):
    assert ensemble_wide_geometry(*shape) == want
    assert ensemble_wide_geometry(*shape, deterministic=True) == want  # (the output layer is not in LDS: its width does not enter)


def test_auto_reads_the_shape_alone():
    for out_dim, det in ((18, False), (377, False), (377, True), (512, False)):
        cols = -(-(out_dim if det else 2 * out_dim) // 16) * 16
        want = "wide" if ENSEMBLE_WIDE_MIN_OUT_COLS is not None and cols >= ENSEMBLE_WIDE_MIN_OUT_COLS else "tile"
        assert ensemble_kernel_for("auto", out_dim, det) == want
        assert ensemble_kernel_for("tile", out_dim, det) == "tile" and ensemble_kernel_for("wide", out_dim, det) == "wide"
    with pytest.raises(ValueError, match="kernel"):
        ensemble_kernel_for("broad", 18)
