"""The host side of product= (hipets.SACUpdater / make_sac_updater / hipets_set_sac_product), without a GPU."""
import os
import re
import warnings

import pytest

import hipets
import sac_restatement as sr
from hipets import _lib
from hipets import sac as hsac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_is_validated_before_anything_else():
    for make in (hipets.SACUpdater, hipets.make_sac_updater):
        with pytest.raises(ValueError, match="product"):
            make(sr.TinySAC(5, 2, 8), product="rows")
    # a known name goes on to the usual checks: the modules are on the CPU here
    with pytest.raises(hipets.UnsupportedModelError, match="on cpu"):
        hipets.SACUpdater(sr.TinySAC(5, 2, 8), product="blocked")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        hipets.make_sac_updater(sr.TinySAC(5, 2, 8), product="auto")
    assert len(w) == 1 and "on cpu" in str(w[0].message)


def test_auto_rule_on_each_side_of_its_threshold(monkeypatch):
    assert hsac.sac_product_for("tile", 1024) == "tile" and hsac.sac_product_for("blocked", 16) == "blocked"
    edge = hsac.SAC_BLOCKED_MIN_HIDDEN
    if edge is None:  # the measured outcome: the blocked route won at no width, "auto" is "tile" everywhere
        assert [hsac.sac_product_for("auto", h) for h in (1, 256, 1024)] == ["tile"] * 3
    else:
        assert hsac.sac_product_for("auto", edge - 1) == "tile" and hsac.sac_product_for("auto", edge) == "blocked"
    monkeypatch.setattr(hsac, "SAC_BLOCKED_MIN_HIDDEN", 512)  # the rule itself, whatever the measurements set
    assert [hsac.sac_product_for("auto", h) for h in (511, 512, 1024)] == ["tile", "blocked", "blocked"]


def test_abi_addition_keeps_the_version():
    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    assert re.search(r"#define HIPETS_ABI_VERSION 9\b", header) and _lib.ABI_VERSION == 9
    assert "hipets_set_sac_product" in _lib.SYMBOLS and re.search(r"\bint hipets_set_sac_product\(hipets_engine\* e, int32_t kind\);", header)
    for name, kind in _lib.SAC_PRODUCT.items():
        assert re.search(rf"#define HIPETS_SAC_PRODUCT_{name.upper()} {kind}\b", header)
    assert _lib.SAC_PRODUCT == {"tile": 0, "blocked": 1}
