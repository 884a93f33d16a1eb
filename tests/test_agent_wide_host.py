"""The host side of kernel= / agent_kernel= (hipets.SACActor, hipets.SACCritic, hipets_set_agent_kernel), without a GPU."""
import os
import re

import pytest

from conftest import ROOT
from hipets import _lib
from hipets import sac as hsac

LDS_LIMIT = 160 * 1024


def test_agent_kernel_for(monkeypatch):
    assert hsac.agent_kernel_for("tile", 1024) == "tile" and hsac.agent_kernel_for("wide", 16) == "wide"
    with pytest.raises(ValueError, match="kernel must be one of"):
        hsac.agent_kernel_for("blocked", 256)
    if hsac.AGENT_WIDE_MIN_HIDDEN is None:  # the wide form won at no measured width: "auto" is the tile form
        assert [hsac.agent_kernel_for("auto", h) for h in (1, 512, 1024)] == ["tile"] * 3
    monkeypatch.setattr(hsac, "AGENT_WIDE_MIN_HIDDEN", 512)
    assert [hsac.agent_kernel_for("auto", h) for h in (511, 512, 1024)] == ["tile", "wide", "wide"]


@pytest.mark.parametrize("k0,hidden,last,wc,tiles,lds", [
    (544, 1024, 64, 64, 8, 157696), (512, 1024, 64, 64, 8, 149504),  # the ABI's limits: critic (one tile asked for is fewer bytes), actor
    (17, 512, 12, 256, 4, 75776), (17, 1024, 12, 256, 8, 75776), (376, 1024, 34, 128, 8, 133120),  # the measured actor shapes
    (23, 256, 1, 256, 2, 75776), (393, 1024, 1, 128, 8, 137216),  # the measured critic shapes
    (3, 20, 2, 64, 1, 40960), (35, 136, 34, 256, 2, 106496)])  # small: the head partials are the larger area
def test_the_lds_rule(k0, hidden, last, wc, tiles, lds):
    assert hsac.agent_wide_geometry(k0, hidden, last) == (wc, tiles, lds) and lds <= LDS_LIMIT


def test_the_switch_is_declared():
    with open(os.path.join(ROOT, "include", "hipets.h")) as fh:
        header = fh.read()
    assert "hipets_set_agent_kernel" in _lib.SYMBOLS and re.search(r"\bint hipets_set_agent_kernel\(hipets_engine\* e, int32_t kind\);", header)
    for name, kind in _lib.AGENT_KERNEL.items():
        assert re.search(rf"#define HIPETS_AGENT_KERNEL_{name.upper()} {kind}\b", header)
