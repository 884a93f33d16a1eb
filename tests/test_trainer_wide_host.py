"""The wide trainer setting on the host, no GPU: Engine.train_steps(kernel="wide") / Engine.train_eval(kernel="wide") against the recording
stand-in library of test_engine_binding_host -- set, call, reset, also when the call raises, nothing extra at the defaults -- and the
Python mirror of HIPETS_TRAIN_WIDE_MAX_HID."""
import os
import re

import pytest
import torch

from hipets import HipetsError, _lib
from test_engine_binding_host import E, HID, OBS, eng, t  # noqa: F401  (eng: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "hipets_set_train_width"


def _arguments(method):
    ws, bs = [t(E, 5, HID), t(E, HID, 2 * OBS)], [t(E, 1, HID), t(E, 1, 2 * OBS)]
    if method == "train_eval":
        return dict(weights=ws, biases=bs, x=t(10, 5), y=t(10, OBS))
    like = lambda ts: [torch.zeros_like(x) for x in ts]  # noqa: E731
    return dict(weights=ws, biases=bs, exp_avg=(like(ws), like(bs)), exp_avg_sq=(like(ws), like(bs)), min_logvar=t(1, OBS), max_logvar=t(1, OBS),
                x=t(10, 5), y=t(10, OBS), idx=t(2, E, 4, dtype=torch.int32), rows=t(2, dtype=torch.int32), step0=0, lr=1e-3)


@pytest.mark.parametrize("method", ["train_steps", "train_eval"])
def test_wide_is_set_called_and_put_back(eng, method):  # noqa: F811
    kw, symbol, run = _arguments(method), "hipets_" + method, getattr(eng, method)
    order = lambda: [(s, r["kind"]) if s.startswith("hipets_set_") else s for s, r in eng._lib.calls]  # noqa: E731
    wide = [(SWITCH, _lib.TRAIN_WIDTH["wide"]), symbol, (SWITCH, _lib.TRAIN_WIDTH["narrow"])]
    run(**kw, kernel="wide")
    assert order() == wide
    eng._lib.calls.clear()
    eng._lib.raises[symbol] = HipetsError("refused", _lib.ERR_INVALID_ARGUMENT)
    with pytest.raises(HipetsError, match="refused"):
        run(**kw, kernel="wide")
    assert order() == wide
    eng._lib.calls.clear()
    del eng._lib.raises[symbol]
    run(**kw)
    assert order() == [symbol]
    with pytest.raises(ValueError):
        run(**kw, kernel="neither")
    assert order() == [symbol]


def test_the_limit_mirrors_the_header():
    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))  # noqa: E731
    assert _lib.TRAIN_WIDE_MAX_HID == macro("HIPETS_TRAIN_WIDE_MAX_HID")
    assert _lib.TRAIN_WIDTH == {"narrow": macro("HIPETS_TRAIN_WIDTH_NARROW"), "wide": macro("HIPETS_TRAIN_WIDTH_WIDE")}
