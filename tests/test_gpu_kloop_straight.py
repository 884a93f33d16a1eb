"""The straight k loops of the fused fp32 instances with one wave per SIMD (csrc/gemm_f32.hpp "conditional k-steps", kForked): the
k-steps of the last chunk skip themselves inside their asm statement, and the input layer forks once on its chunk count into whole
bodies.  Same operands in the same order, so same bits -- checked here on the shapes tests/fused_f32_edges.py leaves out: input widths
19, 23 .. 47 of family A (obs 17, act 2, 6 .. 30: two and three chunks x 1 .. 4 real k-steps in the last one, i.e. both bodies of the
forked input layer at every tail) crossed with the hidden widths 193, 200, 204, 208 (1 .. 4 real k-steps in the last chunk of every op a
hidden layer feeds), at R = 3 forced, in DEVICE mode -- one persistent launch of five logical workgroups: the resident-heads twin -- and
in FAST mode, bit for bit against the forced generic instance and, DEVICE, against per-step launches (the plain instance)."""
import pytest
import torch

from bf16_restatement import SEED, SID, EdgeCase
from conftest import to_spec
from fused_f32_edges import _MKW, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, R = 17, 3
WIDTHS = (19, 23, 27, 31, 35, 39, 43, 47)
HIDS = (193, 200, 204, 208)


def _case(width, hid, pop=40):
    act = width - OBS
    kw = dict(dict(ensemble_size=5, hid=hid), **_MKW["A"])
    return EdgeCase(f"A_in{width}_hid{hid}", OBS, act, kw, pop, 5, 4, 0, 2.0, 16.0, 8.0)


def test_widths_cover_both_bodies_at_every_tail():
    """(no GPU work) chunks and real k-steps of the last chunk, as csrc/rollout_types.hpp LayerMeta defines them"""
    op0 = {(-(-w // 16), -(-(w - 16 * (-(-w // 16) - 1)) // 4)) for w in WIDTHS}
    assert op0 == {(kc, t) for kc in (2, 3) for t in (1, 2, 3, 4)}
    assert [-(-(h - 192) // 4) for h in HIDS] == [1, 2, 3, 4] and all(-(-h // 16) == 13 for h in HIDS)


def _check(engine, c, mode):
    om, actions, s0, _, _ = build(c)
    engine.set_model(to_spec(om, c.obs, c.act))
    assert engine.kernel_class(c.pop, c.P, c.H, mode, rows_per_group=R) == ("fused", R)
    kw = dict(mode=mode, seed=SEED, stream_id=SID, rows_per_group=R)
    hip = engine.rollout(actions.to(DEV), s0, c.P, **kw).clone()
    assert torch.isfinite(hip).all()
    gen = engine.rollout(actions.to(DEV), s0, c.P, generic_kernel=True, **kw).clone()
    assert torch.equal(hip, gen), f"max |lean - generic| {(hip - gen).abs().max().item():.3e}"
    if mode == "device":
        engine.set_persistent(False)
        try:
            steps = engine.rollout(actions.to(DEV), s0, c.P, **kw)
        finally:
            engine.set_persistent(True)
        assert torch.equal(hip, steps), f"max |persistent - per step| {(hip - steps).abs().max().item():.3e}"


@pytest.mark.parametrize("mode", ("device", "fast"))
@pytest.mark.parametrize("hid", HIDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_straight_k_loops_return_the_generic_bits(engine, width, hid, mode):
    _check(engine, _case(width, hid), mode)


@pytest.mark.parametrize("mode", ("device", "fast"))
def test_five_row_batch(engine, mode):
    """one candidate: five rows, one per member, 43 padding rows in every workgroup (three chunks, three real k-steps; hid 204)"""
    _check(engine, _case(43, 204, pop=1), mode)
