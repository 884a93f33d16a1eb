"""The shape-specialised fused fp32 rollout instances (KSpec::FUSE) at the edges of their shape families, on the GPU: every row of
tests/fused_f32_edges.py at every row-tile count R its family has an instance for (forced with rows_per_group), in both launch modes,
against the fp32 oracle on the draws the engine exports -- every candidate within T2, none masked --, against the generic instance and,
in DEVICE mode, one persistent launch against per-step launches.  tests/test_fused_f32_edges_host.py holds the CPU conditions of every
(row, R, mode): each single-column loss moves a return by >= 4 T2, the oracle's own summation order uses <= T2 / 4, no state is within
1e-4 of a termination threshold.  profiles/fused_f32_edges.json holds the figures measured on MI355X."""
import json

import pytest
import torch

from bf16_restatement import SEED, SID, threshold_margin
from conftest import to_spec
from fused_f32_edges import BY_NAME, CASE_IDS, CASES, NEIGHBOURS, build, neighbour_case, t2
from oracle import device_draws
from oracle import pets_oracle as po
from test_gpu_rollout import assert_same_arithmetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _draws(engine, pop, P, H, mode, R=0):
    """The engine's own draws for (SEED, SID) as oracle arguments; FAST: the member schedule of the geometry a call with
    rows_per_group = R has (0: the default call's), and that geometry's row-tile count"""
    kw = dict(eps=engine.fast_normals(H, pop * P, SEED, SID).cpu())
    r = R
    if mode == "device":
        kw["perms"] = engine.device_perms(H, pop * P, SEED, SID).cpu()
    else:
        nwg, r = engine.fast_geometry(pop, P, H, R)
        sched = engine.fast_schedule(H, nwg, SEED, SID).cpu()
        wg = device_draws.fast_row_workgroup(torch.arange(pop * P), P, r)
        kw["members"] = torch.stack([sched[t][wg].long() for t in range(H)])
    return kw, r


def _oracle(engine, om, actions, s0, pop, P, H, mode, R=0):
    """(oracle returns on the engine's draws, T2 tolerance): finite, and no traced state within 1e-4 of a termination threshold -- the cap
    on candidates left out of a comparison is 0"""
    kw, r = _draws(engine, pop, P, H, mode, R)
    assert R == 0 or r == R
    tr = {}
    ref = po.rollout(om, actions, s0, P, trace=tr, **kw)
    assert torch.isfinite(ref).all()
    assert threshold_margin(om, tr) >= 1e-4, threshold_margin(om, tr)
    return ref, t2(ref)


@pytest.mark.parametrize("row,R,mode", CASES, ids=CASE_IDS)
def test_fused_f32_edge_rows(engine, row, R, mode):
    """1. the call runs the family's instance at R row tiles (("fused", R); W: ("wide", R)) -- an R whose LDS does not hold the row fails here;
    2. |hip_i - ref_i| <= T2_i = 1e-4 max(1, |ref_i|) for EVERY candidate, all values finite (ref: po.rollout on the exported draws);
    3. the same call on the generic instance returns the same bits (one-tile fused instances sum hidden columns 192..207 in another order
       -- KSpec::KSPLIT --: 1e-5, tests/test_gpu_rollout.py assert_same_arithmetic).  W: the general layout holds one row tile of a
       738-column output layer, so the generic twin runs at its own R -- in DEVICE mode, where the permutation and not the geometry
       decides a row's member, that is the same call; the FAST call at R = 2 has no generic twin;
    4. DEVICE mode: one persistent launch equals the per-step launches of `set_persistent(False)` bit for bit.  At R = 3 and depth 4 the
       persistent launch is the resident-heads twin (KSpec::RES: these 200 rows are five workgroups, one per member, all of them
       resident), at every edge of its families -- the one-chunk head of the input layer at tail_steps 1..4 among them -- and the
       per-step launches are the plain instance.  No observable tells the twin from the plain persistent form: both return these
       bits.  Which calls ask for it is a host rule, stated for this table by tests/test_fused_f32_edges_host.py
       test_which_device_calls_ask_for_the_resident_twin (and pinned as compiled by tests/test_resident_heads_rule.py)."""
    c = row.case
    om, actions, s0, _, _ = build(c)
    engine.set_model(to_spec(om, c.obs, c.act))
    cls = engine.kernel_class(c.pop, c.P, c.H, mode, rows_per_group=R)
    assert cls == ("wide" if row.family == "W" else "fused", R)
    kw = dict(mode=mode, seed=SEED, stream_id=SID)
    hip = engine.rollout(actions.to(DEV), s0, c.P, rows_per_group=R, **kw).clone()
    ref, tol = _oracle(engine, om, actions, s0, c.pop, c.P, c.H, mode, R)
    assert torch.isfinite(hip).all()
    err = (hip.cpu() - ref).abs()
    print("F32_EDGE_PARITY " + json.dumps({"case": c.name, "R": R, "mode": mode, "kernel_class": cls[0], "max_err": err.max().item(),
                                           "of_tol": (err / tol).max().item()}))
    bad = err > tol
    assert not bad.any(), f"max |hip - ref| {err.max():.3e} ({(err / tol).max():.2f} x tol) at candidate {int(bad.nonzero()[0])}"
    if row.family != "W":
        gen = engine.rollout(actions.to(DEV), s0, c.P, rows_per_group=R, generic_kernel=True, **kw)
        assert_same_arithmetic(hip, gen, cls)
    elif mode == "device" or R == 1:
        gen = engine.rollout(actions.to(DEV), s0, c.P, rows_per_group=R if mode == "fast" else 0, generic_kernel=True, **kw)
        assert torch.isfinite(gen).all() and torch.equal(hip, gen)
    if mode == "device":
        engine.set_persistent(False)
        try:
            steps = engine.rollout(actions.to(DEV), s0, c.P, rows_per_group=R, **kw)
        finally:
            engine.set_persistent(True)
        assert torch.equal(hip, steps)


# the family member set again after each neighbour: its first row, at the family's first R
_MEMBER = {"A": "A_in18", "I": "I_in3", "W": "W_obs369"}


@pytest.mark.parametrize("nb", NEIGHBOURS, ids=lambda n: n.name)
def test_neighbours_run_no_fused_instance(engine, nb):
    """One step outside a family (tests/fused_f32_edges.py NEIGHBOURS): the default call runs no fused instance (W's neighbour: nor the
    WIDE one), returns the forced generic instance's bits and the oracle's returns within T2; and the family member set right after it
    returns what it returned before -- nothing of the other layout (row stride, head-pair pack, LDS sizes) is left behind."""
    m = BY_NAME[_MEMBER[nb.family]]
    mc, R = m.case, m.Rs[0]
    good, g_actions, g_s0, _, _ = build(mc)
    member_class = ("wide" if m.family == "W" else "fused", R)
    engine.set_model(to_spec(good, mc.obs, mc.act))
    before = {}
    for mode in ("device", "fast"):
        assert engine.kernel_class(mc.pop, mc.P, mc.H, mode, rows_per_group=R) == member_class
        before[mode] = engine.rollout(g_actions.to(DEV), g_s0, mc.P, mode=mode, seed=SEED, stream_id=SID, rows_per_group=R).clone()
    om, actions, s0, _, _ = neighbour_case(nb)
    engine.set_model(to_spec(om, nb.obs, nb.act))
    for mode in ("device", "fast"):
        cls, _ = engine.kernel_class(40, 5, 4, mode)
        assert cls not in ("fused", "wide"), cls
        a = engine.rollout(actions.to(DEV), s0, 5, mode=mode, seed=SEED, stream_id=SID).clone()
        b = engine.rollout(actions.to(DEV), s0, 5, mode=mode, seed=SEED, stream_id=SID, generic_kernel=True)
        assert torch.isfinite(a).all() and torch.equal(a, b)
        ref, tol = _oracle(engine, om, actions, s0, 40, 5, 4, mode)
        err = (a.cpu() - ref).abs()
        print("F32_EDGE_NEIGHBOUR " + json.dumps({"case": nb.name, "mode": mode, "kernel_class": cls, "max_err": err.max().item(), "of_tol": (err / tol).max().item()}))
        assert not (err > tol).any(), f"max |hip - ref| {err.max():.3e} ({(err / tol).max():.2f} x tol)"
    engine.set_model(to_spec(good, mc.obs, mc.act))
    for mode in ("device", "fast"):
        assert engine.kernel_class(mc.pop, mc.P, mc.H, mode, rows_per_group=R) == member_class
        after = engine.rollout(g_actions.to(DEV), g_s0, mc.P, mode=mode, seed=SEED, stream_id=SID, rows_per_group=R)
        assert torch.isfinite(after).all() and torch.equal(after, before[mode])
