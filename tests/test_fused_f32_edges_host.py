"""The edge table of the fused fp32 rollout instances (tests/fused_f32_edges.py), the host side: that every row lies inside its shape
family and every neighbour outside, stated on a restatement of the shape arithmetic of csrc/model.hip and the family conditions of
csrc/launch.hpp; that the table covers the edges it claims; which DEVICE calls ask for the resident-heads twin; and, per (row, R, mode),
what the GPU comparison of tests/test_gpu_fused_f32_edges.py can see -- measured on the CPU before a GPU is touched."""
import json
import os
import re

import pytest
import torch

from bf16_restatement import cpu_draws, threshold_margin
from conftest import ROOT
from fused_f32_edges import BY_NAME, CASE_IDS, CASES, FAMILIES, NEIGHBOURS, ROWS, build, f32_figures, mutations_of, neighbour_case
from oracle import pets_oracle as po

LDS_MAX = 160 * 1024  # csrc/engine.hip: what a workgroup may opt in to
N_CU = 256


# ---------------------------------------------------------------------------------------------------------------------
# csrc/model.hip hipets_set_model, restated: the padded shapes of the ops and the LDS row stride
# ---------------------------------------------------------------------------------------------------------------------
def up16(x):
    return (x + 15) // 16 * 16


def shape_of(obs, act, mkw):
    hid, learned = mkw.get("hid", 200), bool(mkw.get("learned_rewards"))
    obs_process, reward, term = mkw.get("obs_process", "none"), mkw.get("reward", "halfcheetah"), mkw.get("termination", "no_termination")
    n_layers = mkw.get("num_layers", 4) + 1
    in_dim = obs + (1 if obs_process == "cartpole_pets" else 0) + act
    out_dim = obs + (1 if learned else 0)
    Ks = [in_dim] + [hid] * (n_layers - 1)
    Ns = [hid] * (n_layers - 1) + [2 * out_dim]
    ops = [dict(K=k, Kp=up16(k), Np=up16(n), KC=up16(k) // 16, tail_steps=(k - (up16(k) - 16) + 3) // 4) for k, n in zip(Ks, Ns)]
    ld = max(max(o["Kp"], o["Np"]) for o in ops)
    while ld % 64 != 8:
        ld += 4
    return dict(obs=obs, act=act, in_dim=in_dim, out_dim=out_dim, n_layers=n_layers, ops=ops, hidC=up16(hid) // 16, outC=up16(2 * out_dim) // 16, ld=ld,
                reward="LEARNED" if reward is None else reward.upper(), term="NONE" if term == "no_termination" else term.upper(),
                obs_process=obs_process.upper())


def lean_ld(hidc, outc):  # csrc/kspec.hpp
    m = max(hidc, outc) * 16
    while m % 64 != 8:
        m += 4
    return m


def fused_term_ok(s):  # csrc/launch.hpp
    if s["term"] == "INVERTED_PENDULUM" and s["obs"] > 4:
        return False
    if s["term"] == "HOPPER":
        return s["reward"] == "LEARNED"
    return not (s["reward"] == "LEARNED" and s["term"] != "NONE" and s["obs"] >= 8)


def in_family(s, fam):
    """csrc/launch.hpp lean_shape_is + fused_term_ok (the synthetic models are SiLU, f64-normalised, stochastic and not BasicEnsembles:
    the rest of spec_model holds for every row and neighbour)"""
    hc, oc, rw, tm, ob = fam.shape
    return (s["hidC"], s["outC"], s["reward"], s["term"], s["obs_process"], s["ld"]) == (hc, oc, rw, tm, ob, lean_ld(hc, oc)) and fused_term_ok(s)


def families_of(s):
    return [name for name, fam in FAMILIES.items() if in_family(s, fam)]


def smem_bytes(rows, s):
    """csrc/rollout_smem.hpp rollout_smem_bytes of the general layout (no expectation propagation, H = 4), section by section"""
    a16 = lambda x: (x + 15) // 16 * 16
    n = 2 * a16(rows * s["ld"] * 4) + 4 * a16(rows * 4) + a16(2 * rows * 4) + a16(56 * 8) + a16(4 * 16 * 8) + 16   # buf0 .. dump (LayerMeta: 56 bytes x 8)
    n += 2 * 4 * 64 * 16 if rows == 16 else 0                                                                     # part
    n += a16(rows * s["obs"] * 4) + a16(2 * rows * s["act"] * 4) + 2 * a16(s["in_dim"] * 8)                     # state, actn, nmean, nstd
    return n + 2 * a16(s["out_dim"] * 4) + a16(s["obs"] * 4) + a16(4 * 4)                                       # minlv, maxlv, nodelta, sched


def test_family_table_is_the_headers():
    """FAMILIES against the text of csrc/launch.hpp: every HIPETS_LEAN_SHAPES_R<R> entry is a family that lists R, and nothing else is"""
    text = open(os.path.join(ROOT, "mbrl-lib_amd", "csrc", "launch.hpp")).read()
    listed = {}
    for R in (1, 2, 3, 4):
        body = re.search(r"#define HIPETS_LEAN_SHAPES_R%d\(X\)((?:.*\\\n)*.*)\n" % R, text).group(1)
        for hc, oc, rw, tm, ob in re.findall(r"X\((\d+), (\d+), HIPETS_REW_(\w+), HIPETS_TERM_(\w+), HIPETS_OBS_(\w+)\)", body):
            listed.setdefault((int(hc), int(oc), rw, tm, ob), []).append(R)
    assert listed == {fam.shape: list(fam.Rs) for fam in FAMILIES.values()}
    assert "constexpr int kSplMaxTiles = 8;" in open(os.path.join(ROOT, "mbrl-lib_amd", "csrc", "kspec.hpp")).read()  # W: 47 > 8 tiles is KSpec::WIDE


def test_every_row_is_inside_its_family_and_every_neighbour_outside():
    for r in ROWS:
        s = shape_of(r.case.obs, r.case.act, r.case.mkw)
        assert families_of(s) == [r.family], (r.case.name, s)
        assert FAMILIES[r.family].obs_lo <= r.case.obs <= FAMILIES[r.family].obs_hi
        assert (r.case.pop, r.case.P, r.case.H) in ((40, 5, 4), (1, 5, 4)) and len(r.case.mkw.get("elite") or range(r.case.mkw["ensemble_size"])) == 5
    for nb in NEIGHBOURS:
        assert families_of(shape_of(nb.obs, nb.act, nb.mkw)) == [], nb.name
    # each neighbour is ONE step outside: the same model with the stepped quantity put back is inside
    back = {"A_obs16": dict(obs=17), "A_obs25": dict(obs=24), "A_hid192": dict(hid=193), "A_hid209": dict(hid=208), "A_in257": dict(act=232),
            "I_obs5": dict(obs=4), "W_obs368": dict(obs=369)}
    for nb in NEIGHBOURS:
        if nb.name in back:
            fix = dict(back[nb.name])
            obs, act = fix.pop("obs", nb.obs), fix.pop("act", nb.act)
            assert families_of(shape_of(obs, act, dict(nb.mkw, **fix))) == [nb.family], nb.name
    # LT_obs8 has no family to step back into (no termination function but inverted_pendulum and hopper is fused next to a learned reward);
    # what keeps it out is fused_term_ok's obs_dim >= 8 clause, whatever table a later round adds
    lt = shape_of(8, 1, BY_NAME["I_in5"].case.mkw | dict(termination="cartpole"))
    assert not fused_term_ok(lt) and fused_term_ok(dict(lt, obs=7))


def test_the_input_width_limit_is_the_row_stride():
    """in <= 256 is nowhere written: 257 input columns pad to Kp 272, the widest activation, and the row stride (>= it, 8 mod 64) goes
    from the 264 floats the instances were compiled for to 328"""
    a = BY_NAME["A_in256"].case
    assert shape_of(a.obs, a.act, a.mkw)["ld"] == 264 == lean_ld(13, 3) and shape_of(a.obs, a.act + 1, a.mkw)["ld"] == 328
    assert shape_of(a.obs, a.act, a.mkw)["ops"][0]["KC"] == 16


def test_rows_run_at_every_row_tile_count_of_their_family_that_fits_the_lds():
    """... which is every R for all rows but two: A_in256 (232 action columns, double buffered) does not fit three row tiles, B_in97 (56
    action columns next to 4 x 16 rows of activations) not four.  A forced R that does not fit is an error, not another instance."""
    dropped = {}
    for r in ROWS:
        if r.family == "W":  # (the WIDE layout has its own, smaller, sizes; its two R are the two WIDE instances)
            assert r.Rs == FAMILIES["W"].Rs
            continue
        s = shape_of(r.case.obs, r.case.act, r.case.mkw)
        fits = tuple(R for R in FAMILIES[r.family].Rs if smem_bytes(16 * R, s) <= LDS_MAX)
        assert r.Rs == fits, (r.case.name, [smem_bytes(16 * R, s) for R in FAMILIES[r.family].Rs])
        if fits != FAMILIES[r.family].Rs:
            dropped[r.case.name] = sorted(set(FAMILIES[r.family].Rs) - set(fits))
    assert dropped == {"A_in256": [3], "B_in97": [4]}


def test_the_table_covers_the_edges_it_claims():
    shapes = {r.case.name: shape_of(r.case.obs, r.case.act, r.case.mkw) for r in ROWS}
    op0 = {n: s["ops"][0] for n, s in shapes.items()}
    assert {o["KC"] for o in op0.values()} >= {1, 2, 3, 4, 5, 16}
    assert {o["tail_steps"] for o in op0.values() if o["KC"] == 1} == {1, 2, 3, 4}
    # the resident twin's one-chunk head: the R = 3 rows with KC 1 visit every arm, and KC 2 next to them
    res = {n: op0[n] for n in op0 if 3 in BY_NAME[n].Rs and BY_NAME[n].family in ("P", "I")}
    for fam in ("P", "I"):
        mine = [o for n, o in res.items() if BY_NAME[n].family == fam]
        assert {o["tail_steps"] for o in mine if o["KC"] == 1} == {1, 2, 3, 4} and any(o["KC"] == 2 for o in mine), fam
    assert {r.case.mkw["hid"] for r in ROWS} == {193, 200, 204, 208}
    assert {s["ops"][1]["tail_steps"] for s in shapes.values()} == {1, 2, 3, 4}  # ... i.e. every tail of the ops fed by a hidden layer
    assert {r.case.mkw.get("num_layers", 4) for r in ROWS} == {1, 4, 7}
    for name, fam in FAMILIES.items():
        seen = {r.case.obs for r in ROWS if r.family == name}
        assert seen >= ({fam.obs_lo} if name == "W" else {fam.obs_lo, fam.obs_hi}), name  # (W: one row, the lower edge)
    for fam, hids in (("A", {193, 204, 208}), ("Ao", {193, 208}), ("B", {193, 208}), ("P", {193, 208}), ("I", {193, 208}), ("L", {193, 208}), ("H", {204})):
        assert {r.case.mkw["hid"] for r in ROWS if r.family == fam} >= hids, fam
    ins = {n: s["in_dim"] for n, s in shapes.items()}
    assert [ins[n] for n in ("A_in18", "A_in28", "A_in32", "A_in33", "A_in64", "A_in65", "A_in256")] == [18, 28, 32, 33, 64, 65, 256]
    assert [ins[n] for n in ("B_in42", "B_in64", "B_in65", "B_in97")] == [42, 64, 65, 97]
    assert [ins[n] for n in ("C_in4", "C_in16", "C_in17", "P_in4", "P_in6", "P_in12", "P_in16", "P_in17")] == [4, 16, 17, 4, 6, 12, 16, 17]
    assert [ins[n] for n in ("I_in3", "I_in5", "I_in12", "I_in16", "I_in17")] == [3, 5, 12, 16, 17]
    # full and nearly empty last output tiles; the reward column first in / last of a tile
    assert 2 * shapes["A_in32"]["out_dim"] == 48 and 2 * shapes["A_in18"]["out_dim"] == 34 and 2 * shapes["C_in16"]["out_dim"] == 16
    assert 2 * shapes["W_obs369"]["out_dim"] == 46 * 16 + 2
    assert shapes["L_obs16"]["out_dim"] - 1 == 16 and shapes["L_obs23"]["out_dim"] == 24  # output column obs: 8 c with c = 2, and 8 c + 7
    assert any(r.case.mkw.get("elite") == [0, 2, 3, 5, 6] and r.case.mkw["ensemble_size"] == 7 for r in ROWS) and {r.case.pop for r in ROWS} == {1, 40}
    assert len(CASES) == sum(2 * len(r.Rs) for r in ROWS)


def resident_heads_wanted(R, n_layers, logical, n_cu, horizon):
    """csrc/residency_rule.hpp, restated (tests/test_resident_heads_rule.py pins the compiled rule)"""
    return R == 3 and n_layers == 5 and 1 <= logical <= n_cu and horizon > 1


def test_which_device_calls_ask_for_the_resident_twin():
    """Every R = 3 row of depth 4 -- 200 rows are one 48-row workgroup per member, five logical workgroups on 256 CUs --, and no other call:
    not the depth-1 and depth-7 rows at R = 3 (the twin's heads are told apart by a switch over exactly five ops), no other R."""
    asks = set()
    for r, R, mode in CASES:
        if mode != "device":
            continue
        c = r.case
        logical = 5 * -(-(-(-(c.pop * c.P // 5) // 16)) // R)
        if resident_heads_wanted(R, shape_of(c.obs, c.act, c.mkw)["n_layers"], logical, N_CU, c.H) and r.family != "W":
            asks.add((c.name, R))
    want = {(r.case.name, 3) for r in ROWS if 3 in r.Rs and r.case.mkw.get("num_layers", 4) == 4}
    assert asks == want
    assert ("A_depth1", 3) not in asks and ("A_depth7", 3) not in asks and 3 in BY_NAME["A_depth1"].Rs and 3 in BY_NAME["A_depth7"].Rs
    assert {BY_NAME[n].family for n, _ in asks} == {"A", "Ao", "B", "P", "I"}  # the families with an R = 3 instance


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU comparison of every (row, R, mode) can see
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,R,mode", CASES, ids=CASE_IDS)
def test_row_cpu_conditions(monkeypatch, row, R, mode):
    """Against the fp32 oracle, tol_i = T2_i = 1e-4 max(1, |ref_i|), on the CPU restatement of the draws the GPU test replays (FAST: the
    member schedule of R row tiles per workgroup):
    (a) power: zeroing the last input row of layer 0, the last hidden row of layer 1 (where a hidden -> hidden layer exists), the last
        mean or the last log-variance column -- learned rewards: the reward's, AND the last state dim's -- moves some candidate's return by
        >= 4 x its tolerance (the device may itself use up to 1 x);
    (b) spread: the oracle accumulated in f64 stays within tol / 4 of itself for every candidate;
    (c) the returns are finite and no traced state is within 1e-4 of a threshold of the row's termination function: no candidate needs
        masking on the GPU;
    (d) with a termination function, some row ends before the last step and some row never ends: both sides of the termination lane."""
    f = f32_figures(monkeypatch, row.case, mode, R)
    print("F32_EDGE_CPU " + json.dumps({"case": row.case.name, "R": R, "mode": mode, **f}))
    assert f["finite"]
    assert sorted(f["power"]) == sorted(mutations_of(build(row.case)[0]))
    assert ("hid_row" in f["power"]) == (row.case.mkw.get("num_layers", 4) > 1) and ("state_lv_col" in f["power"]) == bool(row.case.mkw.get("learned_rewards"))
    assert min(f["power"].values()) >= 4.0, f["power"]
    assert f["spread"] <= 0.25, f["spread"]
    assert f["margin"] >= 1e-4, f["margin"]
    assert (f["margin"] < float("inf")) == (row.case.mkw.get("termination") is not None)
    assert f["ends_early"] and f["survives"]


@pytest.mark.parametrize("nb", NEIGHBOURS, ids=lambda n: n.name)
def test_neighbour_cpu_conditions(nb):
    """(c) for the neighbours, whose GPU test compares with the oracle at T2 on whatever geometry the default call picks"""
    om, actions, s0, _, _ = neighbour_case(nb)
    for mode, R in [("device", 1)] + [("fast", R) for R in (1, 2, 3, 4)]:
        tr = {}
        ref = po.rollout(om, actions, s0, 5, trace=tr, **cpu_draws(om, 40, 5, 4, mode, R))
        assert torch.isfinite(ref).all() and threshold_margin(om, tr) >= 1e-4, (mode, R)
