"""The shape-specialised ("lean", KSpec::FUSE) fp32 rollout instances at the edges of their shape families: one table of models, the
families' neighbours that must NOT run such an instance, and the CPU figures that say what a GPU comparison of each row can see.
Shared by tests/test_fused_f32_edges_host.py (no GPU) and tests/test_gpu_fused_f32_edges.py.

An instance accepts a family of models (csrc/launch.hpp lean_shape_is: hidden column tiles, output column tiles, reward, termination
and obs-preprocessing form, the LDS row stride); the input width (KC = Kp / 16 of op 0 is a run-time value), the action width, the depth
and the member subset are open.  The rows probe what is open, at every row-tile count R the family's table lists and in both launch
modes; a row's return is the only observable, so edge_case (tests/bf16_restatement.py) gives the edge columns enough gain to be seen and
f32_figures measures, on the CPU and on the draws the GPU tests replay, that they are."""
import collections
import dataclasses

import torch

from bf16_restatement import EdgeCase, T2_REL, MUTATIONS, cpu_draws, edge_case, mutated, reference_rollout, scaled_case, threshold_margin
from oracle import pets_oracle as po

# family -> (hidden column tiles, output column tiles, reward, termination, obs preprocessing), the R of csrc/launch.hpp
# HIPETS_LEAN_SHAPES_R<R> that list it, and the obs range the output-tile count (and, for I, launch.hpp fused_term_ok; for C, P and I the
# forms' own lower limits, csrc/model.hip) leaves.  tests/test_fused_f32_edges_host.py checks the first two against the header's text.
Family = collections.namedtuple("Family", "shape Rs obs_lo obs_hi")
FAMILIES = {
    "A": Family((13, 3, "HALFCHEETAH", "NONE", "NONE"), (1, 2, 3), 17, 24),
    "Ao": Family((13, 3, "HALFCHEETAH", "NONE", "HALFCHEETAH"), (1, 2, 3), 17, 24),
    "B": Family((13, 6, "HALFCHEETAH", "HUMANOID", "NONE"), (2, 3, 4), 41, 48),
    "C": Family((13, 1, "CARTPOLE", "CARTPOLE", "NONE"), (1, 2), 3, 8),
    "P": Family((13, 1, "CARTPOLE_PETS", "NONE", "CARTPOLE_PETS"), (3,), 2, 8),
    "I": Family((13, 1, "LEARNED", "INVERTED_PENDULUM", "NONE"), (3,), 2, 4),
    "L": Family((13, 3, "LEARNED", "NONE", "NONE"), (1, 2), 16, 23),
    "Lo": Family((13, 3, "LEARNED", "NONE", "HALFCHEETAH"), (1, 2), 16, 23),
    "H": Family((13, 2, "LEARNED", "HOPPER", "NONE"), (1, 2), 8, 15),
    "W": Family((13, 47, "HALFCHEETAH", "HUMANOID", "NONE"), (1, 2), 369, 376),  # KSpec::WIDE
}
_MKW = {
    "A": dict(),
    "Ao": dict(obs_process="halfcheetah"),
    "B": dict(termination="humanoid"),
    "C": dict(reward="cartpole", termination="cartpole", lv_bias=-5.0),  # (lv_bias: build, below)
    "P": dict(reward="cartpole_pets", obs_process="cartpole_pets"),
    "I": dict(learned_rewards=True, reward=None, termination="inverted_pendulum"),
    "L": dict(learned_rewards=True, reward=None),
    "Lo": dict(learned_rewards=True, reward=None, obs_process="halfcheetah"),
    "H": dict(learned_rewards=True, reward=None, termination="hopper"),
    "W": dict(termination="humanoid"),
}

# a table row: the family, the model and its gains (an EdgeCase), and the row-tile counts it runs at: the family's, but for A_in256
Row = collections.namedtuple("Row", "family case Rs")
F32_MUTATIONS = MUTATIONS + ("state_mean_col", "state_lv_col")  # the last two: learned-reward models only


def _row(family, name, obs, act, seed, gain, g_in, g_lv, Rs=None, pop=40, **mkw):
    kw = dict(dict(ensemble_size=5, hid=200), **_MKW[family])
    kw.update(mkw)
    return Row(family, EdgeCase(name, obs, act, kw, pop, 5, 4, seed, gain, g_in, g_lv), tuple(Rs or FAMILIES[family].Rs))


_SUBSET = dict(ensemble_size=7, elite=[0, 2, 3, 5, 6])
# name, obs, act, (seed, gain, g_in, g_lv) -- all pop 40 x P 5 (200 rows, 40 per member), H 4, five members, but A_pop1 (five rows).  Seed and
# gains come from the search tests/bf16_restatement.py describes (seeds 0..47 x (g_in, g_lv) x gain in {2, 3}; the bf16x3 entries of
# families A and B first), for the first triple at which every condition of tests/test_fused_f32_edges_host.py holds in both launch modes
# and at every R of the row.  (B_in42 and B_in97 left their bf16x3 entries, at which no row survives the FAST draws of R = 4 and R = 2:
# condition (d).)
ROWS = [
    # --- A: X(13, 3, HALFCHEETAH, NONE, NONE), obs 17..24, R 1 / 2 / 3
    _row("A", "A_in18", 17, 1, 1, 2.0, 4.0, 8.0),        # KC 2 (the producer deals 0-1-0-1), tail 1: two live columns in the second chunk; 14 padding columns in output tile 3
    _row("A", "A_in28", 24, 4, 0, 2.0, 16.0, 8.0),       # KC 2, tail 3
    _row("A", "A_in32", 24, 8, 2, 2.0, 4.0, 4.0),        # KC 2, tail 4; output tiles exactly full
    _row("A", "A_in33", 24, 9, 1, 2.0, 8.0, 4.0),        # KC 3: the K-split producer deals 0-1-1-1 chunks to waves 0..3
    _row("A", "A_in64", 17, 47, 3, 2.0, 4.0, 8.0),       # KC 4: one chunk per wave
    _row("A", "A_in65", 20, 45, 3, 2.0, 32.0, 8.0),      # KC 5: 1-1-1-2
    # KC 16, the family's last input width (in 257 has another LDS row stride): every K-split slot full.  232 action columns: the
    # double-buffered actions take 2 x 16 R x 232 x 4 bytes next to 2 x 16 R x 264 x 4 of activations -- R = 3 does not fit 160 KiB
    _row("A", "A_in256", 24, 232, 30, 2.0, 16.0, 8.0, Rs=(1, 2)),
    _row("A", "A_hid193", 17, 6, 8, 2.0, 16.0, 8.0, hid=193),   # tail_steps 1 of every hidden-fed op: the 13th tile holds ONE live column
    _row("A", "A_hid204", 20, 6, 0, 2.0, 16.0, 8.0, hid=204),   # tail_steps 3
    _row("A", "A_hid208", 24, 6, 0, 2.0, 4.0, 8.0, hid=208),    # tail_steps 4
    _row("A", "A_depth1", 17, 6, 0, 2.0, 8.0, 8.0, num_layers=1),   # two ops: the output layer reads partial buffer (2 - 2) & 1
    _row("A", "A_depth7", 24, 9, 2, 2.0, 16.0, 8.0, num_layers=7),  # eight ops
    _row("A", "A_subset", 24, 9, 4, 2.0, 4.0, 4.0, **_SUBSET),      # 7 members, elites [0, 2, 3, 5, 6]
    _row("A", "A_pop1", 24, 9, 0, 2.0, 16.0, 8.0, pop=1),           # one candidate: five rows, one per member
    # --- A with obs preprocessing: X(13, 3, HALFCHEETAH, NONE, HALFCHEETAH)
    _row("Ao", "Ao_obs17_hid193", 17, 6, 0, 2.0, 16.0, 8.0, hid=193),
    _row("Ao", "Ao_obs17_hid208", 17, 6, 0, 2.0, 16.0, 8.0, hid=208),
    _row("Ao", "Ao_obs24_hid193", 24, 6, 0, 2.0, 16.0, 8.0, hid=193),
    _row("Ao", "Ao_obs24_hid208", 24, 6, 0, 2.0, 16.0, 8.0, hid=208),
    # --- B: X(13, 6, HALFCHEETAH, HUMANOID, NONE), obs 41..48, R 2 / 3 / 4
    _row("B", "B_in42", 41, 1, 0, 2.0, 16.0, 8.0),
    _row("B", "B_in64", 48, 16, 4, 2.0, 8.0, 8.0),       # output tiles exactly full
    _row("B", "B_in65", 48, 17, 2, 2.0, 32.0, 8.0),
    _row("B", "B_in97", 41, 56, 3, 2.0, 16.0, 8.0, Rs=(2, 3)),   # 56 action columns: four row tiles do not fit the LDS
    _row("B", "B_hid193", 48, 17, 0, 2.0, 16.0, 8.0, hid=193),
    _row("B", "B_hid208", 48, 17, 0, 2.0, 16.0, 8.0, hid=208),
    # --- C: X(13, 1, CARTPOLE, CARTPOLE, NONE), obs 3..8 (the forms read dims 0 and 2), one output tile, R 1 / 2
    _row("C", "C_in4", 3, 1, 2, 2.0, 16.0, 8.0),         # the smallest obs; KC 1, tail 1
    _row("C", "C_in16", 8, 8, 3, 2.0, 16.0, 8.0),        # the output tile exactly full; KC 1, tail 4
    _row("C", "C_in17", 8, 9, 2, 2.0, 16.0, 8.0),        # KC 2
    # --- P: X(13, 1, CARTPOLE_PETS, NONE, CARTPOLE_PETS), obs 2..8 (in = obs + 1 + act), R 3: the resident twin's one-chunk head
    _row("P", "P_in4", 2, 1, 0, 2.0, 16.0, 8.0),         # tail 1
    _row("P", "P_in6", 4, 1, 0, 2.0, 16.0, 8.0),         # tail 2: pets_cartpole_paper_version
    _row("P", "P_in12", 8, 3, 0, 2.0, 16.0, 8.0),        # tail 3; the output tile exactly full
    _row("P", "P_in16", 8, 7, 0, 2.0, 16.0, 8.0),        # tail 4
    _row("P", "P_in17", 8, 8, 0, 2.0, 16.0, 8.0),        # KC 2: the first width that leaves the one-chunk head
    _row("P", "P_hid193", 4, 1, 0, 2.0, 16.0, 8.0, hid=193),
    _row("P", "P_hid208", 4, 1, 0, 2.0, 16.0, 8.0, hid=208),
    # --- I: X(13, 1, LEARNED, INVERTED_PENDULUM, NONE), obs 2..4, R 3
    _row("I", "I_in3", 2, 1, 2, 2.0, 16.0, 8.0),         # tail 1; the reward column is output column 2
    _row("I", "I_in5", 4, 1, 38, 2.0, 16.0, 8.0),         # tail 2: pets_inv_pendulum
    _row("I", "I_in12", 4, 8, 8, 2.0, 16.0, 8.0),        # tail 3
    _row("I", "I_in16", 4, 12, 8, 2.0, 16.0, 8.0),       # tail 4
    _row("I", "I_in17", 4, 13, 25, 2.0, 16.0, 8.0),       # KC 2
    _row("I", "I_hid193", 4, 1, 14, 2.0, 8.0, 4.0, hid=193),
    _row("I", "I_hid208", 4, 1, 14, 2.0, 16.0, 8.0, hid=208),
    # --- L: X(13, 3, LEARNED, NONE, NONE / HALFCHEETAH), obs 16..23, R 1 / 2: the reward column (output column obs) is the first of
    # column tile 2 in the head-pair order at obs 16 and the last live column of the third tile at obs 23
    _row("L", "L_obs16", 16, 7, 0, 2.0, 16.0, 8.0),
    _row("L", "L_obs23", 23, 7, 0, 2.0, 16.0, 8.0),
    _row("L", "L_hid193", 16, 7, 0, 2.0, 16.0, 8.0, hid=193),
    _row("L", "L_hid208", 23, 7, 0, 2.0, 16.0, 8.0, hid=208),
    _row("Lo", "Lo_obs16", 16, 7, 0, 2.0, 16.0, 8.0),
    _row("Lo", "Lo_obs23", 23, 7, 0, 2.0, 16.0, 8.0),
    # --- H: X(13, 2, LEARNED, HOPPER, NONE), obs 8..15, two output tiles, R 1 / 2
    _row("H", "H_obs8", 8, 3, 33, 2.0, 16.0, 4.0),
    _row("H", "H_obs15", 15, 3, 6, 2.0, 16.0, 8.0),
    _row("H", "H_hid204", 11, 3, 11, 2.0, 8.0, 4.0, hid=204),
    # --- W: X(13, 47, HALFCHEETAH, HUMANOID, NONE), KSpec::WIDE, the family's lower obs edge: 738 output columns = 46 tiles and two columns
    _row("W", "W_obs369", 369, 1, 0, 2.0, 16.0, 8.0),
]
BY_NAME = {r.case.name: r for r in ROWS}
CASES = [(r, R, mode) for r in ROWS for R in r.Rs for mode in ("device", "fast")]
CASE_IDS = [f"{r.case.name}-R{R}-{mode}" for r, R, mode in CASES]

# The neighbours: one step outside a family.  None may run a fused instance (W's: nor the WIDE one).  (name, family it is next to, obs,
# act, model kwargs, seed): stock weights x 2 (scaled_case), the seed the first of 0..47 at which no traced state is within 1e-4 of a
# threshold of the termination function on the DEVICE draws and the FAST draws of every R.
Neighbour = collections.namedtuple("Neighbour", "name family obs act mkw seed")


def _nb(name, family, obs, act, seed=0, **mkw):
    kw = dict(dict(ensemble_size=5, hid=200), **_MKW[family])
    kw.update(mkw)
    return Neighbour(name, family, obs, act, kw, seed)


NEIGHBOURS = [
    _nb("A_obs16", "A", 16, 6), _nb("A_obs25", "A", 25, 6),   # two / four output tiles
    _nb("A_hid192", "A", 17, 6, hid=192), _nb("A_hid209", "A", 17, 6, hid=209),   # twelve / fourteen hidden tiles
    _nb("A_in257", "A", 24, 233),    # Kp 272: the LDS row stride goes from 264 to 328 floats
    _nb("I_obs5", "I", 5, 1),        # inverted_pendulum tests every state dim: the tail's lane holds four (launch.hpp fused_term_ok)
    _nb("LT_obs8", "I", 8, 1, termination="cartpole"),   # learned reward + a termination function: the reward column must sit in tile 0 (obs < 8)
    _nb("W_obs368", "W", 368, 1),    # 46 output tiles
]


def neighbour_case(nb):
    return scaled_case(nb.obs, nb.act, 40, 5, 4, seed=nb.seed, gain=2.0, **nb.mkw)


def build(case):
    """edge_case of the row.  Family C carries `lv_bias`, a bias on every log-variance column of the output layer: the synthetic
    initialiser (zero biases) samples with std 0.8 per step, and the cartpole forms end a row at |theta| > 0.21 and pay 0 or 1 -- four of
    five rows end at every step, no row survives four, and a return moves only where a row crosses a threshold.  At -5 (std 0.08, a
    trained model's scale) rows end at every step, some survive, and the log-variance columns stay inside their bounds, i.e. visible."""
    mkw = dict(case.mkw)
    lv_bias = mkw.pop("lv_bias", None)
    om, *rest = edge_case(case.obs, case.act, case.pop, case.P, case.H, seed=case.seed, gain=case.gain, g_in=case.g_in, g_lv=case.g_lv, **mkw)
    if lv_bias is not None:
        b = [x.clone() for x in om.biases]
        b[-1][:, :, om.out_size:] = lv_bias
        om = dataclasses.replace(om, biases=b)
    return (om, *rest)


def mutations_of(om):
    """the mutations that apply to `om`: hid_row needs a hidden -> hidden layer, the state columns a learned reward"""
    return [m for m in F32_MUTATIONS if (m != "hid_row" or len(om.weights) >= 3) and (om.learned_rewards or not m.startswith("state_"))]


def mutated_f32(om, which):
    """bf16_restatement.mutated, and for learned-reward models (whose columns out - 1 / 2 out - 1 are the REWARD's) the last STATE dim's
    mean ("state_mean_col": column obs - 1) or log-variance ("state_lv_col": column out + obs - 1) column zeroed."""
    if not which.startswith("state_"):
        return mutated(om, which)
    w = [x.clone() for x in om.weights]
    out = om.out_size
    b = [x.clone() for x in om.biases]
    col = out - 2 if which == "state_mean_col" else 2 * out - 2
    w[-1][:, :, col] = 0
    b[-1][:, :, col] = 0
    return dataclasses.replace(om, weights=w, biases=b)


def t2(ref):
    return T2_REL * torch.clamp(ref.abs(), min=1.0)


def termination_use(om, trace):
    """(some row terminates before the last step, some row never terminates) of a traced rollout; (True, True) without a termination fn"""
    if om.termination == "no_termination":
        return True, True
    done = torch.stack(trace["dones"])[..., 0]  # [H, B]
    return bool(done[:-1].any()), bool((~done.any(0)).any())


def f32_figures(monkeypatch, case, mode, R, draws=None, cheap_first=False):
    """The CPU conditions of one row against the fp32 oracle at T2, on the draws of `mode` at R row tiles: power (per applicable mutation
    the largest |mutated - clean| / tol over candidates), spread (the largest |ref - f64-accumulated ref| / tol), margin (threshold_margin
    of the reference), finite, ends_early / survives (termination_use).  cheap_first: stop after the reference rollout where its own
    conditions fail (the search)."""
    om, actions, s0, _, _ = build(case)
    kw = draws if draws is not None else cpu_draws(om, case.pop, case.P, case.H, mode, R)
    tr = {}
    ref = po.rollout(om, actions, s0, case.P, trace=tr, **kw)
    early, survives = termination_use(om, tr)
    f = dict(finite=bool(torch.isfinite(ref).all()), margin=threshold_margin(om, tr), ends_early=early, survives=survives, power={}, spread=float("inf"))
    if cheap_first and not (f["finite"] and f["margin"] >= 1e-4 and early and survives):
        return f
    tol = t2(ref)
    for which in mutations_of(om):
        f["power"][which] = ((po.rollout(mutated_f32(om, which), actions, s0, case.P, **kw) - ref).abs() / tol).max().item()
        if cheap_first and f["power"][which] < 4.0:
            return f
    # (the fp32 oracle is the reference of bf16x3: its f64-accumulated twin)
    f["spread"] = ((reference_rollout(monkeypatch, "bf16x3", om, actions, s0, case.P, acc64=True, **kw) - ref).abs() / tol).max().item()
    return f


def holds(f, om):
    return (f["finite"] and f["margin"] >= 1e-4 and f["ends_early"] and f["survives"] and sorted(f["power"]) == sorted(mutations_of(om)) and
            min(f["power"].values()) >= 4.0 and f["spread"] <= 0.25)


# CPU figures of the table (tests/test_fused_f32_edges_host.py asserts them; draws of (SEED, SID), oracle/device_draws.py), per row, row-tile
# count and launch mode: power = the smallest over the applicable mutations of max |mutated - clean| / T2 (>= 4), spread = max |ref -
# f64-accumulated ref| / T2 (<= 0.25), margin = distance of the nearest traced state from a threshold of the termination function
# (>= 1e-4).  Every row with a termination function has rows that end before the last step and rows that never end.
#   row             seed gain g_in/g_lv  R  mode      power  spread    margin
#   A_in18            1 2 4/8  R1 device      37.4  0.004       inf
#   A_in18            1 2 4/8  R1 fast        38.7  0.002       inf
#   A_in18            1 2 4/8  R2 device      37.4  0.004       inf
#   A_in18            1 2 4/8  R2 fast        47.5  0.002       inf
#   A_in18            1 2 4/8  R3 device      37.4  0.004       inf
#   A_in18            1 2 4/8  R3 fast        61.6  0.006       inf
#   A_in28            0 2 16/8  R1 device     369.6  0.005       inf
#   A_in28            0 2 16/8  R1 fast       379.2  0.005       inf
#   A_in28            0 2 16/8  R2 device     369.6  0.005       inf
#   A_in28            0 2 16/8  R2 fast       299.7  0.005       inf
#   A_in28            0 2 16/8  R3 device     369.6  0.005       inf
#   A_in28            0 2 16/8  R3 fast       373.5  0.006       inf
#   A_in32            2 2 4/4  R1 device      17.9  0.003       inf
#   A_in32            2 2 4/4  R1 fast        28.4  0.004       inf
#   A_in32            2 2 4/4  R2 device      17.9  0.003       inf
#   A_in32            2 2 4/4  R2 fast        28.4  0.004       inf
#   A_in32            2 2 4/4  R3 device      17.9  0.003       inf
#   A_in32            2 2 4/4  R3 fast        60.7  0.004       inf
#   A_in33            1 2 8/4  R1 device      64.2  0.006       inf
#   A_in33            1 2 8/4  R1 fast        74.4  0.003       inf
#   A_in33            1 2 8/4  R2 device      64.2  0.006       inf
#   A_in33            1 2 8/4  R2 fast        70.3  0.002       inf
#   A_in33            1 2 8/4  R3 device      64.2  0.006       inf
#   A_in33            1 2 8/4  R3 fast        88.9  0.004       inf
#   A_in64            3 2 4/8  R1 device      11.6  0.003       inf
#   A_in64            3 2 4/8  R1 fast         4.4  0.003       inf
#   A_in64            3 2 4/8  R2 device      11.6  0.003       inf
#   A_in64            3 2 4/8  R2 fast         7.5  0.001       inf
#   A_in64            3 2 4/8  R3 device      11.6  0.003       inf
#   A_in64            3 2 4/8  R3 fast        16.4  0.002       inf
#   A_in65            3 2 32/8  R1 device     262.4  0.009       inf
#   A_in65            3 2 32/8  R1 fast       227.1  0.018       inf
#   A_in65            3 2 32/8  R2 device     262.4  0.009       inf
#   A_in65            3 2 32/8  R2 fast       165.9  0.006       inf
#   A_in65            3 2 32/8  R3 device     262.4  0.009       inf
#   A_in65            3 2 32/8  R3 fast       359.0  0.011       inf
#   A_in256          30 2 16/8  R1 device       5.4  0.001       inf
#   A_in256          30 2 16/8  R1 fast         7.1  0.001       inf
#   A_in256          30 2 16/8  R2 device       5.4  0.001       inf
#   A_in256          30 2 16/8  R2 fast         7.6  0.001       inf
#   A_hid193          8 2 16/8  R1 device     238.0  0.005       inf
#   A_hid193          8 2 16/8  R1 fast       239.2  0.007       inf
#   A_hid193          8 2 16/8  R2 device     238.0  0.005       inf
#   A_hid193          8 2 16/8  R2 fast       229.9  0.006       inf
#   A_hid193          8 2 16/8  R3 device     238.0  0.005       inf
#   A_hid193          8 2 16/8  R3 fast       431.4  0.008       inf
#   A_hid204          0 2 16/8  R1 device     294.0  0.006       inf
#   A_hid204          0 2 16/8  R1 fast       308.6  0.006       inf
#   A_hid204          0 2 16/8  R2 device     294.0  0.006       inf
#   A_hid204          0 2 16/8  R2 fast       277.8  0.005       inf
#   A_hid204          0 2 16/8  R3 device     294.0  0.006       inf
#   A_hid204          0 2 16/8  R3 fast       259.2  0.006       inf
#   A_hid208          0 2 4/8  R1 device      68.9  0.004       inf
#   A_hid208          0 2 4/8  R1 fast       191.6  0.004       inf
#   A_hid208          0 2 4/8  R2 device      68.9  0.004       inf
#   A_hid208          0 2 4/8  R2 fast        87.9  0.003       inf
#   A_hid208          0 2 4/8  R3 device      68.9  0.004       inf
#   A_hid208          0 2 4/8  R3 fast       108.4  0.004       inf
#   A_depth1          0 2 8/8  R1 device    3730.1  0.027       inf
#   A_depth1          0 2 8/8  R1 fast      2810.4  0.032       inf
#   A_depth1          0 2 8/8  R2 device    3730.1  0.027       inf
#   A_depth1          0 2 8/8  R2 fast      3116.8  0.017       inf
#   A_depth1          0 2 8/8  R3 device    3730.1  0.027       inf
#   A_depth1          0 2 8/8  R3 fast      2171.7  0.014       inf
#   A_depth7          2 2 16/8  R1 device      21.0  0.001       inf
#   A_depth7          2 2 16/8  R1 fast        11.9  0.002       inf
#   A_depth7          2 2 16/8  R2 device      21.0  0.001       inf
#   A_depth7          2 2 16/8  R2 fast        15.8  0.002       inf
#   A_depth7          2 2 16/8  R3 device      21.0  0.001       inf
#   A_depth7          2 2 16/8  R3 fast         7.0  0.002       inf
#   A_subset          4 2 4/4  R1 device      31.6  0.003       inf
#   A_subset          4 2 4/4  R1 fast        17.4  0.004       inf
#   A_subset          4 2 4/4  R2 device      31.6  0.003       inf
#   A_subset          4 2 4/4  R2 fast        41.4  0.002       inf
#   A_subset          4 2 4/4  R3 device      31.6  0.003       inf
#   A_subset          4 2 4/4  R3 fast        58.1  0.003       inf
#   A_pop1            0 2 16/8  R1 device      11.6  0.000       inf
#   A_pop1            0 2 16/8  R1 fast        25.3  0.000       inf
#   A_pop1            0 2 16/8  R2 device      11.6  0.000       inf
#   A_pop1            0 2 16/8  R2 fast        25.3  0.000       inf
#   A_pop1            0 2 16/8  R3 device      11.6  0.000       inf
#   A_pop1            0 2 16/8  R3 fast        25.3  0.000       inf
#   Ao_obs17_hid193   0 2 16/8  R1 device     560.2  0.013       inf
#   Ao_obs17_hid193   0 2 16/8  R1 fast       373.7  0.029       inf
#   Ao_obs17_hid193   0 2 16/8  R2 device     560.2  0.013       inf
#   Ao_obs17_hid193   0 2 16/8  R2 fast       322.2  0.010       inf
#   Ao_obs17_hid193   0 2 16/8  R3 device     560.2  0.013       inf
#   Ao_obs17_hid193   0 2 16/8  R3 fast       241.5  0.014       inf
#   Ao_obs17_hid208   0 2 16/8  R1 device     331.2  0.012       inf
#   Ao_obs17_hid208   0 2 16/8  R1 fast       502.8  0.013       inf
#   Ao_obs17_hid208   0 2 16/8  R2 device     331.2  0.012       inf
#   Ao_obs17_hid208   0 2 16/8  R2 fast       478.0  0.019       inf
#   Ao_obs17_hid208   0 2 16/8  R3 device     331.2  0.012       inf
#   Ao_obs17_hid208   0 2 16/8  R3 fast       363.5  0.017       inf
#   Ao_obs24_hid193   0 2 16/8  R1 device     244.6  0.010       inf
#   Ao_obs24_hid193   0 2 16/8  R1 fast       494.3  0.013       inf
#   Ao_obs24_hid193   0 2 16/8  R2 device     244.6  0.010       inf
#   Ao_obs24_hid193   0 2 16/8  R2 fast       230.0  0.008       inf
#   Ao_obs24_hid193   0 2 16/8  R3 device     244.6  0.010       inf
#   Ao_obs24_hid193   0 2 16/8  R3 fast       164.0  0.008       inf
#   Ao_obs24_hid208   0 2 16/8  R1 device     282.4  0.011       inf
#   Ao_obs24_hid208   0 2 16/8  R1 fast       300.0  0.008       inf
#   Ao_obs24_hid208   0 2 16/8  R2 device     282.4  0.011       inf
#   Ao_obs24_hid208   0 2 16/8  R2 fast       349.3  0.008       inf
#   Ao_obs24_hid208   0 2 16/8  R3 device     282.4  0.011       inf
#   Ao_obs24_hid208   0 2 16/8  R3 fast       359.5  0.010       inf
#   B_in42            0 2 16/8  R2 device      28.6  0.001   8.3e-04
#   B_in42            0 2 16/8  R2 fast       109.5  0.002   1.5e-04
#   B_in42            0 2 16/8  R3 device      28.6  0.001   8.3e-04
#   B_in42            0 2 16/8  R3 fast        88.8  0.002   4.0e-04
#   B_in42            0 2 16/8  R4 device      28.6  0.001   8.3e-04
#   B_in42            0 2 16/8  R4 fast        19.8  0.002   7.0e-04
#   B_in64            4 2 8/8  R2 device      53.4  0.002   2.4e-03
#   B_in64            4 2 8/8  R2 fast        96.0  0.002   1.4e-03
#   B_in64            4 2 8/8  R3 device      53.4  0.002   2.4e-03
#   B_in64            4 2 8/8  R3 fast       919.4  0.003   1.9e-04
#   B_in64            4 2 8/8  R4 device      53.4  0.002   2.4e-03
#   B_in64            4 2 8/8  R4 fast        90.0  0.002   2.8e-03
#   B_in65            2 2 32/8  R2 device      79.6  0.002   9.9e-04
#   B_in65            2 2 32/8  R2 fast       135.0  0.004   8.8e-04
#   B_in65            2 2 32/8  R3 device      79.6  0.002   9.9e-04
#   B_in65            2 2 32/8  R3 fast        91.5  0.002   9.9e-04
#   B_in65            2 2 32/8  R4 device      79.6  0.002   9.9e-04
#   B_in65            2 2 32/8  R4 fast       190.8  0.006   2.0e-04
#   B_in97            3 2 16/8  R2 device      59.6  0.003   1.9e-03
#   B_in97            3 2 16/8  R2 fast        41.9  0.002   1.4e-03
#   B_in97            3 2 16/8  R3 device      59.6  0.003   1.9e-03
#   B_in97            3 2 16/8  R3 fast        52.4  0.003   7.0e-04
#   B_hid193          0 2 16/8  R2 device      55.6  0.002   1.2e-03
#   B_hid193          0 2 16/8  R2 fast        36.1  0.001   7.2e-04
#   B_hid193          0 2 16/8  R3 device      55.6  0.002   1.2e-03
#   B_hid193          0 2 16/8  R3 fast        42.9  0.002   3.6e-04
#   B_hid193          0 2 16/8  R4 device      55.6  0.002   1.2e-03
#   B_hid193          0 2 16/8  R4 fast        39.8  0.002   2.2e-04
#   B_hid208          0 2 16/8  R2 device      47.5  0.002   1.0e-03
#   B_hid208          0 2 16/8  R2 fast        52.9  0.002   9.6e-04
#   B_hid208          0 2 16/8  R3 device      47.5  0.002   1.0e-03
#   B_hid208          0 2 16/8  R3 fast        63.9  0.004   8.0e-04
#   B_hid208          0 2 16/8  R4 device      47.5  0.002   1.0e-03
#   B_hid208          0 2 16/8  R4 fast       141.1  0.002   1.3e-03
#   C_in4             2 2 16/8  R1 device    1500.0  0.000   7.1e-04
#   C_in4             2 2 16/8  R1 fast      1000.0  0.000   1.6e-04
#   C_in4             2 2 16/8  R2 device    1500.0  0.000   7.1e-04
#   C_in4             2 2 16/8  R2 fast      1333.3  0.000   3.7e-04
#   C_in16            3 2 16/8  R1 device    1250.0  0.000   3.0e-04
#   C_in16            3 2 16/8  R1 fast       714.3  0.000   2.9e-04
#   C_in16            3 2 16/8  R2 device    1250.0  0.000   3.0e-04
#   C_in16            3 2 16/8  R2 fast       625.0  0.000   2.0e-04
#   C_in17            2 2 16/8  R1 device    1333.3  0.000   5.7e-04
#   C_in17            2 2 16/8  R1 fast       588.2  0.000   5.0e-04
#   C_in17            2 2 16/8  R2 device    1333.3  0.000   5.7e-04
#   C_in17            2 2 16/8  R2 fast       588.2  0.000   1.3e-04
#   P_in4             0 2 16/8  R3 device     834.9  0.013       inf
#   P_in4             0 2 16/8  R3 fast       707.5  0.017       inf
#   P_in6             0 2 16/8  R3 device     389.4  0.006       inf
#   P_in6             0 2 16/8  R3 fast       129.8  0.008       inf
#   P_in12            0 2 16/8  R3 device     136.9  0.003       inf
#   P_in12            0 2 16/8  R3 fast        70.8  0.004       inf
#   P_in16            0 2 16/8  R3 device     143.0  0.001       inf
#   P_in16            0 2 16/8  R3 fast       262.9  0.002       inf
#   P_in17            0 2 16/8  R3 device     100.0  0.005       inf
#   P_in17            0 2 16/8  R3 fast        98.6  0.001       inf
#   P_hid193          0 2 16/8  R3 device     306.7  0.004       inf
#   P_hid193          0 2 16/8  R3 fast       204.7  0.004       inf
#   P_hid208          0 2 16/8  R3 device     292.6  0.008       inf
#   P_hid208          0 2 16/8  R3 fast       294.2  0.006       inf
#   I_in3             2 2 16/8  R3 device      49.8  0.004   2.1e-03
#   I_in3             2 2 16/8  R3 fast      2881.0  0.006   1.7e-03
#   I_in5            38 2 16/8  R3 device     327.6  0.003   5.0e-04
#   I_in5            38 2 16/8  R3 fast      1556.7  0.004   1.8e-03
#   I_in12            8 2 16/8  R3 device     117.5  0.003   1.3e-04
#   I_in12            8 2 16/8  R3 fast        73.5  0.002   3.1e-03
#   I_in16            8 2 16/8  R3 device      74.5  0.003   4.1e-03
#   I_in16            8 2 16/8  R3 fast       250.9  0.002   8.3e-04
#   I_in17           25 2 16/8  R3 device     161.8  0.004   3.0e-03
#   I_in17           25 2 16/8  R3 fast       168.8  0.003   1.6e-03
#   I_hid193         14 2 8/4  R3 device      35.4  0.002   2.0e-03
#   I_hid193         14 2 8/4  R3 fast        50.3  0.001   3.5e-04
#   I_hid208         14 2 16/8  R3 device     288.1  0.003   5.3e-04
#   I_hid208         14 2 16/8  R3 fast       294.0  0.004   5.2e-04
#   L_obs16           0 2 16/8  R1 device     241.8  0.005       inf
#   L_obs16           0 2 16/8  R1 fast       363.0  0.006       inf
#   L_obs16           0 2 16/8  R2 device     241.8  0.005       inf
#   L_obs16           0 2 16/8  R2 fast       273.5  0.006       inf
#   L_obs23           0 2 16/8  R1 device     404.5  0.004       inf
#   L_obs23           0 2 16/8  R1 fast       254.9  0.006       inf
#   L_obs23           0 2 16/8  R2 device     404.5  0.004       inf
#   L_obs23           0 2 16/8  R2 fast       329.2  0.005       inf
#   L_hid193          0 2 16/8  R1 device     167.3  0.005       inf
#   L_hid193          0 2 16/8  R1 fast       278.4  0.008       inf
#   L_hid193          0 2 16/8  R2 device     167.3  0.005       inf
#   L_hid193          0 2 16/8  R2 fast       228.3  0.004       inf
#   L_hid208          0 2 16/8  R1 device     285.2  0.005       inf
#   L_hid208          0 2 16/8  R1 fast       386.3  0.004       inf
#   L_hid208          0 2 16/8  R2 device     285.2  0.005       inf
#   L_hid208          0 2 16/8  R2 fast       245.2  0.005       inf
#   Lo_obs16          0 2 16/8  R1 device     273.3  0.006       inf
#   Lo_obs16          0 2 16/8  R1 fast       367.1  0.005       inf
#   Lo_obs16          0 2 16/8  R2 device     273.3  0.006       inf
#   Lo_obs16          0 2 16/8  R2 fast       274.0  0.006       inf
#   Lo_obs23          0 2 16/8  R1 device     361.4  0.004       inf
#   Lo_obs23          0 2 16/8  R1 fast       289.5  0.007       inf
#   Lo_obs23          0 2 16/8  R2 device     361.4  0.004       inf
#   Lo_obs23          0 2 16/8  R2 fast       362.6  0.005       inf
#   H_obs8           33 2 16/4  R1 device      58.6  0.002   1.1e-03
#   H_obs8           33 2 16/4  R1 fast        43.7  0.003   6.3e-04
#   H_obs8           33 2 16/4  R2 device      58.6  0.002   1.1e-03
#   H_obs8           33 2 16/4  R2 fast        62.3  0.004   3.2e-03
#   H_obs15           6 2 16/8  R1 device     490.9  0.004   6.8e-04
#   H_obs15           6 2 16/8  R1 fast       309.2  0.003   8.9e-04
#   H_obs15           6 2 16/8  R2 device     490.9  0.004   6.8e-04
#   H_obs15           6 2 16/8  R2 fast       144.6  0.003   7.4e-04
#   H_hid204         11 2 8/4  R1 device      37.9  0.002   2.5e-03
#   H_hid204         11 2 8/4  R1 fast        85.1  0.002   2.8e-03
#   H_hid204         11 2 8/4  R2 device      37.9  0.002   2.5e-03
#   H_hid204         11 2 8/4  R2 fast       160.4  0.002   1.4e-03
#   W_obs369          0 2 16/8  R1 device       9.1  0.001   2.5e-03
#   W_obs369          0 2 16/8  R1 fast        11.8  0.002   2.5e-03
#   W_obs369          0 2 16/8  R2 device       9.1  0.001   2.5e-03
#   W_obs369          0 2 16/8  R2 fast         7.8  0.002   1.4e-03
