"""The arithmetic of precision='bf16' (include/hipets.h HIPETS_PREC_BF16), restated on the oracle: for every linear layer both
operands are rounded to bf16 (round-to-nearest-even), products are exact, accumulation is fp32; bias, activation and everything
outside the linear layers stay fp32.  Shared by tests/test_bf16_host.py and tests/test_gpu_bf16.py."""
import collections
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from oracle import device_draws, feistel_perm
from oracle import pets_oracle as po
from test_gpu_rollout import _random_case


def bf16_rne_bits(x):
    """numpy restatement of csrc/gemm_bf16.hpp bf16_rne_bits: the bf16 nearest-even rounding of finite fp32 values, as fp32."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def members_forward_bf16(m, x):
    """pets_oracle._members_forward with both operands of every matmul rounded to bf16."""
    el = m.active_members
    act = po._ACT[m.activation]
    h = x
    nl = len(m.weights)
    for li in range(nl):
        w = m.weights[li][el, ...]
        b = m.biases[li][el, ...]
        h = h.to(torch.bfloat16).float().matmul(w.to(torch.bfloat16).float()) + b
        if li < nl - 1:
            h = act(h)
    if m.deterministic:
        return h, None
    out = m.out_size
    mean = h[..., :out]
    logvar = h[..., out:]
    logvar = m.max_logvar - F.softplus(m.max_logvar - logvar)
    logvar = m.min_logvar + F.softplus(logvar - m.min_logvar)
    return mean, logvar


def scaled_case(obs, act, pop, P, H, seed=0, gain=2.0, **mkw):
    """test_gpu_rollout._random_case with every weight tensor multiplied by `gain`: the stock synthetic initialiser
    (std 1 / (2 sqrt(in))) has too little gain to tell bf16 from fp32 in one step."""
    om, actions, s0, perms, eps = _random_case(obs, act, pop, P, H, seed=seed, **mkw)
    om = dataclasses.replace(om, weights=[w * gain for w in om.weights])
    return om, actions, s0, perms, eps


def emulated_rollout(monkeypatch, om, actions, s0, P, **kw):
    """po.rollout with the bf16 restatement installed (called directly: the oracle memo never sees it)."""
    with monkeypatch.context() as mp:
        mp.setattr(po, "_members_forward", members_forward_bf16)
        return po.rollout(om, actions, s0, P, **kw)


CFG2 = (17, 6, 500, 20, dict(ensemble_size=5, hid=200))
T1_ATOL = 2e-6   # the fp32 mode's one-step tolerance
T2_REL = 1e-4    # ... and its whole-rollout tolerance: |err| <= 1e-4 max(1, |v|)


# ---------------------------------------------------------------------------------------------------------------------
# Edge probes of the two bf16 / bf16x3 instance families (csrc/launch.hpp b3_shape_is: hid 193..208, obs 17..24 without
# termination -- family A -- or 41..48 with the humanoid one -- family B --, any act_dim, 2..8 linear layers, any member subset).
# The rollout's return is the only observable of these instances, and the halfcheetah reward reads state dim 0 alone: on the stock
# initialiser a lost edge column (the last input row, the last hidden row, the last mean or log-variance column) moves no return by
# as much as the comparison's tolerance.  edge_case() gives the edge columns enough gain to be seen; edge_figures() measures, on the
# CPU and on the draws the GPU tests replay, that they are.
# ---------------------------------------------------------------------------------------------------------------------
SEED, SID = 31, 4  # the (seed, stream) of every GPU replay of these modes
MUTATIONS = ("in_row", "hid_row", "mean_col", "lv_col")
NUDGES = (-2, -1, 1, 2)


def input_rows_of_state_dim(obs_process, d):
    """The layer-0 input rows state dim `d` feeds after obs preprocessing (oracle/pets_oracle.py obs_halfcheetah: [s1, sin s2, cos s2,
    s3:], the same width; obs_cartpole_pets: [sin s1, cos s1, s0, s2:], one column more)."""
    if obs_process == "halfcheetah":
        return {0: [], 1: [0], 2: [1, 2]}.get(d, [d])
    if obs_process == "cartpole_pets":
        return {0: [2], 1: [0, 1]}.get(d, [d + 1])
    return [d]


def edge_case(obs, act, pop, P, H, seed=0, gain=2.0, g_in=16.0, g_lv=8.0, **mkw):
    """scaled_case, and on top of `gain`: the layer-0 input row(s) state dim obs - 1 feeds after obs preprocessing times `g_in`, the
    output layer's column 2 out - 1 (the last log-variance) times `g_lv`.  The last state dim then feeds back into the network at every
    step, and its own mean and variance -- the last mean column, the last log-variance column -- reach state dim 0, which the reward
    reads.  Learned rewards: columns out - 1 / 2 out - 1 are the REWARD's mean and log-variance; the last state dim's own log-variance
    column, out + obs - 1, gets `g_lv` too -- both paths into the return are gained."""
    om, actions, s0, perms, eps = scaled_case(obs, act, pop, P, H, seed=seed, gain=gain, **mkw)
    w = [x.clone() for x in om.weights]
    for r in input_rows_of_state_dim(om.obs_process, obs - 1):
        w[0][:, r, :] *= g_in
    w[-1][:, :, 2 * om.out_size - 1] *= g_lv
    if om.learned_rewards:
        w[-1][:, :, om.out_size + obs - 1] *= g_lv
    return dataclasses.replace(om, weights=w), actions, s0, perms, eps


def mutated(om, which):
    """`om` as a kernel that lost one edge column would compute it: the last input row of layer 0 ("in_row"), the last hidden row of
    layer 1 ("hid_row": None where layer 1 is the output layer), the last mean ("mean_col") or log-variance ("lv_col") column zeroed."""
    w = [x.clone() for x in om.weights]
    b = [x.clone() for x in om.biases]
    out = om.out_size
    if which == "in_row":
        w[0][:, -1, :] = 0
    elif which == "hid_row":
        if len(w) < 3:
            return None
        w[1][:, -1, :] = 0
    else:
        col = out - 1 if which == "mean_col" else 2 * out - 1
        w[-1][:, :, col] = 0
        b[-1][:, :, col] = 0
    return dataclasses.replace(om, weights=w, biases=b)


def _members_forward_restated(rounded, acc64, nudge=0):
    """_members_forward with the operands of every matmul rounded to bf16 (`rounded`) and / or the products accumulated in f64 and
    rounded to fp32 once (`acc64`): the same restatement under another summation order.  nudge: every activation is moved by that
    many fp32 ulps (x (1 + nudge 2^-23)) before it is rounded to bf16 -- the values within `nudge` ulps of a bf16 rounding boundary
    land on its other side, as they may on a device whose elementwise functions differ from torch's by a few ulps."""
    def forward(m, x):
        el = m.active_members
        act = po._ACT[m.activation]
        h = x
        nl = len(m.weights)
        for li in range(nl):
            w = m.weights[li][el, ...]
            a = h
            if nudge:
                a = (a.double() * (1 + nudge * 2.0 ** -23)).float()
            if rounded:
                a, w = a.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
            h = (a.double().matmul(w.double()).float() if acc64 else a.matmul(w)) + m.biases[li][el, ...]
            if li < nl - 1:
                h = act(h)
        out = m.out_size
        logvar = m.max_logvar - F.softplus(m.max_logvar - h[..., out:])
        return h[..., :out], m.min_logvar + F.softplus(logvar - m.min_logvar)
    return forward


def reference_rollout(monkeypatch, prec, om, actions, s0, P, acc64=False, nudge=0, **kw):
    """The reference of precision `prec`: the bf16 emulation for "bf16", the fp32 oracle for "bf16x3"; acc64: its f64-accumulated twin;
    nudge: its twin with every activation moved by that many fp32 ulps before the bf16 rounding."""
    if prec == "bf16x3" and not acc64 and not nudge:
        return po.rollout(om, actions, s0, P, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(po, "_members_forward", _members_forward_restated(prec == "bf16", acc64, nudge) if acc64 or nudge else members_forward_bf16)
        return po.rollout(om, actions, s0, P, **kw)


def cpu_draws(om, pop, P, H, mode, row_tiles=3):
    """oracle kwargs of a (SEED, SID) rollout from the CPU restatements of the in-kernel draws at `row_tiles` row tiles per workgroup
    (the FAST member schedule is per workgroup; the bf16 / bf16x3 instances run three in both modes)."""
    B, M = pop * P, len(om.active_members)
    kw = dict(eps=torch.from_numpy(device_draws.fast_normals(H, B, om.out_size, SEED, SID)))
    if mode == "device":
        kw["perms"] = torch.stack([torch.from_numpy(feistel_perm.permutation(B, SEED, SID, t).astype(np.int64)) for t in range(H)])
    else:
        sched = torch.from_numpy(device_draws.member_schedule(H, device_draws.fast_workgroups(B, row_tiles), M, SEED, SID))
        wg = torch.as_tensor(np.asarray(device_draws.fast_row_workgroup(torch.arange(B), P, row_tiles))).long()
        kw["members"] = torch.stack([sched[t].long()[wg] for t in range(H)])
    return kw


def tolerance(prec, ref, D):
    """bf16: max(T2 of the emulation, D / 4) (tests/test_gpu_bf16.py); bf16x3: T2 of the fp32 oracle (tests/test_gpu_bf16x3.py)."""
    t2 = T2_REL * torch.clamp(ref.abs(), min=1.0)
    return torch.maximum(t2, torch.tensor(D / 4)) if prec == "bf16" else t2


def threshold_margin(om, trace):
    """smallest distance of a traced next state from a threshold of the model's termination function (tests/test_gpu_closed_forms.py
    threshold_margin lists them): humanoid heights 1.0 / 2.0; cartpole |x| 2.4, |theta| 12 degrees; inverted_pendulum |dim 1| 0.2; hopper
    height 0.7, |angle| 0.2, |dims 1..| 100.  inf for models without one of these termination functions."""
    if om.termination not in ("humanoid", "cartpole", "inverted_pendulum", "hopper"):
        return float("inf")
    n = torch.stack(trace["next_obs"])
    if om.termination == "humanoid":
        z = n[..., 0]
        return torch.minimum((z - 1.0).abs(), (z - 2.0).abs()).min().item()
    if om.termination == "cartpole":
        return torch.minimum((n[..., 0].abs() - 2.4).abs(), (n[..., 2].abs() - 12 * 2 * np.pi / 360).abs()).min().item()
    if om.termination == "inverted_pendulum":
        return (n[..., 1].abs() - 0.2).abs().min().item()
    return min((n[..., 0] - 0.7).abs().min().item(), (n[..., 1].abs() - 0.2).abs().min().item(), (n[..., 1:].abs() - 100.0).abs().min().item())


def edge_figures(monkeypatch, case, prec, mode, draws=None):
    """The CPU conditions of one edge case against the reference of `prec`, on the draws of `mode`: power (per mutation, the largest
    |mutated - clean| / tol over candidates), spread (the largest |ref - f64-accumulated ref| / tol), D = max |emu - f32|, told (the
    largest |emu - f32| / T2 tolerance), margin (threshold_margin of the reference), finite, and for bf16 flip: per nudge of
    NUDGES fp32 ulps the largest |ref - nudged ref| / tol (bf16x3 carries every fp32 bit: nothing to flip, empty)."""
    om, actions, s0, _, _ = edge_case(case.obs, case.act, case.pop, case.P, case.H, seed=case.seed, gain=case.gain, g_in=case.g_in,
                                      g_lv=case.g_lv, **case.mkw)
    kw = draws if draws is not None else cpu_draws(om, case.pop, case.P, case.H, mode)
    tr = {}
    ref = reference_rollout(monkeypatch, prec, om, actions, s0, case.P, trace=tr, **kw)
    f32 = po.rollout(om, actions, s0, case.P, **kw)
    emu = ref if prec == "bf16" else reference_rollout(monkeypatch, "bf16", om, actions, s0, case.P, **kw)
    D = (emu - f32).abs().max().item()
    tol = tolerance(prec, ref, D)
    power = {}
    for which in MUTATIONS:
        mut = mutated(om, which)
        if mut is not None:
            power[which] = ((reference_rollout(monkeypatch, prec, mut, actions, s0, case.P, **kw) - ref).abs() / tol).max().item()
    spread = ((reference_rollout(monkeypatch, prec, om, actions, s0, case.P, acc64=True, **kw) - ref).abs() / tol).max().item()
    told = ((emu - f32).abs() / (T2_REL * torch.clamp(f32.abs(), min=1.0))).max().item()
    flip = {}
    if prec == "bf16":
        flip = {k: ((reference_rollout(monkeypatch, prec, om, actions, s0, case.P, nudge=k, **kw) - ref).abs() / tol).max().item() for k in NUDGES}
    return dict(power=power, spread=spread, flip=flip, D=D, told=told, margin=threshold_margin(om, tr), finite=bool(torch.isfinite(ref).all()))


EdgeCase = collections.namedtuple("EdgeCase", "name obs act mkw pop P H seed gain g_in g_lv")
_A = dict(ensemble_size=5, hid=200)
_B = dict(ensemble_size=5, hid=200, termination="humanoid")


def _case(name, obs, act, mkw, seed, gain, g_in, g_lv, pop=40):
    return EdgeCase(name, obs, act, mkw, pop, 5, 4, seed, gain, g_in, g_lv)


# name, obs, act, model kwargs, (seed, gain, g_in, g_lv) -- all pop 40 x P 5, H 4 but the two single-candidate cases.  Seed and gains
# come from a search over seeds 0..47 x (g_in, g_lv) in {16/8, 8/4, 32/8, 16/4, 4/4, 8/8, 4/8} x gain in {2, 3} for a triple at which
# every CPU condition of tests/test_bf16_host.py holds for both precisions and both launch modes.  (A first table, chosen without the
# flip condition (e), put A_in65 at seed 0, 16/8: the bf16 kernel agreed with the emulation to 1e-5 over the first two steps and left
# it at ONE candidate in step 3 -- 3.1e-4, then 3.5e-3 = 1.7 tol after step 4, the rollout's own amplification; on the CPU a one-ulp
# nudge of the activations before their bf16 rounding moves that case by 0.87 tol.  With g_in on one input row, one bf16 flip of
# that input is worth about a tolerance: hence (e), and gains no larger than the power condition needs.)
EDGE_CASES = [
    # family A: X(13, 3, HALFCHEETAH, NONE) -- obs 17..24, no termination
    _case("A_in18", 17, 1, _A, 1, 2.0, 4.0, 8.0),      # in 18; 14 padding columns in the third output tile
    _case("A_in32", 24, 8, _A, 2, 2.0, 4.0, 4.0),       # in 32: one full k chunk; output tiles exactly full
    _case("A_in33", 24, 9, _A, 1, 2.0, 8.0, 4.0),       # in 33: one column in the second chunk
    _case("A_in64", 17, 47, _A, 3, 2.0, 4.0, 8.0),     # in 64: two full chunks
    _case("A_in65", 20, 45, _A, 3, 2.0, 32.0, 8.0),     # in 65: three chunks
    _case("A_in97", 24, 73, _A, 41, 2.0, 16.0, 4.0),     # in 97: four chunks -- the whole kBf16Ahead ring, no refill
    _case("A_in129", 24, 105, _A, 10, 2.0, 32.0, 8.0),   # in 129: five chunks -- the first ring refill
    _case("A_hid193", 17, 6, dict(_A, hid=193), 8, 2.0, 16.0, 8.0),   # lower hidden-width edge
    _case("A_hid208", 24, 6, dict(_A, hid=208), 0, 2.0, 4.0, 8.0),    # upper hidden-width edge
    _case("A_depth1", 17, 6, dict(_A, num_layers=1), 0, 2.0, 8.0, 8.0),  # two linear layers: no hidden -> hidden one
    _case("A_depth7", 24, 9, dict(_A, num_layers=7), 2, 2.0, 16.0, 8.0),  # eight linear layers
    _case("A_subset", 24, 9, dict(ensemble_size=7, hid=200, elite=[0, 2, 3, 5, 6]), 4, 2.0, 4.0, 4.0),  # non-prefix member subset
    _case("A_pop1", 24, 9, _A, 0, 2.0, 16.0, 8.0, pop=1),  # five rows: a single ragged tile
    # the gained variant of tests/test_gpu_bf16x3.py's small case (17, 6, 7, 5, 4), whose stock weights give the four mutations a power
    # of 3.0 / 1.9 / 0.01 / 0.00 (DEVICE) and 1.7 / 1.6 / 0.01 / 0.00 (FAST) of T2: 35 rows, seven per member
    _case("A_pop7", 17, 6, _A, 0, 2.0, 4.0, 4.0, pop=7),
    # family B: X(13, 6, HALFCHEETAH, HUMANOID) -- obs 41..48, humanoid termination
    _case("B_in42", 41, 1, _B, 3, 3.0, 16.0, 8.0),
    _case("B_in64", 48, 16, _B, 4, 2.0, 8.0, 8.0),     # in 64; output tiles exactly full
    _case("B_in65", 48, 17, _B, 2, 2.0, 32.0, 8.0),
    _case("B_in97", 41, 56, _B, 5, 3.0, 32.0, 8.0),
    _case("B_pop1", 48, 17, _B, 2, 2.0, 16.0, 8.0, pop=1),
]
# bf16x3 rows are three bf16 planes wide (1360 bytes against 464): at three row tiles the two activation buffers take 130 560 of the
# 163 840 bytes of LDS, and the double-buffered actions (2 x 48 x act_dim floats) fit up to act_dim 64 at obs 24 and 55 at obs 41
# (csrc/rollout_smem.hpp rollout_smem_bytes).  The mode has no other instance, so wider models are refused (B3_TOO_WIDE, the refusal
# tests); the four-chunk cases run at the widest act_dim that fits, i.e. with three input chunks, and the five-chunk case has no
# bf16x3 counterpart (its k loop keeps two fragment sets, not a ring: chunk counts 1, 2 and 3 cover its prologue, body and tail).
_B3_WIDEST = {"A_in97": _case("A_in88", 24, 64, _A, 0, 2.0, 16.0, 8.0), "B_in97": _case("B_in96", 41, 55, _B, 0, 2.0, 16.0, 8.0)}
EDGE_CASES_B3 = [_B3_WIDEST.get(c.name, c) for c in EDGE_CASES if c.name != "A_in129"]
B3_TOO_WIDE = [(24, 65, _A), (24, 105, _A), (41, 56, _B)]  # (obs, act, model kwargs): one more action column than fits, and the bf16 cases' widths
CASES_OF = {"bf16": EDGE_CASES, "bf16x3": EDGE_CASES_B3}

# CPU figures of the table (tests/test_bf16_host.py asserts them; draws of (SEED, SID), oracle/device_draws.py).  Per launch mode:
# power = the smallest over the mutations of max |mutated - clean| / tol (>= 4), spread = max |ref - f64-accumulated ref| / tol
# (<= 0.25), flip = max |ref - nudged ref| / tol over nudges of +-1, +-2 ulps (bf16: <= 0.5), D = max |emu - f32|, told = max |emu - f32|
# / T2 (bf16: >= 4), margin = distance of the nearest height from 1.0 / 2.0.
#   mode    case      seed gain g_in/g_lv | DEVICE power spread flip D told margin | FAST power spread flip D told margin
#   bf16    A_in18    1 2 4/8 |     8.2  0.149  0.41  2.00e-03   20.0      inf |    12.6  0.034  0.26  2.14e-03   21.4      inf
#   bf16    A_in32    2 2 4/4 |    13.7  0.205  0.33  1.20e-03    9.5      inf |    27.5  0.097  0.44  1.19e-03    7.3      inf
#   bf16    A_in33    1 2 8/4 |    15.9  0.089  0.42  3.04e-03   23.4      inf |    26.7  0.060  0.27  2.42e-03   16.8      inf
#   bf16    A_in64    3 2 4/8 |     5.6  0.107  0.32  1.21e-03    6.7      inf |     4.8  0.090  0.32  2.32e-03    8.1      inf
#   bf16    A_in65    3 2 32/8 |     4.4  0.064  0.42  3.95e-02  213.4      inf |     4.7  0.127  0.20  4.53e-02  208.4      inf
#   bf16    A_in97    41 2 16/4 |    17.6  0.230  0.27  6.74e-03   12.3      inf |     9.6  0.191  0.38  1.17e-02    9.2      inf
#   bf16    A_in129   10 2 32/8 |    15.7  0.058  0.35  1.14e-02    7.1      inf |    19.1  0.115  0.34  9.78e-03    5.7      inf
#   bf16    A_hid193  8 2 16/8 |    11.8  0.024  0.28  1.98e-02  197.8      inf |     8.7  0.044  0.20  2.39e-02  130.6      inf
#   bf16    A_hid208  0 2 4/8 |    25.4  0.039  0.44  2.15e-03   21.5      inf |    18.6  0.022  0.38  2.62e-03   16.5      inf
#   bf16    A_depth1  0 2 8/8 |    64.8  0.003  0.15  4.21e-02  326.2      inf |    75.4  0.088  0.12  4.00e-02  171.9      inf
#   bf16    A_depth7  2 2 16/8 |    11.8  0.217  0.41  9.88e-04    7.4      inf |     5.6  0.207  0.46  8.26e-04    8.1      inf
#   bf16    A_subset  4 2 4/4 |     9.7  0.216  0.22  1.23e-03   11.9      inf |    15.8  0.100  0.26  1.54e-03    7.2      inf
#   bf16    A_pop1    0 2 16/8 |    14.6  0.000  0.00  8.07e-04    4.3      inf |     4.6  0.000  0.00  3.04e-03   16.6      inf
#   bf16    A_pop7    0 2 4/4 |    10.5  0.004  0.19  2.15e-03   15.0      inf |     8.1  0.114  0.18  2.07e-03   15.0      inf
#   bf16    B_in42    3 3 16/8 |     6.7  0.003  0.03  1.29e+00 9841.2  5.4e-04 |   133.0  0.015  0.33  2.57e-02   72.4  5.4e-04
#   bf16    B_in64    4 2 8/8 |    24.0  0.014  0.31  2.03e-03    8.2  1.8e-03 |   156.1  0.009  0.15  2.35e-03   11.5  1.9e-04
#   bf16    B_in65    2 2 32/8 |    11.8  0.001  0.49  4.10e-03   16.1  9.8e-04 |    12.8  0.230  0.13  3.44e-03   34.4  9.8e-04
#   bf16    B_in97    5 3 32/8 |    38.2  0.007  0.04  5.00e-01 4254.3  2.2e-03 |    12.1  0.000  0.03  6.79e-01 6787.3  2.2e-03
#   bf16    B_pop1    2 2 16/8 |     9.3  0.001  0.00  7.56e-04    5.6  4.4e-02 |    10.4  0.000  0.00  6.48e-04    4.2  3.7e-02
#   bf16x3  A_in18    1 2 4/8 |    37.4  0.004  0.00  2.00e-03   20.0      inf |    61.6  0.006  0.00  2.14e-03   21.4      inf
#   bf16x3  A_in32    2 2 4/4 |    17.9  0.003  0.00  1.20e-03    9.5      inf |    60.7  0.004  0.00  1.19e-03    7.3      inf
#   bf16x3  A_in33    1 2 8/4 |    64.2  0.006  0.00  3.04e-03   23.4      inf |    88.9  0.004  0.00  2.42e-03   16.8      inf
#   bf16x3  A_in64    3 2 4/8 |    11.6  0.003  0.00  1.21e-03    6.7      inf |    16.4  0.002  0.00  2.32e-03    8.1      inf
#   bf16x3  A_in65    3 2 32/8 |   262.4  0.009  0.00  3.95e-02  213.4      inf |   359.0  0.011  0.00  4.53e-02  208.4      inf
#   bf16x3  A_in88    0 2 16/8 |    86.4  0.001  0.00  5.91e-03    6.2      inf |    75.9  0.002  0.00  6.47e-03    9.9      inf
#   bf16x3  A_hid193  8 2 16/8 |   238.0  0.005  0.00  1.98e-02  197.8      inf |   431.4  0.008  0.00  2.39e-02  130.6      inf
#   bf16x3  A_hid208  0 2 4/8 |    68.9  0.004  0.00  2.15e-03   21.5      inf |   108.4  0.004  0.00  2.62e-03   16.5      inf
#   bf16x3  A_depth1  0 2 8/8 |  3730.1  0.027  0.00  4.21e-02  326.2      inf |  2171.7  0.014  0.00  4.00e-02  171.9      inf
#   bf16x3  A_depth7  2 2 16/8 |    21.0  0.001  0.00  9.88e-04    7.4      inf |     7.0  0.002  0.00  8.26e-04    8.1      inf
#   bf16x3  A_subset  4 2 4/4 |    31.6  0.003  0.00  1.23e-03   11.9      inf |    58.1  0.003  0.00  1.54e-03    7.2      inf
#   bf16x3  A_pop1    0 2 16/8 |    11.6  0.000  0.00  8.07e-04    4.3      inf |    25.3  0.000  0.00  3.04e-03   16.6      inf
#   bf16x3  A_pop7    0 2 4/4 |    53.5  0.002  0.00  2.15e-03   15.0      inf |    34.3  0.002  0.00  2.07e-03   15.0      inf
#   bf16x3  B_in42    3 3 16/8 |  4555.3  0.019  0.00  1.29e+00 9841.2  5.5e-04 |  4216.0  0.013  0.00  2.57e-02   72.4  6.7e-04
#   bf16x3  B_in64    4 2 8/8 |    53.4  0.002  0.00  2.03e-03    8.2  2.4e-03 |   919.4  0.003  0.00  2.35e-03   11.5  1.9e-04
#   bf16x3  B_in65    2 2 32/8 |    79.6  0.002  0.00  4.10e-03   16.1  9.9e-04 |    91.5  0.002  0.00  3.44e-03   34.4  9.9e-04
#   bf16x3  B_in96    0 2 16/8 |    23.5  0.002  0.00  6.52e-04    6.5  2.0e-03 |    21.5  0.001  0.00  8.45e-04    8.4  3.5e-04
#   bf16x3  B_pop1    2 2 16/8 |    14.6  0.000  0.00  7.56e-04    5.6  4.4e-02 |    10.3  0.000  0.00  6.48e-04    4.2  3.7e-02
