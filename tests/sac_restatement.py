"""TEST HELPER (not collected): our own restatement of one SAC update (mbrl/third_party/pytorch_sac_pranz24/sac.py:76-173 with
model.py's GaussianPolicy / QNetwork) from explicit weight arrays in torch autograd, in the reference's op order, in float32 or
float64 (the dtype of the arrays it is given), with torch.optim.Adam written out by hand (train_restatement.adam_), each of the three
optimizers with its own settings, step count and (for a resumed run) starting moments;

plus a small SAC-shaped agent (TinySAC: the attributes hipets.SACUpdater reads, and a stock-torch ``update_parameters`` over
torch.optim.Adam) so that the GPU tests run where mbrl is not installed, the shared cases, and the condition every case's inputs
must meet (``check_kinks``): a kink -- a ReLU, min(q1, q2), the log_std clamp -- must not hide an error or fake one.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import train_restatement as tr

POLICY = ("pw1", "pb1", "pw2", "pb2", "pwm", "pbm", "pws", "pbs")
CRITIC = tuple(f"c{k}{i}" for i in range(1, 7) for k in "wb")  # cw1, cb1, .. cw6, cb6 (1-3 = Q1, 4-6 = Q2)
TARGET = tuple("t" + n[1:] for n in CRITIC)
MOMENTS = POLICY + CRITIC + ("log_alpha",)  # the trained tensors: what has Adam moments
LOG_SIG_MIN, LOG_SIG_MAX, EPSILON = -20.0, 2.0, 1e-6
HP = dict(gamma=0.99, tau=0.005, lr=3e-4, alpha=0.2, betas=(0.9, 0.999), eps=1e-8)
KINK_MARGIN = 1e-4
# A starting optimizer state spreads its elements' moment scales over this many decades below the gradient's rms (start_state).  All at
# one scale, sqrt(v) >> eps everywhere and exchanging two optimizers' eps (1e-8 / 1e-7) moves no parameter by the 1e-7 floor of
# train_restatement.check; a trained network holds quiet units whose moments have decayed, and there eps decides the step.
START_DECADES = 4.0


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def policy_sample(p, x, eps, scale, bias, rec=None):
    """GaussianPolicy.sample (model.py:88-108): (action, log_prob [B, 1]); ``rec`` collects the kinks' arguments"""
    z1 = F.linear(x, p["pw1"], p["pb1"])
    z2 = F.linear(F.relu(z1), p["pw2"], p["pb2"])
    h2 = F.relu(z2)
    mean = F.linear(h2, p["pwm"], p["pbm"])
    raw = F.linear(h2, p["pws"], p["pbs"])
    log_std = torch.clamp(raw, min=LOG_SIG_MIN, max=LOG_SIG_MAX)
    std = log_std.exp()
    x_t = mean + eps * std  # Normal.rsample
    y_t = torch.tanh(x_t)
    action = y_t * scale + bias
    log_prob = -((x_t - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))  # Normal.log_prob
    log_prob = log_prob - torch.log(scale * (1 - y_t.pow(2)) + EPSILON)
    if rec is not None:
        rec["relu"] += [z1.detach(), z2.detach()]
        rec["clamp"].append(raw.detach())
    return action, log_prob.sum(1, keepdim=True)


def q_forward(p, names, state, action, rec=None):
    """QNetwork.forward (model.py:50-63) over the parameters ``names`` (CRITIC or TARGET)"""
    xu = torch.cat([state, action], 1)
    out = []
    for j in (0, 6):
        z1 = F.linear(xu, p[names[j]], p[names[j + 1]])
        z2 = F.linear(F.relu(z1), p[names[j + 2]], p[names[j + 3]])
        out.append(F.linear(F.relu(z2), p[names[j + 4]], p[names[j + 5]]))
        if rec is not None:
            rec["relu"] += [z1.detach(), z2.detach()]
    return out


OPTIMIZERS = ("critic", "policy", "alpha")


def adam_settings(adam=None, hp=HP):
    """{"critic" | "policy" | "alpha": {"lr", "betas", "eps"}}: ``hp``'s for every optimizer, overridden by what ``adam`` names"""
    out = {which: dict(lr=hp["lr"], betas=hp["betas"], eps=hp["eps"]) for which in OPTIMIZERS}
    for which, own in (adam or {}).items():
        out[which].update(own)
    return out


def _adam_group(st, names, grads, which, lr, hp):
    st["steps"][which] += 1
    for n, g in zip(names, grads):
        tr.adam_(st["p"][n], g, st["m"][n], st["v"][n], st["steps"][which], lr, betas=hp["betas"], eps=hp["eps"])


def update(st, batch, eps_next, eps_cur, updates, hp, interval=1, tuning=True, target_entropy=None, adam=None, lrs=None):
    """One update in place on ``st`` = {"p": parameters by name (+ "log_alpha"), "m" / "v": Adam moments, "steps": {"critic",
    "policy", "alpha"}, "alpha": the coefficient in use, "scale" / "bias": the action rescaling}.  ``batch`` = (state, action,
    next_state, reward [B, 1], mask [B, 1]) in st's dtype.  ``adam``: every optimizer's own settings (adam_settings; None = hp's for
    all three); ``lrs``: this update's learning rates (critic, policy, alpha) in place of the settings' (a scheduler).  Returns the
    results and taps, and under "kinks" the arguments of every kink of the update."""
    adam = adam_settings(hp=hp) if adam is None else adam
    lr = dict(zip(OPTIMIZERS, lrs)) if lrs is not None else {which: adam[which]["lr"] for which in OPTIMIZERS}
    p = st["p"]
    state, action, next_state, reward, mask = batch
    rec = {"relu": [], "clamp": [], "min": []}
    alpha = st["alpha"]
    with torch.no_grad():
        a2, lp2 = policy_sample(p, next_state, eps_next, st["scale"], st["bias"], rec)
        q1t, q2t = q_forward(p, TARGET, next_state, a2, rec)
        rec["min"].append(q1t - q2t)
        y = reward + mask * hp["gamma"] * (torch.min(q1t, q2t) - alpha * lp2)
    cp = {n: p[n].clone().requires_grad_(True) for n in CRITIC}
    q1, q2 = q_forward(cp, CRITIC, state, action, rec)
    l1, l2 = F.mse_loss(q1, y), F.mse_loss(q2, y)
    grads = torch.autograd.grad(l1 + l2, [cp[n] for n in CRITIC])
    with torch.no_grad():
        _adam_group(st, CRITIC, grads, "critic", lr["critic"], adam["critic"])
    pp = {n: p[n].clone().requires_grad_(True) for n in POLICY}
    pi, lp = policy_sample(pp, state, eps_cur, st["scale"], st["bias"], rec)
    q1p, q2p = q_forward(p, CRITIC, state, pi, rec)
    rec["min"].append((q1p - q2p).detach())
    policy_loss = (alpha * lp - torch.min(q1p, q2p)).mean()
    grads = torch.autograd.grad(policy_loss, [pp[n] for n in POLICY])
    with torch.no_grad():
        _adam_group(st, POLICY, grads, "policy", lr["policy"], adam["policy"])
        if tuning:
            la = p["log_alpha"].clone().requires_grad_(True)
            with torch.enable_grad():
                alpha_loss = -(la * (lp + target_entropy).detach()).mean()
                (g,) = torch.autograd.grad(alpha_loss, [la])
            _adam_group(st, ["log_alpha"], [g], "alpha", lr["alpha"], adam["alpha"])
            st["alpha"] = p["log_alpha"].exp()
            alpha_out = st["alpha"].reshape(())
        else:
            alpha_loss = torch.zeros((), dtype=state.dtype)
            alpha_out = torch.as_tensor(alpha, dtype=state.dtype).reshape(())
        if updates % interval == 0:
            for c, t in zip(CRITIC, TARGET):
                p[t].copy_(p[t] * (1.0 - hp["tau"]) + p[c] * hp["tau"])
    return dict(q1=q1.detach().reshape(-1), q2=q2.detach().reshape(-1), y=y.reshape(-1), log_pi_next=lp2.reshape(-1),
                log_pi=lp.detach().reshape(-1), losses=torch.stack([l1.detach(), l2.detach(), policy_loss.detach(), alpha_loss.detach().reshape(()),
                                                                    alpha_out.detach()]), kinks=rec)


def kink_report(rec):
    """(signs of every kink's argument as one flat bool tensor, the smallest distance of an argument to its kink)"""
    flags, margin = [], float("inf")
    for z in rec["relu"] + rec["min"]:
        flags.append((z > 0).reshape(-1))
        margin = min(margin, z.abs().min().item())
    for raw in rec["clamp"]:
        flags += [(raw < LOG_SIG_MIN).reshape(-1), (raw > LOG_SIG_MAX).reshape(-1)]
        margin = min(margin, (raw - LOG_SIG_MIN).abs().min().item(), (raw - LOG_SIG_MAX).abs().min().item())
    return torch.cat(flags), margin


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _uniform(g, shape, a):
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * a


def _layer(g, x, n_out, sigma):
    """A [n_out, in] layer over inputs ``x``.  sigma None: Xavier-uniform weights, N(0, 0.1) biases.  Otherwise the weights are scaled
    so that the products have standard deviation 0.05 over x and every unit's bias is +- sigma * 0.05: most units are on or off for
    all rows, a few pre-activations cross zero, and very few come close to it."""
    n_in = x.shape[1]
    w = _uniform(g, (n_out, n_in), math.sqrt(6.0 / (n_in + n_out)))
    if sigma is None:
        return w, torch.randn(n_out, generator=g, dtype=torch.float64) * 0.1
    z = x @ w.T
    w = w * (0.05 / max(z.std().item(), 1e-12)) if z.numel() > 1 else w
    sign = (torch.rand(n_out, generator=g, dtype=torch.float64) < 0.5).to(torch.float64) * 2 - 1
    return w, sign * 0.05 * sigma


def make_inputs(obs, act, hid, B, seed, n_updates=1, sigma=None, clamp=False, start_draws=None):
    """float64 parameters and ``n_updates`` batches with their normal tables for a shape; ``clamp``: log_std head biases past both
    bounds of the clamp on the first and the last action dim.  ``start_draws``: a dict that receives, per trained tensor, the unit
    draws of a starting optimizer state (start_state), drawn after everything else so that no other draw moves."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    batches = []
    for _ in range(n_updates):
        term = (torch.rand(B, 1, generator=g, dtype=torch.float64) < 0.2).to(torch.float64)
        batches.append(dict(state=rn(B, obs), action=_uniform(g, (B, act), 1.0), next_state=rn(B, obs), reward=rn(B, 1), terminated=term,
                            eps_next=rn(B, act), eps_cur=rn(B, act)))
    b0 = batches[0]
    p = {}
    p["pw1"], p["pb1"] = _layer(g, b0["state"], hid, sigma)
    h = F.relu(F.linear(b0["state"], p["pw1"], p["pb1"]))
    p["pw2"], p["pb2"] = _layer(g, h, hid, sigma)
    h = F.relu(F.linear(h, p["pw2"], p["pb2"]))
    p["pwm"], p["pbm"] = _layer(g, h, act, None)
    p["pws"], p["pbs"] = _layer(g, h, act, None)
    p["pbs"] = p["pbs"] - 1.0
    if clamp:
        p["pbs"][0] = 30.0
        p["pbs"][-1] = -45.0 if act > 1 else 30.0
    xu = torch.cat([b0["state"], b0["action"]], 1)
    for j in (1, 4):
        p[f"cw{j}"], p[f"cb{j}"] = _layer(g, xu, hid, sigma)
        h = F.relu(F.linear(xu, p[f"cw{j}"], p[f"cb{j}"]))
        p[f"cw{j + 1}"], p[f"cb{j + 1}"] = _layer(g, h, hid, sigma)
        h = F.relu(F.linear(h, p[f"cw{j + 1}"], p[f"cb{j + 1}"]))
        p[f"cw{j + 2}"], p[f"cb{j + 2}"] = _layer(g, h, 1, None)
    for c, t in zip(CRITIC, TARGET):  # a target that is near the critic, not on it
        p[t] = p[c] + (rn(*p[c].shape) * 0.05 * p[c].abs().mean() if c[1] == "w" else 0.0)
    p["log_alpha"] = torch.full((1,), math.log(0.3), dtype=torch.float64)
    scale = 0.5 + torch.rand(act, generator=g, dtype=torch.float64)
    bias = rn(act) * 0.1
    if start_draws is not None:
        for n in MOMENTS:
            start_draws[n] = (rn(*p[n].shape),) + tuple(torch.rand(*p[n].shape, generator=g, dtype=torch.float64) for _ in range(2))
    return p, batches, scale, bias


def fresh_state(p, scale, bias, dtype, device="cpu", alpha=HP["alpha"], start=None):
    """``start``: {"steps": the optimizers' step counts, "m" / "v": float64 moments by name} to resume from, instead of a new optimizer"""
    ps = {n: t.to(device, dtype).clone() for n, t in p.items()}
    if start is None:
        m, v = ({n: torch.zeros_like(ps[n]) for n in MOMENTS} for _ in range(2))
        steps = dict(critic=0, policy=0, alpha=0)
    else:
        m, v = ({n: start[k][n].to(device, dtype).clone() for n in MOMENTS} for k in ("m", "v"))
        steps = dict(start["steps"])
    return dict(p=ps, m=m, v=v, steps=steps, alpha=alpha, scale=scale.to(device, dtype), bias=bias.to(device, dtype))


def start_state(case, steps, draws):
    """A resumed optimizer state for ``case``: the step counts ``steps`` and, per trained tensor, moments at the scale of that tensor's
    gradient in the case's first update (g, taken from the float64 restatement of a new optimizer's first step, m = 0.1 g).  Per
    element s = rms(g) 10^(-START_DECADES U(0, 1)), exp_avg = s N(0, 1), exp_avg_sq = s^2 U(0.25, 1.25): strictly positive, and
    m / sqrt(v) of order one and not saturated in every element."""
    p, batches, scale, bias = case["inputs"]
    st = fresh_state(p, scale, bias, torch.float64)
    update(st, batch_tensors(batches[0], torch.float64), batches[0]["eps_next"], batches[0]["eps_cur"], case["first_update"], HP,
           interval=case["interval"], tuning=case["tuning"], target_entropy=case["target_entropy"])
    m, v = {}, {}
    for n in MOMENTS:
        g = st["m"][n] / (1.0 - HP["betas"][0])
        s = max(g.pow(2).mean().sqrt().item(), 1e-6) * 10.0 ** (-START_DECADES * draws[n][2])
        m[n], v[n] = draws[n][0] * s, (draws[n][1] + 0.25) * s ** 2
    return dict(steps=dict(steps), m=m, v=v)


def batch_tensors(b, dtype, reverse_mask=True):
    mask = 1.0 - b["terminated"] if reverse_mask else b["terminated"]
    return tuple(b[k].to(dtype) for k in ("state", "action", "next_state", "reward")) + (mask.to(dtype),)


def restate(case, dtype, eps=None, reverse_rows=False):
    """Every update of ``case`` in ``dtype``: (final state, [per-update outputs]).  ``eps``: [(eps_next, eps_cur)] per update in place
    of the case's own normal tables.  ``reverse_rows``: every batch in reverse row order -- the same update with every contraction
    over the batch (the weight gradients, the means) summed the other way round; per-row outputs come back in the case's order."""
    p, batches, scale, bias = case["inputs"]
    st = fresh_state(p, scale, bias, dtype, start=case["start"])
    adam, lrs = adam_settings(case["adam"]), case["lrs"]
    outs = []
    flip = (lambda t: t.flip(0)) if reverse_rows else (lambda t: t)
    for u, b in enumerate(batches):
        e_next, e_cur = eps[u] if eps is not None else (b["eps_next"], b["eps_cur"])
        out = update(st, tuple(flip(t) for t in batch_tensors(b, dtype)), flip(torch.as_tensor(e_next).to(dtype)), flip(torch.as_tensor(e_cur).to(dtype)),
                     case["first_update"] + u, HP, interval=case["interval"], tuning=case["tuning"], target_entropy=case["target_entropy"],
                     adam=adam, lrs=lrs[u] if lrs is not None else None)
        for k in ("q1", "q2", "y", "log_pi_next", "log_pi"):
            out[k] = flip(out[k])
        outs.append(out)
    return st, outs


def check_kinks(out32, out64, what):
    """The condition on a case's inputs: through every update the float32 and float64 restatements take the same ReLU masks, the same
    min(q1, q2) side and the same clamp flags, and no float64 argument lies closer to its kink than KINK_MARGIN."""
    for u, (a, b) in enumerate(zip(out32, out64)):
        f32, _ = kink_report(a["kinks"])
        f64, margin = kink_report(b["kinks"])
        assert torch.equal(f32, f64), f"{what}: update {u}: the float32 and float64 restatements take different sides of a kink"
        assert margin >= KINK_MARGIN, f"{what}: update {u}: an argument lies {margin:.3e} from its kink (< {KINK_MARGIN})"


# name -> (obs, act, hidden, B), seed, and how the hidden layers are built (make_inputs: sigma).  The seeds were searched so that
# check_kinks holds (tests/make_sac_update_golden.py --search prints them); build_case asserts it at every use.
CASES = {
    "s1_1_1_1": dict(shape=(1, 1, 1, 1), seed=0),
    "s5_2_15_15": dict(shape=(5, 2, 15, 15), seed=0),
    "s5_2_16_16": dict(shape=(5, 2, 16, 16), seed=1),
    "s17_6_17_17": dict(shape=(17, 6, 17, 17), seed=0),
    "s23_6_72_33": dict(shape=(23, 6, 72, 33), seed=1, sigma=3.0),
    "s17_6_256_256": dict(shape=(17, 6, 256, 256), seed=0, sigma=5.0),
    "s17_6_512_256": dict(shape=(17, 6, 512, 256), seed=0, sigma=5.0),
    "s376_17_1024_256": dict(shape=(376, 17, 1024, 256), seed=0, sigma=5.0),
    "s512_32_1024_17": dict(shape=(512, 32, 1024, 17), seed=0, sigma=5.0),
    "fixed_alpha": dict(shape=(5, 2, 16, 17), seed=0, tuning=False),
    "clamp": dict(shape=(5, 3, 16, 17), seed=2, clamp=True),
    "twenty_i1": dict(shape=(5, 2, 16, 17), seed=0, sigma=3.0, n_updates=20, interval=1),
    "twenty_i3": dict(shape=(5, 2, 16, 17), seed=0, sigma=3.0, n_updates=20, interval=3, first_update=1),
    # the batch's row stride W = 2 obs + act + 2 a multiple of 4 (16-byte loads of the state rows), batches past 256
    "s27_8_64_257": dict(shape=(27, 8, 64, 257), seed=25, sigma=3.0),   # W = 64: vector loads with a ragged tail (K = 27), 17 row tiles
    "s11_4_32_1024": dict(shape=(11, 4, 32, 1024), seed=0, sigma=5.0),  # W = 28, the largest batch
    "s3_4_20_273": dict(shape=(3, 4, 20, 273), seed=1, sigma=3.0),      # W = 12, K = 3 below one vector group
}
# three optimizers that share no number (the policy's beta1 <= 0.5 takes the other branch of Tensor.lerp_), resumed from non-zero
# moments at three different step counts, and a target entropy that is not -act
RESUMED_ADAM = dict(critic=dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8), policy=dict(lr=1e-3, betas=(0.3, 0.95), eps=1e-6),
                    alpha=dict(lr=5e-4, betas=(0.8, 0.99), eps=1e-7))
RESUMED_STEPS = dict(critic=7, policy=3, alpha=11)
_LRS = tuple(RESUMED_ADAM[which]["lr"] for which in ("critic", "policy", "alpha"))
CASES["resumed"] = dict(shape=(5, 2, 16, 17), seed=0, sigma=3.0, adam=RESUMED_ADAM, start_steps=RESUMED_STEPS, target_entropy=-1.25)
# ... and three updates from there, a scheduler halving the policy's learning rate before the third
CASES["resumed_three"] = dict(CASES["resumed"], seed=0, n_updates=3, interval=2, lrs=(_LRS, _LRS, (_LRS[0], 0.5 * _LRS[1], _LRS[2])))
ONE_UPDATE = [n for n in CASES if n.startswith("s")]
RECORDED = ("s1_1_1_1", "s5_2_15_15", "s5_2_16_16", "s17_6_17_17", "fixed_alpha", "clamp", "resumed")  # the cases tests/golden/sac_update_cases.npz holds
_BUILT = {}


def complete_case(name, spec):
    """``spec`` with every optional field at its default, its inputs and (with "start_steps") its starting optimizer state"""
    c = dict(spec)
    for key, default in (("sigma", None), ("clamp", False), ("tuning", True), ("n_updates", 1), ("interval", 1), ("first_update", 0),
                         ("adam", None), ("start_steps", None), ("lrs", None), ("target_entropy", -float(c["shape"][1]))):
        c.setdefault(key, default)
    c["name"] = name
    draws = {} if c["start_steps"] is not None else None
    c["inputs"] = make_inputs(*c["shape"], c["seed"], c["n_updates"], c["sigma"], c["clamp"], start_draws=draws)
    c["start"] = start_state(c, c["start_steps"], draws) if draws is not None else None
    return c


# every exchange of one per-optimizer quantity between two optimizers (a kernel that reads the policy's beta2 where the alpha
# optimizer's is meant computes the case with those two exchanged)
SWAPS = [(field, a, b) for field in ("lr", "beta1", "beta2", "eps", "step") for a, b in (("critic", "policy"), ("policy", "alpha"), ("critic", "alpha"))]


def swapped(case, field, a, b):
    """``case`` with ``field`` of the optimizers ``a`` and ``b`` exchanged"""
    adam = {which: dict(own, betas=list(own["betas"])) for which, own in adam_settings(case["adam"]).items()}
    start = dict(case["start"], steps=dict(case["start"]["steps"]))
    if field == "step":
        start["steps"][a], start["steps"][b] = start["steps"][b], start["steps"][a]
    elif field in ("beta1", "beta2"):
        i = int(field[-1]) - 1
        adam[a]["betas"][i], adam[b]["betas"][i] = adam[b]["betas"][i], adam[a]["betas"][i]
    else:
        adam[a][field], adam[b][field] = adam[b][field], adam[a][field]
    lrs = None
    if case["lrs"] is not None:  # (a schedule names its learning rates itself)
        order = {"lr": {a: b, b: a}}.get(field, {})
        lrs = [tuple(u[OPTIMIZERS.index(order.get(which, which))] for which in OPTIMIZERS) for u in case["lrs"]]
    return dict(case, adam=adam, start=start, lrs=lrs)


def allowance(f32, f64, f32_others=()):
    """What train_restatement.check allows between a kernel's result and ``f64``"""
    d_all = [tr.dist(f32, f64)] + [tr.dist(t, f64) for t in f32_others]
    d_32 = max(d_all) if max(d_all) > 4 * min(d_all) + 1e-7 else d_all[0]
    return 4 * d_32 + 1e-7


def swap_separation(case, field, a, b):
    """(what, ratio): over every trained tensor's parameter and moments after the case's updates, the largest distance of the
    float64 restatement with the exchange from the one without, in units of train_restatement.check's allowance for that quantity.
    Kernels that make the exchange land within their own error of the exchanged result; that error is what the allowance bounds.
    So a ratio above 2 means check must refuse them on that quantity."""
    other, _ = restate(swapped(case, field, a, b), torch.float64)
    best = ("", 0.0)
    for kind in ("p", "m", "v"):
        for n in MOMENTS:
            ratio = tr.dist(other[kind][n], case["f64"][kind][n]) / allowance(case["f32"][kind][n], case["f64"][kind][n], [case["f32r"][kind][n]])
            best = max(best, (f"{kind} {n}", ratio), key=lambda t: t[1])
    return best


def build_case(name):
    """The case's inputs and both restatements, computed once per process and shared (nobody edits them)."""
    if name not in _BUILT:
        c = complete_case(name, CASES[name])
        c["f64"], c["out64"] = restate(c, torch.float64)
        c["f32"], c["out32"] = restate(c, torch.float32)
        c["f32r"], c["out32r"] = restate(c, torch.float32, reverse_rows=True)  # (train_restatement.check's f32_others)
        check_kinks(c["out32"], c["out64"], name)
        if c["start"] is not None:  # a condition on the case, like check_kinks: parity with it tells the optimizers' quantities apart
            c["swaps"] = {s: swap_separation(c, *s) for s in SWAPS}
            for s, (what, ratio) in c["swaps"].items():
                assert ratio > 2.0, f"{name}: exchanging {s[0]} of {s[1]} and {s[2]} moves nothing past twice the rule's allowance ({what}: {ratio:.2f}x)"
        _BUILT[name] = c
    return _BUILT[name]


# ---- a SAC-shaped agent ---------------------------------------------------------------------------------------------------------------
class TinyGaussianPolicy(torch.nn.Module):
    def __init__(self, obs, act, hid):
        super().__init__()
        self.linear1, self.linear2 = torch.nn.Linear(obs, hid), torch.nn.Linear(hid, hid)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(hid, act), torch.nn.Linear(hid, act)
        self.action_scale, self.action_bias = torch.ones(act), torch.zeros(act)

    def sample(self, state, eps=None):
        p = {"pw1": self.linear1.weight, "pb1": self.linear1.bias, "pw2": self.linear2.weight, "pb2": self.linear2.bias,
             "pwm": self.mean_linear.weight, "pbm": self.mean_linear.bias, "pws": self.log_std_linear.weight, "pbs": self.log_std_linear.bias}
        if eps is None:
            eps = torch.empty(state.shape[0], self.mean_linear.out_features, dtype=state.dtype, device=state.device).normal_()
        return policy_sample(p, state, eps, self.action_scale, self.action_bias)

    def to(self, device):
        self.action_scale, self.action_bias = self.action_scale.to(device), self.action_bias.to(device)
        return super().to(device)


class TinyQNetwork(torch.nn.Module):
    def __init__(self, obs, act, hid):
        super().__init__()
        for j in (1, 4):
            setattr(self, f"linear{j}", torch.nn.Linear(obs + act, hid))
            setattr(self, f"linear{j + 1}", torch.nn.Linear(hid, hid))
            setattr(self, f"linear{j + 2}", torch.nn.Linear(hid, 1))

    def forward(self, state, action):
        p = {f"c{k}{i}": getattr(getattr(self, f"linear{i}"), "weight" if k == "w" else "bias") for i in range(1, 7) for k in "wb"}
        return q_forward(p, CRITIC, state, action)


class TinySAC:
    """The attributes hipets.SACUpdater reads from a pytorch_sac_pranz24.SAC, and a stock-torch ``update_parameters`` over
    torch.optim.Adam in the order of sac.py:76-173 (the route an MBPO run takes without the update kernels)."""

    def __init__(self, obs, act, hid, device="cpu", tuning=True, lr=HP["lr"], interval=1, alpha=HP["alpha"], deterministic=False,
                 adam=None, target_entropy=None):
        """``adam``: per-optimizer settings (adam_settings), written into each optimizer's ``param_groups[0]``"""
        self.gamma, self.tau, self.alpha = HP["gamma"], HP["tau"], alpha
        self.target_update_interval, self.automatic_entropy_tuning, self.device = interval, tuning, torch.device(device)
        self.critic = TinyQNetwork(obs, act, hid).to(device)
        self.critic_target = TinyQNetwork(obs, act, hid).to(device)
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.critic_optim = torch.optim.Adam(self.critic.parameters(), lr=lr)
        if deterministic:  # (a DeterministicPolicy has one head, `mean`)
            self.policy = torch.nn.Module()
            self.policy.linear1, self.policy.linear2, self.policy.mean = torch.nn.Linear(obs, hid), torch.nn.Linear(hid, hid), torch.nn.Linear(hid, act)
            self.policy.to(device)
        else:
            self.policy = TinyGaussianPolicy(obs, act, hid).to(device)
        self.policy_optim = torch.optim.Adam(self.policy.parameters(), lr=lr)
        if tuning:
            self.target_entropy = -float(act) if target_entropy is None else float(target_entropy)
            self.log_alpha = torch.zeros(1, requires_grad=True, device=device)
            self.alpha_optim = torch.optim.Adam([self.log_alpha], lr=lr)
        for which, own in (adam or {}).items():
            if which != "alpha" or tuning:
                group = getattr(self, which + "_optim").param_groups[0]
                group["lr"], group["betas"], group["eps"] = own["lr"], tuple(own["betas"]), own["eps"]

    def load_start(self, start):
        """A starting optimizer state (start_state) into ``optimizer.state``, laid out as torch.optim.Adam._init_group lays it out:
        ``step`` a float scalar on the host, the moments float32 on the parameter's device"""
        live = self.params()
        for n in MOMENTS:
            if n == "log_alpha" and not self.automatic_entropy_tuning:
                continue
            which = "alpha" if n == "log_alpha" else ("policy" if n[0] == "p" else "critic")
            self.optimizer_of(n).state[live[n]] = dict(step=torch.tensor(float(start["steps"][which]), dtype=torch.float32),
                                                       exp_avg=start["m"][n].to(self.device, torch.float32).clone(),
                                                       exp_avg_sq=start["v"][n].to(self.device, torch.float32).clone())

    def load(self, p, scale, bias):
        """Parameters by restatement name (float64 arrays) into the modules"""
        with torch.no_grad():
            for n, t in p.items():
                if n == "log_alpha":
                    if self.automatic_entropy_tuning:
                        self.log_alpha.copy_(t)
                    continue
                net = {"p": self.policy, "c": self.critic, "t": self.critic_target}[n[0]]
                layer = {"1": "linear1", "2": "linear2", "m": "mean_linear", "s": "log_std_linear"}[n[2]] if n[0] == "p" else f"linear{n[2]}"
                getattr(getattr(net, layer), "weight" if n[1] == "w" else "bias").copy_(t)
            self.policy.action_scale = scale.to(self.device, torch.float32)
            self.policy.action_bias = bias.to(self.device, torch.float32)

    def params(self):
        """{restatement name: live tensor}"""
        out = {}
        for n in POLICY + CRITIC + TARGET:
            net = {"p": self.policy, "c": self.critic, "t": self.critic_target}[n[0]]
            layer = {"1": "linear1", "2": "linear2", "m": "mean_linear", "s": "log_std_linear"}[n[2]] if n[0] == "p" else f"linear{n[2]}"
            out[n] = getattr(getattr(net, layer), "weight" if n[1] == "w" else "bias")
        if self.automatic_entropy_tuning:
            out["log_alpha"] = self.log_alpha
        return out

    def optimizer_of(self, name):
        return self.alpha_optim if name == "log_alpha" else (self.policy_optim if name[0] == "p" else self.critic_optim)

    def update_parameters(self, memory, batch_size, updates, logger=None, reverse_mask=False):
        state, action, next_state, reward, mask, _ = memory.sample(batch_size).astuple()
        f = lambda v: torch.FloatTensor(np.asarray(v, dtype=np.float32)).to(self.device)  # noqa: E731
        state, action, next_state, reward, mask = f(state), f(action), f(next_state), f(reward).unsqueeze(1), f(mask).unsqueeze(1)
        if reverse_mask:
            mask = mask.logical_not()
        with torch.no_grad():
            a2, lp2 = self.policy.sample(next_state)
            q1t, q2t = self.critic_target(next_state, a2)
            y = reward + mask * self.gamma * (torch.min(q1t, q2t) - self.alpha * lp2)
        q1, q2 = self.critic(state, action)
        l1, l2 = F.mse_loss(q1, y), F.mse_loss(q2, y)
        self.critic_optim.zero_grad()
        (l1 + l2).backward()
        self.critic_optim.step()
        pi, lp = self.policy.sample(state)
        q1p, q2p = self.critic(state, pi)
        policy_loss = (self.alpha * lp - torch.min(q1p, q2p)).mean()
        self.policy_optim.zero_grad()
        policy_loss.backward()
        self.policy_optim.step()
        if self.automatic_entropy_tuning:
            alpha_loss = -(self.log_alpha * (lp + self.target_entropy).detach()).mean()
            self.alpha_optim.zero_grad()
            alpha_loss.backward()
            self.alpha_optim.step()
            self.alpha = self.log_alpha.exp()
            alpha_log = self.alpha.clone()
        else:
            alpha_loss, alpha_log = torch.tensor(0.0), torch.tensor(self.alpha)
        if updates % self.target_update_interval == 0:
            with torch.no_grad():
                for t, c in zip(self.critic_target.parameters(), self.critic.parameters()):
                    t.copy_(t * (1.0 - self.tau) + c * self.tau)
        return l1.item(), l2.item(), policy_loss.item(), alpha_loss.item(), alpha_log.item()


class FixedMemory:
    """A replay buffer whose ``sample`` hands out prepared batches in order (what the tests feed both routes)"""

    def __init__(self, batches):
        self.batches, self.next = list(batches), 0

    def sample(self, batch_size):
        b = self.batches[self.next % len(self.batches)]
        self.next += 1
        assert len(b["state"]) == batch_size
        tup = (b["state"].float().numpy(), b["action"].float().numpy(), b["next_state"].float().numpy(), b["reward"].float().numpy().reshape(-1),
               b["terminated"].numpy().reshape(-1) != 0, np.zeros(batch_size, dtype=bool))
        return SimpleNamespace(astuple=lambda: tup)

    def __len__(self):
        return 10 ** 6


def agent_for(case, device):
    """A TinySAC at the case's initial parameters on ``device`` and the memory that replays its batches"""
    obs, act, hid, _ = case["shape"]
    p, batches, scale, bias = case["inputs"]
    sac = TinySAC(obs, act, hid, device=device, tuning=case["tuning"], interval=case["interval"], adam=case["adam"],
                  target_entropy=case["target_entropy"])
    sac.load(p, scale, bias)
    if case["start"] is not None:
        sac.load_start(case["start"])
    return sac, FixedMemory(batches)
