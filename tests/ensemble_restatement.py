"""TEST INFRASTRUCTURE: restatements of what hipets/ensemble.py replaces, and the cases the ensemble tests share.

  model_input             OneDTransitionRewardModel._get_model_input (one_dim_tr_model.py:103-116): obs_process, cat, normaliser in its
                          own dtype, then float32 (float64 throughout with f64=True).
  ensemble_f64            GaussianMLP.forward(x, use_propagation=False) (gaussian_mlp.py:140-154) for the requested members and the four
                          statistics of hipets_ensemble_predict, in float64.  The GPU tests' reference.
  ensemble_f32_torch      the same through torch CPU float32: matmul, the activation module, F.softplus, torch.var(unbiased=False).  Pinned
                          to the reference's own classes by tests/golden/ensemble_predict_cases.npz (tests/make_ensemble_golden.py).
  naive_disagreement_f32  the one-pass E[x^2] - E[x]^2 form in float32, which the kernel must NOT use (the near-agreement claim).
  penalty_np              hipets_uncertainty_penalty in numpy float32, one rounded operation per line.
  GPU_CASES / make_case   the shapes of tests/test_gpu_ensemble.py, built from a generator seeded by the case's name; building a case
                          asserts its own premises (separation of the members, the clamp shares).
"""
import numpy as np

T1 = dict(rtol=1e-5, atol=2e-6)  # tests/policy_restatement.py
STATS = ("max_std", "disagreement", "total_std", "max_deviation")


def t1_share(got, ref64):
    """per element, the share of T1 that `got` uses against the float64 `ref64`"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref64) / (T1["atol"] + T1["rtol"] * np.abs(ref64))


def bound_factor(f32, f64):
    """the project's rule: max(1, 4 u), u the largest share of T1 the float32 torch restatement itself uses against float64"""
    return max(1.0, 4.0 * float(np.max(t1_share(f32, f64))))


# ---- the model input ----------------------------------------------------------------------------
def processed_obs(case, obs):
    cols = case.get("columns")
    if cols is None:
        return obs
    out = obs[:, [d for d, _ in cols]].copy()
    for k, (_, fn) in enumerate(cols):
        if fn == "sin":
            out[:, k] = np.sin(out[:, k])
        elif fn == "cos":
            out[:, k] = np.cos(out[:, k])
    return out


def model_input(case, obs, act, f64=False):
    """[B, in_dim]: float32 as the reference forms it (the normaliser's arithmetic in its own dtype), or float64 throughout"""
    obs = np.asarray(obs, dtype=np.float64 if f64 else np.float32)
    act = np.asarray(act, dtype=obs.dtype)
    x = np.concatenate([processed_obs(case, obs), act], axis=1)
    if case["normalizer"] == "none":
        return x
    dt = np.float64 if (f64 or case["normalizer"] == "f64") else np.float32
    x = (x.astype(dt) - case["norm_mean"].astype(dt)) / case["norm_std"].astype(dt)
    return x if f64 else x.astype(np.float32)


# ---- the forward ----------------------------------------------------------------------------------
def _act_np(name, z, slope):
    if name == "relu":
        return np.maximum(z, 0.0)
    if name == "silu":
        return z / (1.0 + np.exp(-z))
    if name == "leaky_relu":
        return np.where(z > 0, z, z * slope)
    if name == "tanh":
        return np.tanh(z)
    return 1.0 / (1.0 + np.exp(-z))


def _softplus64(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def member_list(case, only_elite):
    return list(case["elites"]) if (only_elite and case.get("elites") is not None) else list(range(case["E"]))


def raw_heads_f64(case, x, members, weights=None, biases=None):
    """the last layer's raw output [n, B, out_total] in float64"""
    ws = case["weights"] if weights is None else weights
    bs = case["biases"] if biases is None else biases
    h = np.broadcast_to(np.asarray(x, np.float64), (len(members),) + x.shape)
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w[members].astype(np.float64) + b[members].astype(np.float64)
        if l < len(ws) - 1:
            h = _act_np(case["activation"], h, case["slope"])
    return h


def _bounds(case, members, dtype):
    lo, hi = np.asarray(case["min_logvar"], dtype), np.asarray(case["max_logvar"], dtype)
    if lo.shape[0] > 1:  # every member owns its bounds
        return lo[members][:, None, :], hi[members][:, None, :]
    return lo[None], hi[None]


def statistics_f64(mean, logvar):
    n = mean.shape[0]
    var_m = mean.var(axis=0).sum(-1)
    ev = np.exp(logvar).sum(-1) if logvar is not None else np.zeros(mean.shape[:2])
    dev = np.sqrt(((mean - mean[:1]) ** 2).sum(-1))
    return np.stack([np.sqrt(ev).max(0), np.sqrt(var_m), np.sqrt(var_m + ev.sum(0) / n), dev.max(0)], axis=-1)


def ensemble_f64(case, x, only_elite=False):
    """(mean [n, B, out], logvar [n, B, out] | None, stats [B, 4]) in float64 from a model input `x` [B, in]"""
    members = member_list(case, only_elite)
    raw = raw_heads_f64(case, np.asarray(x, np.float64), members)
    out = case["out_dim"]
    if case["deterministic"]:
        return raw, None, statistics_f64(raw, None)
    mean, lv = raw[..., :out], raw[..., out:]
    lo, hi = _bounds(case, members, np.float64)
    lv = hi - _softplus64(hi - lv)
    lv = lo + _softplus64(lv - lo)
    return mean, lv, statistics_f64(mean, lv)


def ensemble_f32_torch(case, x, only_elite=False):
    """the same through torch CPU float32, op by op as the reference's modules run them"""
    import torch
    import torch.nn.functional as F

    members = member_list(case, only_elite)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    acts = {"relu": torch.relu, "silu": F.silu, "leaky_relu": lambda z: F.leaky_relu(z, case["slope"]), "tanh": torch.tanh, "sigmoid": torch.sigmoid}
    h = t(x)
    for l, (w, b) in enumerate(zip(case["weights"], case["biases"])):
        h = h.matmul(t(w[members])) + t(b[members])  # EnsembleLinearLayer.forward (models/util.py:54-65)
        if l < len(case["weights"]) - 1:
            h = acts[case["activation"]](h)
    out = case["out_dim"]
    if case["deterministic"]:
        mean, lv = h, None
    else:
        mean, lv = h[..., :out], h[..., out:]
        lo, hi = (t(a) for a in _bounds(case, members, np.float32))
        lv = hi - F.softplus(hi - lv)
        lv = lo + F.softplus(lv - lo)
    var_m = mean.var(dim=0, unbiased=False).sum(-1)
    ev = lv.exp().sum(-1) if lv is not None else torch.zeros(mean.shape[:2])
    dev = (mean - mean[:1]).pow(2).sum(-1).sqrt()
    stats = torch.stack([ev.sqrt().max(0).values, var_m.sqrt(), (var_m + ev.mean(0)).sqrt(), dev.max(0).values], dim=-1)
    return mean.numpy(), None if lv is None else lv.numpy(), stats.numpy()


def naive_disagreement_f32(mean):
    """sqrt(sum_d (E[x^2] - E[x]^2)) accumulated in float32 over the members in order: the form the kernel must not use"""
    mean = np.asarray(mean, np.float32)
    n = np.float32(mean.shape[0])
    s1 = np.zeros(mean.shape[1:], np.float32)
    s2 = np.zeros(mean.shape[1:], np.float32)
    for m in mean:
        s1 = s1 + m
        s2 = s2 + m * m
    var = s2 / n - (s1 / n) * (s1 / n)
    return np.sqrt(np.maximum(var.sum(-1, dtype=np.float32), np.float32(0)))


def shifted_disagreement_f32(mean):
    """the kernel's rule in float32: sums about the first member's mean"""
    mean = np.asarray(mean, np.float32)
    n = np.float32(mean.shape[0])
    d = mean - mean[:1]
    s1 = np.zeros(mean.shape[1:], np.float32)
    ssq = np.zeros(mean.shape[1], np.float32)
    for m in d:
        s1 = s1 + m
        ssq = ssq + (m * m).sum(-1, dtype=np.float32)
    t = s1 / n
    return np.sqrt(np.maximum(ssq / n - (t * t).sum(-1, dtype=np.float32), np.float32(0)))


# ---- the penalty ------------------------------------------------------------------------------------
def penalty_np(stats, stat, coef, rewards, dones, halt_threshold=None, halt_reward=None):
    """hipets_uncertainty_penalty: (rewards float32 [B], dones uint8 [B]) after the launch"""
    u = np.asarray(stats, np.float32)[:, stat]
    p = np.float32(coef) * u
    r = np.asarray(rewards, np.float32) - p
    d = np.asarray(dones).astype(np.uint8).copy()
    if halt_threshold is not None:
        with np.errstate(invalid="ignore"):
            halted = u > np.float32(halt_threshold)  # (a NaN u never halts)
        d[halted] = 1
        if halt_reward is not None:
            r = np.where(halted, np.float32(halt_reward), r)
    return r.astype(np.float32), d


# ---- the cases ----------------------------------------------------------------------------------------
# name -> E, obs, act, hid, linear layers, activation, learned reward, normaliser, rows; further keys per case below
GPU_CASES = {
    "small_silu": dict(E=3, obs=3, act=2, hid=20, layers=3, activation="silu", learned=True, normalizer="f64", rows=80),
    "exact16": dict(E=2, obs=8, act=8, hid=16, layers=3, activation="silu", learned=False, normalizer="none", rows=48),
    "stock": dict(E=7, obs=17, act=6, hid=200, layers=5, activation="silu", learned=True, normalizer="f64", rows=1000, elites=[5, 0, 3, 6, 2]),
    "head9tiles": dict(E=2, obs=70, act=2, hid=32, layers=3, activation="silu", learned=True, normalizer="f32", rows=40),
    "det_relu": dict(E=4, obs=5, act=2, hid=24, layers=3, activation="relu", learned=False, normalizer="none", rows=50, deterministic=True),
    "basic_tanh": dict(E=3, obs=4, act=2, hid=20, layers=3, activation="tanh", learned=False, normalizer="f32", rows=50, basic=True),
    "columns_f32": dict(E=3, obs=4, act=2, hid=20, layers=3, activation="leaky_relu", learned=False, normalizer="f32", rows=50,
                        columns=[(0, "id"), (1, "sin"), (1, "cos"), (2, "id"), (2, "id"), (3, "id")]),
    "columns_id": dict(E=2, obs=4, act=2, hid=20, layers=2, activation="sigmoid", learned=False, normalizer="f32", rows=50,
                       columns=[(3, "id"), (1, "id"), (1, "id"), (0, "id")]),
    "clamped": dict(E=3, obs=6, act=2, hid=24, layers=3, activation="silu", learned=True, normalizer="none", rows=64, clamp=True),
    "near_agree": dict(E=5, obs=17, act=6, hid=200, layers=5, activation="silu", learned=True, normalizer="none", rows=64, near=(1e-2, 5.0)),
    "humanoid_fit": dict(E=2, obs=376, act=17, hid=200, layers=5, activation="silu", learned=True, normalizer="f64", rows=40),
}


def _swap_moves_every_row(case, x):
    """exchanging members 0 and 1 in any single layer moves member 0's float64 mean by more than T1 on every row"""
    out = case["out_dim"]
    base = raw_heads_f64(case, x, [0])[0][:, :out]
    for l in range(len(case["weights"])):
        ws, bs = [w.copy() for w in case["weights"]], [b.copy() for b in case["biases"]]
        ws[l][[0, 1]] = ws[l][[1, 0]]
        bs[l][[0, 1]] = bs[l][[1, 0]]
        moved = raw_heads_f64(case, x, [0], ws, bs)[0][:, :out]
        if not (t1_share(moved, base).max(axis=1) > 1.0).all():
            return False
    return True


def make_case(name, near=None):
    """the arrays of a case (see the module docstring).  `near`: (relative perturbation, shift) in place of the case's own"""
    c = dict(GPU_CASES[name])
    rng = np.random.default_rng([ord(ch) for ch in name])
    E, obs, act, hid, L = c["E"], c["obs"], c["act"], c["hid"], c["layers"]
    det = bool(c.get("deterministic", False))
    out = obs + (1 if c["learned"] else 0)
    in_dim = (len(c["columns"]) if c.get("columns") else obs) + act
    dims = [in_dim] + [hid] * (L - 1) + [out if det else 2 * out]
    near = c.get("near") if near is None else near
    ws, bs = [], []
    for l in range(L):
        k, n = dims[l], dims[l + 1]
        if near:  # one shared draw, every member a small relative perturbation of it
            w0 = rng.standard_normal((1, k, n)) / np.sqrt(k)
            b0 = rng.uniform(-0.1, 0.1, (1, 1, n))
            w = w0 * (1.0 + near[0] * rng.standard_normal((E, k, n)))
            b = b0 * (1.0 + near[0] * rng.standard_normal((E, 1, n)))
            if l == L - 1:
                b[:, :, :out] += near[1]  # the shared shift of the mean columns
        else:
            w = rng.standard_normal((E, k, n)) / np.sqrt(k)
            b = rng.uniform(-0.1, 0.1, (E, 1, n))
        ws.append(w.astype(np.float32))
        bs.append(b.astype(np.float32))
    case = dict(name=name, E=E, obs_dim=obs, act_dim=act, in_dim=in_dim, out_dim=out, hid=hid, activation=c["activation"], slope=0.05,
                deterministic=det, learned_rewards=c["learned"], normalizer=c["normalizer"], columns=c.get("columns"), elites=c.get("elites"),
                basic=bool(c.get("basic", False)), weights=ws, biases=bs)
    if c["normalizer"] != "none":
        dt = np.float64 if c["normalizer"] == "f64" else np.float32
        case["norm_mean"] = rng.uniform(-0.5, 0.5, (1, in_dim)).astype(dt)
        case["norm_std"] = rng.uniform(0.5, 2.0, (1, in_dim)).astype(dt)
    case["obs"] = (1.5 * rng.standard_normal((c["rows"], obs))).astype(np.float32)
    case["act"] = rng.uniform(-1, 1, (c["rows"], act)).astype(np.float32)
    x64 = model_input(case, case["obs"], case["act"], f64=True)
    if not det:
        rows = E if case["basic"] else 1
        if c.get("clamp"):  # bounds at the 40th / 60th percentile of the raw log-variances, per column
            raw = raw_heads_f64(case, x64, list(range(E)))[..., out:].reshape(-1, out)
            lo, hi = np.percentile(raw, 40, axis=0)[None], np.percentile(raw, 60, axis=0)[None]
            case["min_logvar"], case["max_logvar"] = lo.astype(np.float32), hi.astype(np.float32)
            above, below = float((raw > case["max_logvar"]).mean()), float((raw < case["min_logvar"]).mean())
            assert 0.35 < above < 0.45 and 0.35 < below < 0.45, (above, below)
        else:  # (per-member rows differ by far more than T1)
            case["min_logvar"] = (-6.0 + rng.uniform(-1.5, 1.5, (rows, out))).astype(np.float32)
            case["max_logvar"] = (0.5 + rng.uniform(-0.4, 0.4, (rows, out))).astype(np.float32)
    assert _swap_moves_every_row(case, x64), f"{name}: members 0 and 1 are not separated in every layer"
    return case


def case_spec(case, **kw):
    """hipets.ModelSpec of a case (reward / termination are not read by the ensemble kernel)"""
    import torch

    import hipets

    t = torch.from_numpy
    cols = None if case["columns"] is None else hipets.ObsColumns(tuple(hipets.ObsColumn(d, fn) for d, fn in case["columns"]))
    return hipets.ModelSpec(
        weights=[t(w) for w in case["weights"]], biases=[t(b) for b in case["biases"]], obs_dim=case["obs_dim"], act_dim=case["act_dim"],
        min_logvar=None if case["deterministic"] else t(case["min_logvar"]), max_logvar=None if case["deterministic"] else t(case["max_logvar"]),
        elite_models=case["elites"], activation=case["activation"], leaky_slope=case["slope"], deterministic=case["deterministic"],
        norm_mean=t(case["norm_mean"]) if case["normalizer"] != "none" else None, norm_std=t(case["norm_std"]) if case["normalizer"] != "none" else None,
        learned_rewards=case["learned_rewards"], obs_process=cols if cols is not None else "none", reward=None if case["learned_rewards"] else "none",
        ensemble_kind="basic_ensemble" if case["basic"] else "gaussian_mlp", **kw)
