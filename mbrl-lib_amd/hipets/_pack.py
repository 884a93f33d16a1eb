"""The descriptors of include/hipets.h, packed from specs and tensors.  Pure functions: no library call and no device API, so that
every one of them runs in a host test (tests/test_engine_binding_host.py).  Each returns the filled struct and a keep-alive list: what
the struct points to and nothing else references, to be held until the library call that reads the struct has returned."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .model import BoxTermination, ModelSpec, ObsColumns, RewardTerms


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _check_dev(t: torch.Tensor, dtype, device, name: str, shape=None, numel=None):
    if not isinstance(t, torch.Tensor) or t.device != device:
        raise ValueError(f"{name} must be a tensor on {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} must have {numel} elements, got {t.numel()}")


def member_slots(members: torch.Tensor, n_members: int, device) -> tuple:
    """Row -> member map(s) ``members`` int64 [T, B] -> (slots int64 [T, M * rpm] on ``device``, rpm): slot m * rpm + j holds
    the j-th row (ascending) of member m, -1 pads the tail (hipets_rollout_opts.rows_per_member).  Pure index plumbing
    with torch ops on whichever device ``members`` lives: a CPU map gets the tight rpm = largest member count; a device
    map uses rpm = B so that no count has to travel to the host (all-padding workgroups exit immediately)."""
    T, B = members.shape
    members = members.to(torch.int64)
    counts = torch.zeros(T, n_members, dtype=torch.int64, device=members.device).scatter_add_(1, members, torch.ones_like(members))
    rpm = int(counts.max()) if members.device.type == "cpu" else B
    order = members.argsort(dim=1, stable=True)
    sorted_m = members.gather(1, order)
    starts = counts.cumsum(1) - counts
    pos = torch.arange(B, device=members.device).unsqueeze(0) - starts.gather(1, sorted_m)
    slots = torch.full((T, n_members * rpm), -1, dtype=torch.int64, device=members.device)
    slots.scatter_(1, sorted_m * rpm + pos, order)
    return slots.to(device).contiguous(), max(rpm, 1)


def pack_reward_terms(rt: RewardTerms):
    """The ``hipets_reward_term`` array of a table: ``level`` and ``op`` go into the upper bits of ``fn`` (``_lib.term_word``), so a
    plain term -- level 0, add -- packs to the bare fn code an ABI v9 client writes."""
    return (_lib.RewardTermC * max(1, len(rt.terms)))(*[
        _lib.RewardTermC(_lib.term_word(_lib.TERM_FN[t.fn], _lib.TERM_OP[t.op], t.level), _lib.TERM_SRC[t.source], int(t.i),
                         -1 if t.j is None else int(t.j), float(t.c), float(t.w))
        for t in rt.terms])


def pack_model_desc(spec: ModelSpec, ws, bs):
    """hipets_model_desc of ``spec`` over its converted (device, f32, contiguous) weights ``ws`` / biases ``bs`` -> (desc, the
    hipets_obs_column table of an ObsColumns model -- hipets_set_model_columns' own argument -- or None, keep-alive list)."""
    members, n = spec.members, len(ws)
    d = _lib.ModelDesc(obs_dim=spec.obs_dim, act_dim=spec.act_dim, in_dim=spec.in_dim, out_dim=spec.out_dim, hid=spec.hid, n_layers=n,
                       ensemble_size=spec.ensemble_size, n_members=len(members), activation=_lib.ACT[spec.activation],
                       leaky_slope=float(spec.leaky_slope), propagation=_lib.PROP[spec.propagation], deterministic=int(spec.deterministic),
                       target_is_delta=int(spec.target_is_delta), learned_rewards=int(spec.learned_rewards),
                       n_no_delta=len(spec.no_delta_list), ensemble_kind=_lib.ENSEMBLE[spec.ensemble_kind], precision=_lib.PREC[spec.precision])
    d.members = (C.c_int32 * len(members))(*members)
    d.no_delta = (C.c_int32 * max(1, len(spec.no_delta_list)))(*[int(i) for i in spec.no_delta_list])
    d.weights = (C.c_void_p * n)(*[w.data_ptr() for w in ws])
    d.biases = (C.c_void_p * n)(*[b.data_ptr() for b in bs])
    keep, cols = [ws, bs], None  # (the ctypes arrays assigned to pointer fields are referenced by the struct itself)
    if isinstance(spec.obs_process, ObsColumns):
        cols = (_lib.ObsColumnC * len(spec.obs_process.columns))(*[_lib.ObsColumnC(int(c.dim), _lib.COL_FN[c.fn]) for c in spec.obs_process.columns])
        d.obs_process = _lib.OBS["columns"]
    else:
        d.obs_process = _lib.OBS[spec.obs_process]
    if isinstance(spec.reward, RewardTerms):
        rt = spec.reward
        d.reward_fn, d.reward_terms, d.n_reward_terms = _lib.REW["terms"], pack_reward_terms(rt), len(rt.terms)
        d.reward_bias, d.alive_bonus = rt.bias, rt.alive_bonus
    else:
        d.reward_fn = _lib.REW[spec.reward]
    if isinstance(spec.termination, BoxTermination):
        box = spec.termination
        d.term_intervals = (_lib.TermIntervalC * max(1, len(box.intervals)))(*[
            _lib.TermIntervalC(int(iv.dim), (_lib.BOX_LO_OPEN if iv.lo_open else 0) | (_lib.BOX_HI_OPEN if iv.hi_open else 0), float(iv.lo), float(iv.hi))
            for iv in box.intervals])
        d.termination_fn, d.n_term_intervals, d.term_require_finite = _lib.TERM["box"], len(box.intervals), int(box.require_finite)
    else:
        d.termination_fn = _lib.TERM[spec.termination]

    def host(t, np_type, c_type):  # a HOST array behind a typed pointer
        arr = np.ascontiguousarray(t.numpy().reshape(-1), dtype=np_type)
        keep.append(arr)
        return arr.ctypes.data_as(C.POINTER(c_type))

    if spec.norm_mean is not None:
        d.normalizer = _lib.NORM["f64" if spec.norm_mean.dtype == torch.float64 else "f32"]
        d.norm_mean = host(spec.norm_mean.detach().cpu().double(), np.float64, C.c_double)
        d.norm_std = host(spec.norm_std.detach().cpu().double(), np.float64, C.c_double)
    else:
        d.normalizer = _lib.NORM["none"]
    if not spec.deterministic:
        lo, hi = spec.min_logvar.detach().cpu().float(), spec.max_logvar.detach().cpu().float()
        if spec.ensemble_kind == "basic_ensemble":  # every member owns its bounds: [M, out] (a shared [1, out] is broadcast)
            lo = lo.reshape(-1, spec.out_dim).expand(len(members), spec.out_dim)
            hi = hi.reshape(-1, spec.out_dim).expand(len(members), spec.out_dim)
        d.min_logvar, d.max_logvar = host(lo, np.float32, C.c_float), host(hi, np.float32, C.c_float)
    return d, cols, keep


def ensemble_lds_bytes(in_dim: int, hid: int, out_dim: int, deterministic: bool, n_layers: int, row_tiles: int = 1) -> int:
    """Dynamic LDS of a hipets_ensemble_predict workgroup of ``row_tiles`` row tiles (csrc/ensemble.hip ensemble_geo): per row the kept
    input (pad16(in) + 4 floats), the two activation buffers (pad16(hid) + 4 and max(pad16(hid), pad16(out_total)) + 4) and the two
    per-column accumulators (2 out_dim); ``n_layers`` does not enter (it only decides which buffer is the wide one)."""
    pad16 = lambda x: (int(x) + 15) // 16 * 16  # noqa: E731
    hp, npo = pad16(hid), pad16(out_dim if deterministic else 2 * out_dim)
    return 16 * 4 * (pad16(in_dim) + 4 + hp + 4 + max(hp, npo) + 4 + 2 * int(out_dim)) * int(row_tiles)


def policy_rollout_lds_bytes(obs_dim: int, act_dim: int, actor_hidden: int, in_dim: int, hid: int, out_dim: int, deterministic: bool, n_layers: int,
                             row_tiles: int = 1) -> int:
    """Dynamic LDS of a hipets_policy_rollout workgroup of ``row_tiles`` row tiles (csrc/policy_rollout.hip rollout_geo): per row the
    state (pad16(obs) + 4 floats), the action (act rounded up to 4) and the larger of the actor's two buffers (pad16(hidden) + 4 and
    max(pad16(hidden), pad16(2 act)) + 4) and the model's areas (the ensemble kernel's input and two buffers, and the members' sum:
    out_dim) -- the two networks never run at once and share that space."""
    pad16 = lambda x: (int(x) + 15) // 16 * 16  # noqa: E731
    hpa = pad16(actor_hidden)
    actor = hpa + 4 + max(hpa, pad16(2 * act_dim)) + 4
    model = ensemble_lds_bytes(in_dim, hid, out_dim, deterministic, n_layers) // 64 - int(out_dim)
    return 16 * 4 * (pad16(obs_dim) + 4 + (int(act_dim) + 3) // 4 * 4 + max(actor, model)) * int(row_tiles)


def check_ensemble_shape(spec: ModelSpec, lds_max: int = 160 * 1024):
    """What hipets_ensemble_set refuses, told without a device: raises UnsupportedModelError naming the reason (fp32 only, E <= 16,
    in_dim / out_dim <= 512, hid <= 1024, one row tile within ``lds_max`` bytes of LDS)."""
    from .model import UnsupportedModelError

    if spec.precision != "f32":
        raise UnsupportedModelError(f"ensemble predictions run in fp32 only: precision {spec.precision!r} has no ensemble kernel")
    for what, v, lim in (("ensemble_size", spec.ensemble_size, _lib.ENSEMBLE_MAX_MEMBERS), ("in_dim", spec.in_dim, _lib.ENSEMBLE_MAX_IN),
                         ("out_dim", spec.out_dim, _lib.ENSEMBLE_MAX_OUT), ("hidden width", spec.hid, _lib.POLICY_MAX_HIDDEN)):
        if v > lim:
            raise UnsupportedModelError(f"ensemble {what} {v} above {lim}")
    need = ensemble_lds_bytes(spec.in_dim, spec.hid, spec.out_dim, spec.deterministic, len(spec.weights))
    if need > lds_max:
        raise UnsupportedModelError(f"ensemble too wide for LDS: one row tile needs {need} bytes, the limit is {lds_max}")


def pack_planet_desc(spec, tensors):
    """hipets_planet_desc of a ``PlaNetSpec`` over its converted tensors (``_lib._PLANET_TENSORS`` order) -> (desc, keep-alive list)"""
    d = _lib.PlanetDesc(latent_size=spec.latent_size, action_size=spec.action_size, belief_size=spec.belief_size, hidden_size=spec.hidden_size,
                        min_std=float(spec.min_std), **{n: t.data_ptr() for n, t in zip(_lib._PLANET_TENSORS, tensors)})
    return d, list(tensors)


def pack_train_desc(device, weights, biases, activation: str, leaky_slope: float, out_dim: int, max_batch: int, adam=None, *,
                    loss: str = "nll", bounds_per_member: bool = False):
    """TrainDesc over the caller's DEVICE tensors (weights[l] [E, d_l, d_l+1], biases[l] [E, 1, d_l+1]); ``adam`` =
    (exp_avg_w, exp_avg_b, exp_avg_sq_w, exp_avg_sq_b, min_logvar, max_logvar, lr, beta1, beta2, eps, weight_decay,
    steps_per_launch).  The returned keep-alive list holds the ctypes arrays the struct points to.  ``loss`` "mse": the last
    layer is out_dim wide and the bounds may be None (NULL in the descriptor); ``bounds_per_member``: the bounds are [E, out_dim]."""
    if loss not in _lib.TRAIN_LOSS:
        raise ValueError(f"unknown loss {loss!r}")
    L = len(weights)
    if L < 2 or L != len(biases):
        raise ValueError("weights / biases: one tensor of each per linear layer, at least 2 layers")
    E, in_dim, hid = int(weights[0].shape[0]), int(weights[0].shape[1]), int(weights[0].shape[2])
    for li, (w, b) in enumerate(zip(weights, biases)):
        d_in = in_dim if li == 0 else hid
        d_out = (out_dim if loss == "mse" else 2 * out_dim) if li == L - 1 else hid
        _check_dev(w, torch.float32, device, f"weights[{li}]", shape=(E, d_in, d_out))
        _check_dev(b, torch.float32, device, f"biases[{li}]", shape=(E, 1, d_out))
    if activation not in _lib.ACT:
        raise ValueError(f"unknown activation {activation!r}")
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])  # noqa: E731
    keep = [arr(weights), arr(biases)]
    d = _lib.TrainDesc(ensemble_size=E, n_layers=L, in_dim=in_dim, hid=hid, out_dim=out_dim, activation=_lib.ACT[activation],
                       leaky_slope=float(leaky_slope), max_batch=int(max_batch))
    d.weights = C.cast(keep[0], C.POINTER(C.c_void_p))
    d.biases = C.cast(keep[1], C.POINTER(C.c_void_p))
    if adam is not None:
        mw, mb, vw, vb, lo, hi, lr, b1, b2, eps, wd, spl = adam
        for name, ts, ref in (("exp_avg_w", mw, weights), ("exp_avg_b", mb, biases), ("exp_avg_sq_w", vw, weights), ("exp_avg_sq_b", vb, biases)):
            if len(ts) != L:
                raise ValueError(f"{name}: one tensor per layer")
            for li, (t, r) in enumerate(zip(ts, ref)):
                _check_dev(t, torch.float32, device, f"{name}[{li}]", shape=tuple(r.shape))
        for name, t in (("min_logvar", lo), ("max_logvar", hi)):
            if t is not None:  # (None = NULL: the library refuses it under NLL)
                _check_dev(t, torch.float32, device, name, numel=E * out_dim if bounds_per_member else out_dim)
        keep += [arr(mw), arr(mb), arr(vw), arr(vb), lo, hi]
        d.exp_avg_w, d.exp_avg_b, d.exp_avg_sq_w, d.exp_avg_sq_b = (C.cast(k, C.POINTER(C.c_void_p)) for k in keep[2:6])
        d.min_logvar = lo.data_ptr() if lo is not None else None
        d.max_logvar = hi.data_ptr() if hi is not None else None
        d.lr, d.beta1, d.beta2, d.eps, d.weight_decay = float(lr), float(b1), float(b2), float(eps), float(wd)
        d.steps_per_launch = int(spl)
    return d, keep


def pack_rollout_opts(spec: ModelSpec, device, mode: str, B: int, H: Optional[int], perms, members, eps, seed: int, stream_id: int,
                      member_schedule, rows_per_group: int, generic_kernel, *, sample: bool = True, perm_stream_id: int = 0, n_workgroups=None,
                      n_env: int = 0, trace_next_obs=None, trace_rewards=None, phase_cycles=None):
    """hipets_rollout_opts of a rollout of B rows over H steps, or -- ``H`` None -- of one step (hipets_step) -> (opts, keep-alive
    list).  The two differ in what they are given: a rollout's row -> member maps are [H, B] ([B] for fixed_model), its eps is [H, B,
    out_dim] and its member schedule [H, ``n_workgroups()``]; a step's maps are [B] and read in EXACT mode only, its eps has B * out_dim
    elements and is read only where the step samples, its schedule has any length."""
    step = H is None
    if mode not in _lib.MODES:
        raise ValueError("mode must be 'exact', 'fast' or 'device'")
    # (generic_kernel: False / True (1: fully generic instance only) / 2 (hidden-static allowed, shape-specialised not))
    o = _lib.RolloutOpts()
    o.mode, o.seed, o.stream_id, o.perm_stream_id = _lib.MODES[mode], int(seed), int(stream_id), int(perm_stream_id)
    o.rows_per_group, o.no_sample, o.generic_kernel, o.n_env = int(rows_per_group), int(not sample), int(generic_kernel), int(n_env)
    if mode == "device" and (perms is not None or eps is not None or members is not None):
        raise ValueError("mode='device' draws its permutation and eps in-kernel" if step else
                         "mode='device' draws its permutations and eps in-kernel: perms / eps / members must be None")
    if step and mode != "exact":
        perms = members = None
    if members is not None or perms is not None:
        want = (B,) if step or spec.propagation == "fixed_model" else (H, B)
    if members is not None:
        if step:
            if perms is not None or tuple(members.shape) != want:
                raise ValueError("members= must be int64 [B], exclusive with perm=")
        elif mode != "exact" or perms is not None:
            raise ValueError("members= (explicit per-row member maps) is an EXACT-mode input, exclusive with perms=")
        elif tuple(members.shape) != want:
            raise ValueError(f"members must have shape {want}")
        perms, o.rows_per_member = member_slots(members.reshape(-1, B), len(spec.members), device)
    elif perms is not None:
        _check_dev(perms, torch.int64, device, "perm" if step else "perms", want if step else None)
        if tuple(perms.shape) != want:
            raise ValueError(f"perms must have shape {want}")
    if step and mode == "exact":
        if not sample or spec.deterministic:
            eps = None  # (the mean: no draw is read)
        elif eps is None:
            raise ValueError("EXACT step with sample=True needs eps [B, out_dim]")
    if eps is not None:
        _check_dev(eps, torch.float32, device, "eps", **({"numel": B * spec.out_dim} if step else {"shape": (H, B, spec.out_dim)}))
    if mode == "exact":
        o.perms, o.eps = _ptr(perms), _ptr(eps)
    elif mode == "fast":
        o.fast_eps = _ptr(eps)
        if member_schedule is not None:
            _check_dev(member_schedule, torch.int32, device, "member_schedule", None if step else (H, n_workgroups()))
            o.member_schedule, o.member_schedule_len = member_schedule.data_ptr(), int(member_schedule.numel())
    if trace_next_obs is not None:
        _check_dev(trace_next_obs, torch.float32, device, "trace_next_obs", (H, B, spec.obs_dim))
        o.trace_next_obs = trace_next_obs.data_ptr()
    if trace_rewards is not None:
        _check_dev(trace_rewards, torch.float32, device, "trace_rewards", (H, B))
        o.trace_rewards = trace_rewards.data_ptr()
    if phase_cycles is not None:
        _check_dev(phase_cycles, torch.int64, device, "phase_cycles", (8, 16))
        o.phase_cycles = phase_cycles.data_ptr()
    return o, [perms]  # (member_slots' map has no other owner)


def pack_plan_trace(buffers: dict, max_rows: int):
    """hipets_plan_trace over the device tensors ``buffers`` (one per pointer field) -> (trace, keep-alive list)"""
    t = _lib.PlanTrace(max_rows=int(max_rows), **{name: buf.data_ptr() for name, buf in buffers.items()})
    return t, list(buffers.values())


POLICY_LAYERS = ("linear1", "linear2", "mean_linear", "log_std_linear")  # GaussianPolicy's nn.Linear modules
POLICY_TENSORS = ("w1", "b1", "w2", "b2", "wm", "bm", "ws", "bs", "action_scale", "action_bias")  # hipets_policy_set, in header order


def pack_policy(policy):
    """A ``GaussianPolicy``-shaped module (pytorch_sac_pranz24/model.py:66-113: linear1, linear2, mean_linear, log_std_linear,
    action_scale, action_bias) -> ((obs_dim, hidden, act_dim), {name: tensor} in ``POLICY_TENSORS`` order).  The layer tensors are the
    module's LIVE parameters (detached, nn.Linear's [out, in]); the reference's scalar action_scale 1 / action_bias 0 are broadcast
    to [act_dim] here.  Anything that is not shaped like a GaussianPolicy -- a DeterministicPolicy has neither head --, or whose sizes
    hipets_policy_set refuses, raises UnsupportedModelError."""
    from .model import UnsupportedModelError

    layers = [getattr(policy, n, None) for n in POLICY_LAYERS]
    if any(l is None or getattr(l, "weight", None) is None or getattr(l, "bias", None) is None or l.weight.ndim != 2 for l in layers):
        raise UnsupportedModelError(f"{type(policy).__name__} is not shaped like a GaussianPolicy (linear1, linear2, mean_linear, log_std_linear with biases)")
    l1, l2, lm, ls = layers
    hidden, obs_dim = (int(v) for v in l1.weight.shape)
    act_dim = int(lm.weight.shape[0])
    if tuple(l2.weight.shape) != (hidden, hidden) or tuple(lm.weight.shape) != (act_dim, hidden) or tuple(ls.weight.shape) != (act_dim, hidden):
        raise UnsupportedModelError("GaussianPolicy layer shapes do not chain: expected [hid, obs], [hid, hid] and two [act, hid] heads")
    if not (1 <= obs_dim <= _lib.POLICY_MAX_OBS and 1 <= hidden <= _lib.POLICY_MAX_HIDDEN and 1 <= act_dim <= _lib.POLICY_MAX_ACT):
        raise UnsupportedModelError(f"policy sizes (obs {obs_dim}, hidden {hidden}, act {act_dim}) outside the actor kernel's "
                                    f"(<= {_lib.POLICY_MAX_OBS}, <= {_lib.POLICY_MAX_HIDDEN}, <= {_lib.POLICY_MAX_ACT})")
    out = {}
    for name, lin in (("1", l1), ("2", l2), ("m", lm), ("s", ls)):
        out["w" + name], out["b" + name] = lin.weight.detach(), lin.bias.detach()
    for name, default in (("action_scale", 1.0), ("action_bias", 0.0)):
        v = torch.as_tensor(getattr(policy, name, default), dtype=torch.float32).detach().reshape(-1)
        if v.numel() not in (1, act_dim):
            raise UnsupportedModelError(f"policy.{name} holds {v.numel()} values for {act_dim} action dims")
        out[name] = v.expand(act_dim)
    return (obs_dim, hidden, act_dim), {n: out[n] for n in POLICY_TENSORS}


CRITIC_LAYERS = ("linear1", "linear2", "linear3", "linear4", "linear5", "linear6")  # hipets_critic_set's pointer table: weight, bias each


def pack_critic(critic, obs_dim: Optional[int] = None):
    """A ``QNetwork``-shaped module (pytorch_sac_pranz24/model.py:36-61: linear1..3 = Q1, linear4..6 = Q2) -> ((K, hidden), [the 12 LIVE
    parameters, weight then bias per layer, detached]) with K = obs_dim + act_dim, the width of linear1's input.  ``obs_dim``: how K
    splits (None: the split is not checked here).  Anything that is not shaped like a QNetwork, or whose sizes hipets_critic_set
    refuses, raises UnsupportedModelError."""
    from .model import UnsupportedModelError

    layers = [getattr(critic, n, None) for n in CRITIC_LAYERS]
    missing = [n for n, l in zip(CRITIC_LAYERS, layers)
               if l is None or getattr(l, "weight", None) is None or getattr(l, "bias", None) is None or l.weight.ndim != 2]
    if missing:
        raise UnsupportedModelError(f"{type(critic).__name__} is not shaped like a QNetwork: no {', '.join(missing)} with a weight and a bias")
    hidden, K = (int(v) for v in layers[0].weight.shape)
    want = [(hidden, K), (hidden, hidden), (1, hidden)] * 2
    for name, lin, shape in zip(CRITIC_LAYERS, layers, want):
        if tuple(lin.weight.shape) != shape or tuple(lin.bias.shape) != (shape[0],):
            raise UnsupportedModelError(f"QNetwork layer shapes do not chain: {name} is {tuple(lin.weight.shape)} with a bias of "
                                        f"{tuple(lin.bias.shape)}, expected {shape} and ({shape[0]},)")
    if not 1 <= hidden <= _lib.POLICY_MAX_HIDDEN or not 2 <= K <= _lib.POLICY_MAX_OBS + _lib.POLICY_MAX_ACT:
        raise UnsupportedModelError(f"critic sizes (obs + act {K}, hidden {hidden}) outside the critic kernel's "
                                    f"(<= {_lib.POLICY_MAX_OBS} + {_lib.POLICY_MAX_ACT}, <= {_lib.POLICY_MAX_HIDDEN})")
    if obs_dim is not None:
        check_critic_split(K, int(obs_dim), K - int(obs_dim))
    tensors = []
    for lin in layers:
        tensors += [lin.weight.detach(), lin.bias.detach()]
    return (K, hidden), tensors


def check_discount(discount) -> float:
    """``discount`` as a float in [0, 1] (what hipets_discounted_returns accepts), or ValueError"""
    g = float(discount)
    if not 0.0 <= g <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"discount must be in [0, 1], got {discount!r}")
    return g


def check_critic_split(K: int, obs_dim: int, act_dim: int):
    """(obs_dim, act_dim) against a critic whose linear1 takes K inputs and against the kernel's limits, or UnsupportedModelError"""
    from .model import UnsupportedModelError

    if obs_dim + act_dim != K:
        raise UnsupportedModelError(f"the critic's linear1 takes {K} inputs, obs_dim + act_dim = {obs_dim} + {act_dim}")
    if not (1 <= obs_dim <= _lib.POLICY_MAX_OBS and 1 <= act_dim <= _lib.POLICY_MAX_ACT):
        raise UnsupportedModelError(f"critic sizes (obs {obs_dim}, act {act_dim}) outside the critic kernel's "
                                    f"(<= {_lib.POLICY_MAX_OBS}, <= {_lib.POLICY_MAX_ACT})")


# ---- where a SAC transition's floats live (csrc/transition_layout.hpp for the kernels): an AREA of ``cap`` rows is five arrays one behind
# the other (``staging_views``), a BATCH ROW is (state, action, next state, reward, mask) ----
def row_width(obs_dim: int, act_dim: int) -> int:
    """Floats of a batch row, and of an area per row"""
    return 2 * obs_dim + act_dim + 2


def row_columns(obs_dim: int, act_dim: int):
    """Where a batch row's (action, next state, reward, mask) start; the state starts at 0"""
    return obs_dim, obs_dim + act_dim, 2 * obs_dim + act_dim, 2 * obs_dim + act_dim + 1


def staging_views(flat, cap: int, obs_dim: int, act_dim: int):
    """The five arrays of hipets_compact_transitions' staging area in ``flat`` (a tensor or a numpy array of at least cap * (2 obs_dim +
    act_dim + 2) float32): (obs [cap, obs_dim], action [cap, act_dim], next_obs [cap, obs_dim], reward [cap], done [cap] as 0.0 / 1.0)"""
    o1 = cap * obs_dim
    o2 = o1 + cap * act_dim
    o3 = o2 + cap * obs_dim
    return (flat[:o1].reshape(cap, obs_dim), flat[o1:o2].reshape(cap, act_dim), flat[o2:o3].reshape(cap, obs_dim), flat[o3:o3 + cap],
            flat[o3 + cap:o3 + 2 * cap])


def pack_sac_batch(transitions, reverse_mask: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
    """``memory.sample(batch_size).astuple()`` -> f32 [B, 2 obs + act + 2], a row = (state, action, next_state, reward, mask): what
    sac.py:80-95 uploads as five tensors.  mask = the terminated flag as a float, or ``1 - terminated`` under ``reverse_mask``
    (``mask_batch.logical_not()``).  The truncated flags are ignored, as there.  ``out``: a [B, width] array to fill."""
    state, action, next_state, reward, terminated = (np.asarray(v) for v in transitions[:5])
    B, obs = state.shape
    act = action.shape[1]
    c_act, c_next, c_rew, c_mask = row_columns(obs, act)
    if out is None:
        out = np.empty((B, row_width(obs, act)), dtype=np.float32)
    out[:, :c_act] = state
    out[:, c_act:c_next] = action
    out[:, c_next:c_rew] = next_state
    out[:, c_rew] = np.reshape(reward, B)
    mask = np.reshape(terminated, B).astype(np.float32)
    out[:, c_mask] = (mask == 0).astype(np.float32) if reverse_mask else mask
    return out
