"""The Engine binding on the host, no GPU and no libhipets.so: the real ``hipets.Engine`` over CPU tensors against a recording stand-in
for the library.  Every expectation is stated by the parameter NAMES of include/hipets.h (test_abi.header_prototypes): the tensor a
caller passes as ``lower`` must be the pointer at the header's parameter ``lower``; descriptors are compared field by field with what
the spec says, copied out while the call runs (the packers drop their keep-alives afterwards); every Python-side refusal raises its
exact message before any library call.  (That the library computes the right thing from these arguments is the GPU suite's business.)"""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest
import torch

import hipets
from hipets import BoxTermination, HipetsError, ModelSpec, ObsColumns, PlaNetSpec, RewardTerm, RewardTerms, _lib
from hipets.engine import Engine, member_slots
from test_abi import HEADER_SCALARS, HEADER_STRUCTS, header_prototypes

PROTOS = header_prototypes()
HANDLE, STREAM = 0x5EED0, 0xABCD00
CPU = torch.device("cpu")
ANY = object()  # an expectation that only says "this parameter is passed"
U64 = 2**64
# pointer fields that are arrays: field -> number of elements, from the snapshot of the scalar fields
ARRAYS = {
    "ModelDesc": {"members": lambda d: d["n_members"], "no_delta": lambda d: d["n_no_delta"], "norm_mean": lambda d: d["in_dim"],
                  "norm_std": lambda d: d["in_dim"], "weights": lambda d: d["n_layers"], "biases": lambda d: d["n_layers"],
                  "min_logvar": lambda d: d["out_dim"] * (d["n_members"] if d["ensemble_kind"] == 1 else 1),
                  "max_logvar": lambda d: d["out_dim"] * (d["n_members"] if d["ensemble_kind"] == 1 else 1),
                  "reward_terms": lambda d: d["n_reward_terms"], "term_intervals": lambda d: d["n_term_intervals"]},
    "TrainDesc": {f: (lambda d: d["n_layers"]) for f in ("weights", "biases", "exp_avg_w", "exp_avg_b", "exp_avg_sq_w", "exp_avg_sq_b")},
}


def snapshot(s):
    """A ctypes Structure as a dict of plain values: arrays behind pointer fields copied out (ARRAYS), NULL as None."""
    d = {f: getattr(s, f) for f, _ in s._fields_}
    for f, v in d.items():
        if isinstance(v, C._Pointer):
            n = ARRAYS[type(s).__name__][f](d)
            d[f] = None if not v else [tuple(getattr(v[i], g) for g, _ in v[i]._fields_) if isinstance(v[i], C.Structure) else v[i] for i in range(n)]
    return d


class FakeLib:
    """Records (symbol, {header parameter name: value}) of every call and returns 0.  Scalars arrive as ctypes' argtypes of the header's
    type deliver them (a Python int wraps into uint64_t); struct pointers as snapshots; byref'd output scalars are filled from
    ``outputs[symbol][name]``; ``peek[name] = (ctype, n)`` copies n elements out from behind a plain pointer parameter or struct field."""

    def __init__(self):
        self.calls, self.outputs, self.peek = [], {}, {}

    def __getattr__(self, symbol):
        if not symbol.startswith("hipets_"):
            raise AttributeError(symbol)
        params = PROTOS[symbol][1]

        def fn(*args):
            assert len(args) == len(params), f"{symbol}: {len(args)} arguments, the header declares {len(params)}"
            rec = {}
            for (ctype, name), a in zip(params, args):
                rec[name] = self._see(symbol, ctype, name, a)
                if name in self.peek and isinstance(rec[name], int):
                    rec[name + "_data"] = self._copy(rec[name], name)
            self.calls.append((symbol, rec))
            return 0

        return fn

    def _copy(self, address, name):
        ct, n = self.peek[name]
        return list(C.cast(address, C.POINTER(ct))[:n])

    def _see(self, symbol, ctype, name, a):
        if ctype in HEADER_SCALARS:
            return HEADER_SCALARS[ctype](a).value
        if a is None:
            return None
        if ctype[:-1] in HEADER_STRUCTS:
            if isinstance(a, C.Array):  # a table (hipets_set_model_columns' cols)
                return [snapshot(x) for x in a]
            snap = snapshot(a._obj)  # (byref)
            snap.update({f + "_data": self._copy(snap[f], f) for f in self.peek if snap.get(f)})
            return snap
        if hasattr(a, "_obj"):  # byref of an output scalar
            if name in self.outputs.get(symbol, {}):
                a._obj.value = self.outputs[symbol][name]
            return "out"
        if isinstance(a, C.Array):  # an output buffer (hipets_comm_unique_id)
            a.raw = self.outputs[symbol][name]
            return "out"
        if isinstance(a, (C.c_void_p, C.c_char_p)):
            return a.value
        return a if isinstance(a, bytes) else int(a)


def make_engine():
    """An Engine without __init__ (which needs a GPU): CPU device, the recording library, a dummy handle."""
    e = object.__new__(Engine)
    e.device, e._lib, e._h = CPU, FakeLib(), C.c_void_p(HANDLE)
    e.spec, e.planet_spec, e.comm_world, e.comm_rank, e.comm_group, e.plan_mode, e._trace = None, None, 1, 0, None, "fast", None
    return e


def patch_cuda(monkeypatch):
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=STREAM))


@pytest.fixture
def eng(monkeypatch):
    patch_cuda(monkeypatch)
    e = make_engine()
    yield e
    e._h = None  # (nothing to destroy)


def plain(v):
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    return snapshot(v) if isinstance(v, C.Structure) else v


def take(eng, symbol):
    """The one call recorded since the last take: it must be ``symbol``."""
    assert [s for s, _ in eng._lib.calls] == [symbol]
    return eng._lib.calls.pop()[1]


def check(rec, symbol, **want):
    """``rec`` has, at every parameter the header declares for ``symbol``, the value ``want`` states under that name (a tensor: its
    data pointer; a struct: its snapshot); the handle at ``e`` and the stream at ``stream`` are implied."""
    types_ = {n: c for c, n in PROTOS[symbol][1]}
    assert sorted(set(want) | ({"e", "stream"} & set(types_))) == sorted(types_), f"{symbol}: expectations must name every header parameter"
    assert rec.get("e", HANDLE) == HANDLE and rec.get("stream", STREAM) == STREAM
    for n, v in want.items():
        if v is not ANY:
            v = HEADER_SCALARS[types_[n]](v).value if types_[n] in HEADER_SCALARS else plain(v)  # (a scalar: as its C type holds it)
            assert rec[n] == v, f"{symbol}: parameter {n}"


def call(eng, method, symbol, rename=None, extra=None, **kw):
    """eng.method(**kw) makes exactly one library call, ``symbol``, whose header parameter N holds the keyword argument N (``rename``:
    header name -> Python name where they differ; ``extra``: header name -> expectation for what is not an argument).  Returns
    (the method's result, the recorded call)."""
    rename, extra = rename or {}, extra or {}
    res = getattr(eng, method)(**kw)
    rec = take(eng, symbol)
    names = [n for _, n in PROTOS[symbol][1] if n not in ("e", "stream")]
    check(rec, symbol, **{n: extra[n] if n in extra else kw[rename.get(n, n)] for n in names})
    return res, rec


def t(*shape, dtype=torch.float32):
    """A fresh tensor: pairwise distinct storage as long as the caller holds them"""
    return torch.zeros(*shape, dtype=dtype)


def f32(x):
    return float(np.float32(x))


OBS, ACT, E, HID = 3, 2, 3, 4
HA = {"horizon": "H", "act_dim": "A"}  # header name -> Python name of the optimizer pieces


def make_spec(**kw):
    g = torch.Generator().manual_seed(0)
    det = kw.get("deterministic", False)
    in_dim = kw.pop("in_dim", OBS + ACT)
    out = OBS * (1 if det else 2)
    base = dict(weights=[torch.randn(E, in_dim, HID, generator=g), torch.randn(E, HID, out, generator=g)],
                biases=[torch.randn(E, 1, HID, generator=g), torch.randn(E, 1, out, generator=g)], obs_dim=OBS, act_dim=ACT,
                min_logvar=None if det else torch.tensor([[-3.0, -2.5, -2.0]]), max_logvar=None if det else torch.tensor([[0.5, 1.0, 1.5]]),
                reward="halfcheetah")
    base.update(kw)
    return ModelSpec(**base)


# ---- the optimizer pieces and the queries: position and value of every argument ---------------------------------------------------
def test_cem_pieces(eng):
    p = Engine.cem_params(5, 3, 2, 4, 2, 0.1, clipped_normal=True)
    mu, disp, lo, hi, pop, z = t(3, 2), t(3, 2), t(3, 2), t(3, 2), t(5, 3, 2), t(5, 3, 2)
    res, rec = call(eng, "cem_sample", "hipets_cem_sample", p=p, mu=mu, dispersion=disp, lower=lo, upper=hi, population=pop, z=None,
                    seed=-1, stream_id=U64 + 5)
    assert res is pop and rec["z"] is None and rec["seed"] == U64 - 1 and rec["stream_id"] == 5
    assert rec["p"]["clipped_normal"] == 1 and rec["p"]["alpha"] == 0.1 and rec["p"]["unbiased_var"] == 1
    res, rec = call(eng, "cem_sample", "hipets_cem_sample", p=p, mu=mu, dispersion=disp, lower=lo, upper=hi, population=pop, z=z, seed=7,
                    stream_id=9)
    assert rec["z"] == z.data_ptr() and (rec["seed"], rec["stream_id"]) == (7, 9)
    vals, bv, bs, ei = t(5), t(1), t(3, 2), t(2, dtype=torch.int32)
    res, _ = call(eng, "cem_refit", "hipets_cem_refit", p=p, values=vals, population=pop, mu=mu, dispersion=disp, best_value=bv,
                  best_solution=bs, elite_idx=ei)
    assert res is None
    call(eng, "cem_refit", "hipets_cem_refit", p=p, values=vals, population=pop, mu=mu, dispersion=disp, best_value=bv, best_solution=bs,
         elite_idx=None)
    elites = torch.tensor([4, 1], dtype=torch.int32)
    call(eng, "cem_refit", "hipets_cem_refit_elites", p=p, values=vals, population=pop, mu=mu, dispersion=disp, best_value=bv,
         best_solution=bs, elite_idx=ei, elites=elites)
    assert ei.tolist() == [4, 1]  # the caller's elites are reported as elite_idx
    src, idx, out = t(5, 6), t(2, dtype=torch.int32), t(2, 6)
    res, rec = call(eng, "gather_rows", "hipets_gather_rows", extra={"rows": 2, "dim": 6, "dst": out}, src=src, index=idx, out=out)
    assert res is out


def test_mppi_and_icem_pieces(eng):
    mean, past, lo, hi, pop, z, vals = t(3, 2), t(2), t(3, 2), t(3, 2), t(5, 3, 2), t(5, 3, 2), t(5)
    res, rec = call(eng, "mppi_sample", "hipets_mppi_sample", HA, pop=5, H=3, A=2, beta=0.25, mean=mean, past_action=past, lower=lo,
                    upper=hi, population=pop, z=z, seed=-2, stream_id=U64)
    assert res is pop and (rec["seed"], rec["stream_id"]) == (U64 - 2, 0)
    call(eng, "mppi_sample", "hipets_mppi_sample", HA, pop=5, H=3, A=2, beta=0.25, mean=mean, past_action=past, lower=lo, upper=hi,
         population=pop, z=None, seed=1, stream_id=2)
    res, _ = call(eng, "mppi_update", "hipets_mppi_update", HA, pop=5, H=3, A=2, gamma=0.9, values=vals, population=pop, mean=mean)
    assert res is mean
    mu, var, normals, big = t(4, 2), t(4, 2), t(2, 5, 2, 3), t(7, 4, 2)
    lo4, hi4 = t(4, 2), t(4, 2)
    res, rec = call(eng, "icem_sample", "hipets_icem_sample", HA, n=5, H=4, A=2, exponent=2.0, mu=mu, var=var, lower=lo4, upper=hi4,
                    population=big, normals=normals, seed=-1, stream_id=3)
    assert res is big and rec["seed"] == U64 - 1
    call(eng, "icem_sample", "hipets_icem_sample", HA, n=5, H=4, A=2, exponent=2.0, mu=mu, var=var, lower=lo4, upper=hi4, population=big,
         normals=None, seed=0, stream_id=0)
    kept, out, noise = t(2, 4, 2), t(2, 4, 2), t(2, 2)
    res, rec = call(eng, "icem_shift", "hipets_icem_shift", HA, keep=2, H=4, A=2, kept=kept, mu=mu, var=var, out=out, end_noise=noise,
                    seed=U64 + 1, stream_id=-1)
    assert res is out and (rec["seed"], rec["stream_id"]) == (1, U64 - 1)
    call(eng, "icem_shift", "hipets_icem_shift", HA, keep=2, H=4, A=2, kept=kept, mu=mu, var=var, out=out, end_noise=None, seed=0,
         stream_id=0)


def test_queries_and_switches(eng):
    out = {"hipets_fast_geometry": {"n_workgroups": 11, "row_tiles": 2}, "hipets_kernel_class": {"kernel_class": 3, "row_tiles": 2},
           "hipets_check_async_error": {"timed_out": 1}, "hipets_planet_kernel_class": {"is_static": 0},
           "hipets_comm_info": {"rank": 2, "world_size": 4}, "hipets_timing_read": {"launches": 9, "total_ms": 1.5},
           "hipets_comm_unique_id": {"id_out": bytes(range(1, 129))}}
    eng._lib.outputs = out
    res, _ = call(eng, "fast_geometry", "hipets_fast_geometry", extra={"n_workgroups": "out", "row_tiles": "out"}, pop=40, num_particles=5,
                  horizon=6, rows_per_group=-1)
    assert res == (11, 2)
    res, rec = call(eng, "kernel_class", "hipets_kernel_class", extra={"kernel_class": "out", "row_tiles": "out", "mode": 1}, pop=40,
                    num_particles=5, horizon=6, mode="fast", rows_per_group=2)
    assert res == ("wide", 2)
    assert call(eng, "check_async_error", "hipets_check_async_error", extra={"timed_out": "out"})[0] is True
    assert call(eng, "planet_kernel_class", "hipets_planet_kernel_class", extra={"is_static": "out"})[0] == "generic"
    assert call(eng, "comm_info", "hipets_comm_info", extra={"rank": "out", "world_size": "out"})[0] == (2, 4)
    assert call(eng, "timing_read", "hipets_timing_read", extra={"launches": "out", "total_ms": "out", "reset": 0}, reset=False)[0] == (9, 1.5)
    call(eng, "timing_enable", "hipets_timing_enable", on=4)
    call(eng, "timing_enable", "hipets_timing_enable", extra={"on": 1}, on=True)
    call(eng, "set_persistent", "hipets_set_persistent", extra={"on": 0}, on=False)
    call(eng, "set_handover_timeout", "hipets_set_handover_timeout", seconds=0.5)
    call(eng, "set_plan_mode", "hipets_set_plan_mode", extra={"mode": 2}, mode="device")
    assert eng.plan_mode == "device"
    assert call(eng, "comm_unique_id", "hipets_comm_unique_id", extra={"id_out": "out"})[0] == bytes(range(1, 129))
    call(eng, "comm_init", "hipets_comm_init", unique_id=bytes(range(1, 129)), rank=1, world_size=2)
    assert (eng.comm_world, eng.comm_rank) == (2, 1)
    eng.comm_group = "group"
    call(eng, "comm_destroy", "hipets_comm_destroy")
    assert (eng.comm_world, eng.comm_rank, eng.comm_group) == (1, 0, None)
    call(eng, "close", "hipets_destroy")
    assert eng._h is None
    eng.close()  # a second close calls nothing
    assert eng._lib.calls == []


def test_replay_exports_and_trajectory_returns(eng):
    eng.spec = make_spec()
    res, rec = call(eng, "fast_schedule", "hipets_fast_schedule", extra={"schedule": ANY}, horizon=4, n_workgroups=3, seed=-1, stream_id=U64 + 2)
    assert res.shape == (4, 3) and res.dtype == torch.int32 and rec["schedule"] == res.data_ptr() and (rec["seed"], rec["stream_id"]) == (U64 - 1, 2)
    res, rec = call(eng, "fast_normals", "hipets_fast_normals", extra={"normals": ANY}, horizon=4, batch=10, seed=3, stream_id=-4)
    assert res.shape == (4, 10, OBS) and res.dtype == torch.float32 and rec["normals"] == res.data_ptr() and rec["stream_id"] == U64 - 4
    res, rec = call(eng, "device_perms", "hipets_device_perms", extra={"perms": ANY}, horizon=4, batch=10, seed=3, stream_id=5)
    assert res.shape == (4, 10) and res.dtype == torch.int64 and rec["perms"] == res.data_ptr()
    eng.spec = make_spec(propagation="fixed_model")
    res, rec = call(eng, "device_perms", "hipets_device_perms", extra={"perms": ANY}, horizon=4, batch=10, seed=3, stream_id=5)
    assert res.shape == (10,) and rec["perms"] == res.data_ptr()
    rewards, dones = t(4, 6), t(4, 6, dtype=torch.bool)
    names = {"horizon": 4, "returns": ANY, "row_totals": None, "first_done": None, "dones": ANY}
    res, rec = call(eng, "trajectory_returns", "hipets_trajectory_returns", extra=names, rewards=rewards, dones=dones, pop=3, num_particles=2)
    assert res.shape == (3,) and res.dtype == torch.float32 and rec["returns"] == res.data_ptr() and rec["dones"] == dones.data_ptr()
    d8 = t(4, 6, dtype=torch.uint8)
    (ret, tot, first), rec = call(eng, "trajectory_returns", "hipets_trajectory_returns", extra=dict(names, row_totals=ANY, first_done=ANY, dones=d8),
                                  rewards=rewards, dones=d8, pop=3, num_particles=2, row_totals=True, first_done=True)
    assert (tot.shape, tot.dtype, first.shape, first.dtype) == ((6,), torch.float32, (6,), torch.int32)
    assert (rec["returns"], rec["row_totals"], rec["first_done"]) == (ret.data_ptr(), tot.data_ptr(), first.data_ptr())
    (ret, tot, first), rec = call(eng, "trajectory_returns", "hipets_trajectory_returns", extra=dict(names, first_done=ANY, dones=d8),
                                  rewards=rewards, dones=d8, pop=3, num_particles=2, first_done=True)
    assert tot is None and rec["first_done"] == first.data_ptr()


# ---- hipets_model_desc, field by field against the spec -----------------------------------------------------------------------------
BOX = BoxTermination([(0, -1.0, 2.0, True, False), (2, -0.5)], require_finite=True)
TERMS = RewardTerms([RewardTerm("square", 1, w=2.0, level=1), RewardTerm("sin", 0, j=2, level=1, op="mul"), RewardTerm("sqrt", 0, source="group", c=0.5),
                     RewardTerm("linear", 1, w=-0.1, source="act"), RewardTerm("exp", 0, source="const", c=1.5, op="div")],
                    bias=0.25, alive_bonus=1.0, termination_fn=BOX)
COLUMNS = ObsColumns([(1, "id"), (2, "sin"), (2, "cos"), (0, "id")])
MODELS = {
    "enums": lambda: make_spec(reward="cartpole", termination="cartpole", obs_process="none", activation="leaky_relu", leaky_slope=0.02,
                               propagation="fixed_model", precision="bf16x3"),
    "tables": lambda: make_spec(reward=TERMS, termination=BOX, obs_process=COLUMNS, in_dim=4 + ACT),
    "basic_shared_bounds": lambda: make_spec(ensemble_kind="basic_ensemble", elite_models=[1], reward="pusher"),
    "basic_own_bounds": lambda: make_spec(ensemble_kind="basic_ensemble", min_logvar=torch.arange(9.0).reshape(3, 3) - 9,
                                          max_logvar=torch.arange(9.0).reshape(3, 3)),
    "deterministic": lambda: make_spec(deterministic=True, reward="none", propagation="expectation"),
    "norm_f32": lambda: make_spec(norm_mean=torch.arange(5, dtype=torch.float32).reshape(1, 5) / 3, norm_std=torch.arange(1, 6, dtype=torch.float32).reshape(1, 5) / 7),
    "norm_f64": lambda: make_spec(norm_mean=torch.arange(5, dtype=torch.float64).reshape(1, 5) / 3, norm_std=torch.arange(1, 6, dtype=torch.float64).reshape(1, 5) / 7),
    "elites_no_delta": lambda: make_spec(elite_models=[2, 0], no_delta_list=[2, 0], target_is_delta=False, termination="hopper", obs_process="halfcheetah"),
    "learned_reward": lambda: ModelSpec(weights=[t(E, OBS + ACT, HID), t(E, HID, 2 * (OBS + 1))], biases=[t(E, 1, HID), t(E, 1, 2 * (OBS + 1))], obs_dim=OBS,
                                        act_dim=ACT, min_logvar=t(1, OBS + 1), max_logvar=t(1, OBS + 1), reward=None, learned_rewards=True),
}


def expected_desc(spec, ws, bs):
    """hipets_model_desc as include/hipets.h describes it, written from the spec alone"""
    tables = isinstance(spec.reward, RewardTerms), isinstance(spec.termination, BoxTermination), isinstance(spec.obs_process, ObsColumns)
    M, basic = spec.members, spec.ensemble_kind == "basic_ensemble"
    want = dict(obs_dim=spec.obs_dim, act_dim=spec.act_dim, in_dim=spec.in_dim, out_dim=spec.out_dim, hid=spec.hid, n_layers=len(spec.weights),
                ensemble_size=spec.ensemble_size, n_members=len(M), members=list(M), activation=_lib.ACT[spec.activation],
                leaky_slope=f32(spec.leaky_slope), propagation=_lib.PROP[spec.propagation], deterministic=int(spec.deterministic),
                obs_process=3 if tables[2] else _lib.OBS[spec.obs_process], reward_fn=7 if tables[0] else _lib.REW[spec.reward],
                termination_fn=7 if tables[1] else _lib.TERM[spec.termination], target_is_delta=int(spec.target_is_delta),
                learned_rewards=int(spec.learned_rewards), n_no_delta=len(spec.no_delta_list), no_delta=list(spec.no_delta_list),
                normalizer=0, norm_mean=None, norm_std=None, min_logvar=None, max_logvar=None, weights=[w.data_ptr() for w in ws],
                biases=[b.data_ptr() for b in bs], ensemble_kind=int(basic), precision=_lib.PREC[spec.precision], reward_terms=None,
                term_intervals=None, n_reward_terms=0, n_term_intervals=0, reward_bias=0.0, alive_bonus=0.0, term_require_finite=0)
    if spec.norm_mean is not None:
        want.update(normalizer=2 if spec.norm_mean.dtype == torch.float64 else 1, norm_mean=spec.norm_mean.double().reshape(-1).tolist(),
                    norm_std=spec.norm_std.double().reshape(-1).tolist())
    if not spec.deterministic:
        rows = len(M) if basic else 1
        want.update(min_logvar=spec.min_logvar.float().reshape(-1, spec.out_dim).expand(rows, spec.out_dim).reshape(-1).tolist(),
                    max_logvar=spec.max_logvar.float().reshape(-1, spec.out_dim).expand(rows, spec.out_dim).reshape(-1).tolist())
    if tables[0]:
        fn, src, op = ("linear", "square", "abs", "sin", "cos", "exp", "sqrt"), ("obs", "act", "group", "const"), ("add", "mul", "div")
        want.update(n_reward_terms=len(spec.reward.terms), reward_bias=f32(spec.reward.bias), alive_bonus=f32(spec.reward.alive_bonus),
                    reward_terms=[(fn.index(r.fn) | op.index(r.op) << 8 | r.level << 16, src.index(r.source), r.i, -1 if r.j is None else r.j,
                                   f32(r.c), f32(r.w)) for r in spec.reward.terms])
    if tables[1]:
        want.update(n_term_intervals=len(spec.termination.intervals), term_require_finite=int(spec.termination.require_finite),
                    term_intervals=[(iv.dim, int(iv.lo_open) | int(iv.hi_open) << 1, f32(iv.lo), f32(iv.hi)) for iv in spec.termination.intervals])
    return want


@pytest.mark.parametrize("name", sorted(MODELS))
def test_set_model_packs_the_descriptor(eng, name):
    spec = MODELS[name]()
    eng.set_model(spec)
    assert eng.spec is spec
    want = expected_desc(spec, spec.weights, spec.biases)  # (f32, contiguous, on the device already: the engine packs the spec's own tensors)
    if isinstance(spec.obs_process, ObsColumns):
        rec = take(eng, "hipets_set_model_columns")
        cols = [{"dim": c.dim, "fn": ("id", "sin", "cos").index(c.fn)} for c in spec.obs_process.columns]
        check(rec, "hipets_set_model_columns", desc=ANY, cols=cols, n_cols=len(cols))
    else:
        rec = take(eng, "hipets_set_model")
        check(rec, "hipets_set_model", desc=ANY)
    assert sorted(rec["desc"]) == sorted(want)
    for f in want:
        assert rec["desc"][f] == want[f], f"hipets_model_desc.{f}"
    if name == "basic_shared_bounds":
        assert rec["desc"]["n_members"] == 3 and rec["desc"]["min_logvar"] == [-3.0, -2.5, -2.0] * 3  # [1, out] arrives as [M, out]; no elites


def test_set_model_converts_weights_to_f32_on_the_device(eng):
    spec = make_spec()
    spec.weights = [w.double() for w in spec.weights]
    spec.biases = [b.transpose(1, 2).contiguous().transpose(1, 2) for b in spec.biases]
    eng.set_model(spec)
    d = take(eng, "hipets_set_model")["desc"]
    assert all(a != w.data_ptr() for a, w in zip(d["weights"], spec.weights)) and len(set(d["weights"] + d["biases"])) == 4


# ---- hipets_rollout_opts --------------------------------------------------------------------------------------------------------
def opts_want(struct=_lib.RolloutOpts, **over):
    want = snapshot(struct())
    want.update({k: plain(v) for k, v in over.items()})
    return want


POP, P, H = 6, 2, 3
B = POP * P


def rollout(eng, **kw):
    """eng.rollout(...) -> (result, recorded hipets_rollout call); actions / s0 / num_particles default"""
    kw.setdefault("actions", t(POP, H, ACT))
    kw.setdefault("s0", np.arange(OBS * kw.get("n_env", 1), dtype=np.float64) + 0.5)
    kw.setdefault("num_particles", P)
    eng._lib.peek = {**eng._lib.peek, "s0": (C.c_float, len(kw["s0"]))}
    res, rec = call(eng, "rollout", "hipets_rollout", extra={"pop": POP, "horizon": H, "opts": ANY, "returns": ANY, "s0": ANY}, **kw)
    assert rec["s0_data"] == [float(v) for v in kw["s0"]]  # staged as f32 on the host, alive during the call
    assert res.data_ptr() == rec["returns"] and res.shape == (POP,) and res.dtype == torch.float32
    return res, rec


def test_rollout_opts_by_mode(eng):
    eng.set_model(make_spec())
    take(eng, "hipets_set_model")
    perms, eps = t(H, B, dtype=torch.int64), t(H, B, OBS)
    _, rec = rollout(eng, mode="exact", perms=perms, eps=eps, seed=-1, stream_id=U64 + 3)
    assert rec["opts"] == opts_want(mode=0, perms=perms, eps=eps, seed=U64 - 1, stream_id=3, n_env=1)
    _, rec = rollout(eng, mode="fast", eps=eps, seed=4, stream_id=5, rows_per_group=2)
    assert rec["opts"] == opts_want(mode=1, fast_eps=eps, seed=4, stream_id=5, rows_per_group=2, n_env=1)
    _, rec = rollout(eng, mode="device", seed=U64, stream_id=-2)
    assert rec["opts"] == opts_want(mode=2, seed=0, stream_id=U64 - 2, n_env=1)
    out = t(POP)
    res, rec = rollout(eng, out=out)  # the default mode is FAST; a caller's out is filled and returned
    assert res is out and rec["opts"] == opts_want(mode=1, n_env=1)
    for flag, want in ((True, 1), (2, 2), (False, 0)):
        assert rollout(eng, mode="device", generic_kernel=flag)[1]["opts"]["generic_kernel"] == want
    tn, tr, pc = t(H, B, OBS), t(H, B), t(8, 16, dtype=torch.int64)
    _, rec = rollout(eng, mode="device", trace_next_obs=tn, trace_rewards=tr, phase_cycles=pc)
    assert rec["opts"] == opts_want(mode=2, n_env=1, trace_next_obs=tn, trace_rewards=tr, phase_cycles=pc)
    _, rec = rollout(eng, mode="device", n_env=3)  # s0 is then [n_env, obs_dim]
    assert rec["opts"] == opts_want(mode=2, n_env=3)


def test_rollout_member_maps_and_schedules(eng):
    eng.set_model(make_spec(elite_models=[2, 0]))
    take(eng, "hipets_set_model")
    members = torch.tensor([[0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1]] * H)
    slots, rpm = member_slots(members, 2, CPU)
    assert rpm == 9
    eng._lib.peek = {"perms": (C.c_int64, slots.numel())}
    _, rec = rollout(eng, mode="exact", members=members)
    assert rec["opts"]["perms_data"] == slots.reshape(-1).tolist() and rec["opts"]["rows_per_member"] == rpm and rec["opts"]["mode"] == 0
    eng._lib.peek = {}
    eng._lib.outputs = {"hipets_fast_geometry": {"n_workgroups": 5, "row_tiles": 1}}
    sched = t(H, 5, dtype=torch.int32)
    res = eng.rollout(t(POP, H, ACT), np.zeros(OBS), P, mode="fast", member_schedule=sched, rows_per_group=1)
    (s1, geo), (s2, rec) = eng._lib.calls
    eng._lib.calls.clear()
    assert (s1, s2) == ("hipets_fast_geometry", "hipets_rollout")
    check(geo, "hipets_fast_geometry", pop=POP, num_particles=P, horizon=H, rows_per_group=1, n_workgroups="out", row_tiles="out")
    assert rec["opts"] == opts_want(mode=1, n_env=1, rows_per_group=1, member_schedule=sched, member_schedule_len=H * 5)
    eng.set_model(make_spec(propagation="fixed_model"))
    take(eng, "hipets_set_model")
    perm = t(B, dtype=torch.int64)
    assert rollout(eng, mode="exact", perms=perm)[1]["opts"]["perms"] == perm.data_ptr()  # fixed_model: one [B] map


def step(eng, **kw):
    kw.setdefault("obs", t(B, OBS))
    kw.setdefault("actions", t(B, ACT))
    (nxt, rew, done), rec = call(eng, "step", "hipets_step", extra={"batch": B, "opts": ANY, "next_obs": ANY, "rewards": ANY, "dones": ANY}, **kw)
    assert nxt.shape == (B, OBS) and nxt.dtype == torch.float32 and nxt.data_ptr() == rec["next_obs"] != kw["obs"].data_ptr()
    assert rew.shape == (B, 1) and rew.dtype == torch.float32 and rew.data_ptr() == rec["rewards"]
    assert done.shape == (B, 1) and done.dtype == torch.bool and rec["dones"] not in (None, rec["rewards"], rec["next_obs"])
    return rec


def test_step_opts_by_mode(eng):
    eng.set_model(make_spec())
    take(eng, "hipets_set_model")
    perm, eps, sched = t(B, dtype=torch.int64), t(B, OBS), t(7, dtype=torch.int32)
    rec = step(eng, mode="exact", perm=perm, eps=eps, seed=-1, stream_id=U64 + 1)
    assert rec["opts"] == opts_want(mode=0, perms=perm, eps=eps, seed=U64 - 1, stream_id=1)
    rec = step(eng, mode="exact", perm=perm, sample=False)  # the mean: no eps needed, none passed
    assert rec["opts"] == opts_want(mode=0, perms=perm, no_sample=1)
    rec = step(eng, mode="fast", eps=eps.view(1, B, OBS), member_schedule=sched, rows_per_group=3, seed=2, stream_id=3)
    assert rec["opts"] == opts_want(mode=1, fast_eps=eps, member_schedule=sched, member_schedule_len=7, rows_per_group=3, seed=2, stream_id=3)
    rec = step(eng)  # the default mode is FAST
    assert rec["opts"] == opts_want(mode=1)
    rec = step(eng, mode="device", sample=False, perm_stream_id=-1, seed=5, stream_id=U64 + 6, generic_kernel=2)
    assert rec["opts"] == opts_want(mode=2, no_sample=1, perm_stream_id=U64 - 1, seed=5, stream_id=6, generic_kernel=2)
    assert step(eng, mode="device", generic_kernel=True, perm_stream_id=U64 + 9)["opts"] == opts_want(mode=2, generic_kernel=1, perm_stream_id=9)
    members = torch.tensor([2, 2, 0, 1, 2, 2, 0, 2, 2, 1, 2, 2])
    slots, rpm = member_slots(members.reshape(1, B), 3, CPU)
    eng._lib.peek = {"perms": (C.c_int64, slots.numel())}
    rec = step(eng, mode="exact", members=members, eps=eps)
    assert rec["opts"]["perms_data"] == slots.reshape(-1).tolist() and rec["opts"]["rows_per_member"] == rpm == 8 and rec["opts"]["eps"] == eps.data_ptr()
    eng._lib.peek = {}
    eng.set_model(make_spec(deterministic=True, reward="none"))
    take(eng, "hipets_set_model")
    assert step(eng, mode="exact", perm=perm)["opts"] == opts_want(mode=0, perms=perm)  # a deterministic model takes no eps


# ---- the fused plans ------------------------------------------------------------------------------------------------------------
MPPI = {"population_size": "pop", "horizon": "H", "act_dim": "A"}


def plan_fixture(eng):
    eng.set_model(make_spec())
    take(eng, "hipets_set_model")
    cem = Engine.cem_params(8, H, ACT, 2, 3, 0.1)
    icem = _lib.IcemParams(population_size=8, horizon=H, act_dim=ACT, num_iterations=2, elite_num=3, keep_elite_size=2, alpha=0.1)
    return cem, icem, t(H, ACT), t(H, ACT)


def s0_of(eng, n_env, kw):
    s0 = np.arange(n_env * OBS, dtype=np.float64).reshape(n_env, OBS) - 1.25
    eng._lib.peek = {"s0": (C.c_float, s0.size)}
    return dict(kw, s0=s0), {"s0": ANY}, s0.reshape(-1).tolist()


@pytest.mark.parametrize("n_env", [1, 2])
def test_local_plans(eng, n_env):
    cem, icem, lo, hi = plan_fixture(eng)
    shape = (H, ACT) if n_env == 1 else (n_env, H, ACT)
    x0, out = t(*shape), t(*shape)
    kw, extra, s0 = s0_of(eng, n_env, dict(lower=lo, upper=hi, num_particles=P, n_env=n_env))
    res, rec = call(eng, "plan_cem", "hipets_plan_cem_batched", extra=dict(extra, out=ANY), p=cem, x0=x0, seed=-1, plan_id=U64 + 2, **kw)
    assert rec["s0_data"] == s0 and res.data_ptr() == rec["out"] not in (x0.data_ptr(), None) and res.shape == shape and res.dtype == torch.float32
    assert (rec["seed"], rec["plan_id"]) == (U64 - 1, 2)
    res, _ = call(eng, "plan_cem", "hipets_plan_cem_batched", extra=extra, p=cem, x0=x0, out=out, seed=1, plan_id=2, **kw)
    assert res is out
    mean = t(*shape)
    res, rec = call(eng, "plan_mppi", "hipets_plan_mppi_batched", MPPI, extra, pop=8, H=H, A=ACT, num_iterations=2, gamma=0.9, beta=0.25,
                    mean=mean, seed=U64, plan_id=-3, **kw)
    assert res is mean and rec["s0_data"] == s0 and (rec["seed"], rec["plan_id"]) == (0, U64 - 3)
    elite, keep = t(*shape[:-2], 3, H, ACT), t(2, n_env, 2, dtype=torch.int32)
    res, rec = call(eng, "plan_icem", "hipets_plan_icem_batched", extra=dict(extra, out=ANY, has_elite=1), p=icem, x0=x0, elite=elite,
                    has_elite=True, keep_idx=keep, seed=3, plan_id=4, **kw)
    assert res.data_ptr() == rec["out"] and res.shape == shape and rec["s0_data"] == s0
    res, rec = call(eng, "plan_icem", "hipets_plan_icem_batched", extra=dict(extra, has_elite=0), p=icem, x0=x0, elite=elite, has_elite=False,
                    keep_idx=None, out=out, seed=3, plan_id=4, **kw)
    assert res is out and rec["keep_idx"] is None


def test_sharded_plans(eng):
    cem, icem, lo, hi = plan_fixture(eng)
    x0, out, mean, elite, keep = t(H, ACT), t(H, ACT), t(H, ACT), t(3, H, ACT), t(2, 2, dtype=torch.int32)
    kw, extra, s0 = s0_of(eng, 1, dict(lower=lo, upper=hi, num_particles=P))
    res, rec = call(eng, "plan_cem_sharded", "hipets_plan_cem_sharded", extra=dict(extra, out=ANY), p=cem, x0=x0, seed=-1, plan_id=U64 + 2, **kw)
    assert res.data_ptr() == rec["out"] and res.shape == (H, ACT) and rec["s0_data"] == s0 and (rec["seed"], rec["plan_id"]) == (U64 - 1, 2)
    assert call(eng, "plan_cem_sharded", "hipets_plan_cem_sharded", extra=extra, p=cem, x0=x0, out=out, seed=3, plan_id=4, **kw)[0] is out
    res, _ = call(eng, "plan_mppi_sharded", "hipets_plan_mppi_sharded", MPPI, extra, pop=8, H=H, A=ACT, num_iterations=2, gamma=0.9, beta=0.25,
                  mean=mean, seed=5, plan_id=6, **kw)
    assert res is mean
    res, rec = call(eng, "plan_icem_sharded", "hipets_plan_icem_sharded", extra=dict(extra, out=ANY, has_elite=1), p=icem, x0=x0, elite=elite,
                    has_elite=1, keep_idx=keep, seed=5, plan_id=-6, **kw)
    assert res.data_ptr() == rec["out"] and res.shape == (H, ACT) and rec["plan_id"] == U64 - 6
    assert call(eng, "plan_icem_sharded", "hipets_plan_icem_sharded", extra=dict(extra, has_elite=0), p=icem, x0=x0, elite=elite, has_elite=False,
                keep_idx=None, out=out, seed=7, plan_id=8, **kw)[0] is out


# ---- PlaNet ---------------------------------------------------------------------------------------------------------------------
LAT, BEL, FCS = 2, 3, 4


def planet_spec():
    shapes = {"w_embed": (BEL, LAT + ACT), "b_embed": (BEL,), "w_ih": (3 * BEL, BEL), "b_ih": (3 * BEL,), "w_hh": (3 * BEL, BEL), "b_hh": (3 * BEL,),
              "w_prior1": (FCS, BEL), "b_prior1": (FCS,), "w_prior2": (2 * LAT, FCS), "b_prior2": (2 * LAT,), "w_rew1": (FCS, BEL + LAT),
              "b_rew1": (FCS,), "w_rew2": (FCS, FCS), "b_rew2": (FCS,), "w_rew3": (1, FCS), "b_rew3": (1,)}
    return PlaNetSpec(min_std=0.2, **{n: t(*s) for n, s in shapes.items()})


def test_planet_model_rollout_and_plans(eng):
    spec = planet_spec()
    eng.planet_set_model(spec)
    rec = take(eng, "hipets_planet_set_model")
    check(rec, "hipets_planet_set_model", d=ANY)
    assert eng.planet_spec is spec
    assert rec["d"] == opts_want(_lib.PlanetDesc, latent_size=LAT, action_size=ACT, belief_size=BEL, hidden_size=FCS, min_std=f32(0.2),
                                 **{n: getattr(spec, n) for n in _lib._PLANET_TENSORS})
    assert len({rec["d"][n] for n in _lib._PLANET_TENSORS}) == 16
    actions, lat, bel = t(POP, H, ACT), t(LAT), t(1, BEL)
    extra = {"pop": POP, "horizon": H, "opts": ANY, "returns": ANY}
    res, rec = call(eng, "planet_rollout", "hipets_planet_rollout", extra=extra, actions=actions, latent0=lat, belief0=bel, num_particles=P,
                    seed=-1, stream_id=U64 + 1)
    assert res.shape == (POP,) and res.dtype == torch.float32 and res.data_ptr() == rec["returns"]
    assert rec["opts"] == opts_want(_lib.PlanetOpts, seed=U64 - 1, stream_id=1, n_env=1)
    eps, tl, tb, tr, pc, out = t(H, B, LAT), t(H, B, LAT), t(H, B, BEL), t(H, B), t(8, 16, dtype=torch.int64), t(POP)
    lat2, bel2 = t(2, LAT), t(2, BEL)
    res, rec = call(eng, "planet_rollout", "hipets_planet_rollout", extra=dict(extra, returns=out), actions=actions, latent0=lat2, belief0=bel2,
                    num_particles=P, eps=eps, sample=False, trace_latent=tl, trace_belief=tb, trace_rewards=tr, phase_cycles=pc, out=out, n_env=2)
    assert res is out and rec["opts"] == opts_want(_lib.PlanetOpts, eps=eps, no_sample=1, trace_latent=tl, trace_belief=tb, trace_rewards=tr,
                                                   phase_cycles=pc, n_env=2)
    cem = Engine.cem_params(8, H, ACT, 2, 3, 0.1)
    icem = _lib.IcemParams(population_size=8, horizon=H, act_dim=ACT, num_iterations=2, elite_num=3, keep_elite_size=2, alpha=0.1)
    lo, hi = t(H, ACT), t(H, ACT)
    # x0 [H, A] and one environment: the un-batched symbol; anything else the batched one
    x0 = t(H, ACT)
    res, rec = call(eng, "plan_planet_cem", "hipets_plan_planet_cem", extra={"out": ANY}, p=cem, x0=x0, lower=lo, upper=hi, latent0=lat, belief0=bel,
                    num_particles=P, seed=-1, plan_id=U64 + 2)
    assert res.shape == (H, ACT) and res.data_ptr() == rec["out"] and (rec["seed"], rec["plan_id"]) == (U64 - 1, 2)
    x1, out1 = t(1, H, ACT), t(1, H, ACT)
    res, _ = call(eng, "plan_planet_cem", "hipets_plan_planet_cem_batched", p=cem, x0=x1, lower=lo, upper=hi, latent0=lat, belief0=bel,
                  num_particles=P, seed=1, plan_id=2, out=out1, n_env=1)
    assert res is out1
    x2, mean2, elite2, keep2 = t(2, H, ACT), t(2, H, ACT), t(2, 3, H, ACT), t(2, 2, 2, dtype=torch.int32)
    res, rec = call(eng, "plan_planet_cem", "hipets_plan_planet_cem_batched", extra={"out": ANY}, p=cem, x0=x2, lower=lo, upper=hi, latent0=lat2,
                    belief0=bel2, num_particles=P, seed=1, plan_id=2, n_env=2)
    assert res.shape == (2, H, ACT) and res.data_ptr() == rec["out"]
    res, rec = call(eng, "plan_planet_mppi", "hipets_plan_planet_mppi_batched", MPPI, pop=8, H=H, A=ACT, num_iterations=2, gamma=0.9, beta=0.25,
                    mean=mean2, lower=lo, upper=hi, latent0=lat2, belief0=bel2, num_particles=P, seed=-5, plan_id=6, n_env=2)
    assert res is mean2 and rec["seed"] == U64 - 5
    res, rec = call(eng, "plan_planet_icem", "hipets_plan_planet_icem_batched", extra={"out": ANY, "has_elite": 1}, p=icem, x0=x2, lower=lo, upper=hi,
                    elite=elite2, has_elite=True, latent0=lat2, belief0=bel2, num_particles=P, seed=5, plan_id=6, keep_idx=keep2, n_env=2)
    assert res.shape == (2, H, ACT) and res.data_ptr() == rec["out"]


# ---- the trainer and the plan trace ---------------------------------------------------------------------------------------------
def test_train_desc_with_and_without_adam(eng):
    N, out, mb = 10, OBS, 4
    like = lambda ts: [torch.zeros_like(x) for x in ts]  # noqa: E731
    ws, bs = [t(E, 5, HID), t(E, HID, HID), t(E, HID, 2 * out)], [t(E, 1, HID), t(E, 1, HID), t(E, 1, 2 * out)]
    m, v, lo, hi = (like(ws), like(bs)), (like(ws), like(bs)), t(1, out), t(1, out)
    x, y, idx, rows = t(N, 5), t(N, out), t(2, E, mb, dtype=torch.int32), t(2, dtype=torch.int32)
    ptrs = lambda ts: [a.data_ptr() for a in ts]  # noqa: E731
    base = dict(ensemble_size=E, n_layers=3, in_dim=5, hid=HID, out_dim=out, activation=_lib.ACT["tanh"], leaky_slope=f32(0.03), weights=ptrs(ws),
                biases=ptrs(bs), exp_avg_w=None, exp_avg_b=None, exp_avg_sq_w=None, exp_avg_sq_b=None)
    (loss, gsq), rec = call(eng, "train_steps", "hipets_train_steps", extra={"d": ANY, "n_rows": N, "n_steps": 2, "loss": ANY, "grad_sq": ANY},
                            weights=ws, biases=bs, exp_avg=m, exp_avg_sq=v, min_logvar=lo, max_logvar=hi, x=x, y=y, idx=idx, rows=rows, step0=2**40,
                            lr=1e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=5e-5, activation="tanh", leaky_slope=0.03, steps_per_launch=6)
    assert loss.shape == gsq.shape == (2, E) and loss.dtype == gsq.dtype == torch.float32 and (rec["loss"], rec["grad_sq"]) == (loss.data_ptr(), gsq.data_ptr())
    assert rec["d"] == opts_want(_lib.TrainDesc, **dict(base, max_batch=mb, exp_avg_w=ptrs(m[0]), exp_avg_b=ptrs(m[1]), exp_avg_sq_w=ptrs(v[0]),
                                                        exp_avg_sq_b=ptrs(v[1]), min_logvar=lo, max_logvar=hi, lr=1e-3, beta1=0.8, beta2=0.95, eps=1e-7,
                                                        weight_decay=5e-5, steps_per_launch=6))
    order = t(N, dtype=torch.int32)
    score, rec = call(eng, "train_eval", "hipets_train_eval", extra={"d": ANY, "n_rows": N, "score": ANY, "row_score": None}, weights=ws, biases=bs, x=x, y=y,
                      order=None, activation="tanh", leaky_slope=0.03)
    assert score.shape == (E,) and score.dtype == torch.float32 and rec["score"] == score.data_ptr()
    assert rec["d"] == opts_want(_lib.TrainDesc, **dict(base, max_batch=1))
    (score, rs), rec = call(eng, "train_eval", "hipets_train_eval", extra={"d": ANY, "n_rows": N, "score": ANY, "row_score": ANY}, weights=ws, biases=bs,
                            x=x, y=y, order=order, activation="tanh", leaky_slope=0.03, row_scores=True)
    assert rs.shape == (E, N) and (rec["score"], rec["row_score"]) == (score.data_ptr(), rs.data_ptr())


@pytest.mark.parametrize("n_env", [1, 2])
def test_plan_trace(eng, n_env):
    tr = eng.set_plan_trace(iters=2, max_rows=6, horizon=H, act_dim=ACT, elite_num=3, n_env=n_env)
    rec = take(eng, "hipets_set_plan_trace")
    env = () if n_env == 1 else (n_env,)
    assert {k: (tuple(v.shape), v.dtype) for k, v in tr.items()} == {
        "populations": ((2, 6, H, ACT), torch.float32), "values": ((2, 6), torch.float32), "mus": ((2, *env, H, ACT), torch.float32),
        "dispersions": ((2, *env, H, ACT), torch.float32), "elite_idx": ((2, *env, 3), torch.int32)}
    check(rec, "hipets_set_plan_trace", trace=opts_want(_lib.PlanTrace, max_rows=6, **tr))
    assert eng._trace is tr  # the engine keeps the buffers alive while the library holds their addresses
    assert eng.set_plan_trace(iters=0) is None and eng._trace is None
    check(take(eng, "hipets_set_plan_trace"), "hipets_set_plan_trace", trace=None)


# ---- every Python-side refusal, with its message, before any library call -------------------------------------------------------------
def refusals():
    """(label, exception type, message, engine -> the refused call)"""
    cem = Engine.cem_params(5, 3, 2, 4, 2, 0.1)
    icem = _lib.IcemParams(population_size=8, horizon=H, act_dim=ACT, num_iterations=2, elite_num=3, keep_elite_size=2, alpha=0.1)
    a, s0 = t(POP, H, ACT), np.zeros(OBS)
    lo, hi, x0 = t(H, ACT), t(H, ACT), t(H, ACT)
    cs = lambda e, **kw: e.cem_sample(**{**dict(p=cem, mu=t(3, 2), dispersion=t(3, 2), lower=t(3, 2), upper=t(3, 2), population=t(5, 3, 2)), **kw})  # noqa: E731
    cr = lambda e, **kw: e.cem_refit(**{**dict(p=cem, values=t(5), population=t(5, 3, 2), mu=t(3, 2), dispersion=t(3, 2), best_value=t(1),  # noqa: E731
                                               best_solution=t(3, 2)), **kw})
    ws, bs = [t(E, 5, HID), t(E, HID, 2 * OBS)], [t(E, 1, HID), t(E, 1, 2 * OBS)]
    td = lambda e, **kw: e.train_eval(**{**dict(weights=ws, biases=bs, x=t(4, 5), y=t(4, OBS)), **kw})  # noqa: E731
    adam = lambda e, **kw: e.train_steps(**{**dict(weights=ws, biases=bs, exp_avg=([t(E, 5, HID), t(E, HID, 2 * OBS)], [t(E, 1, HID), t(E, 1, 2 * OBS)]),  # noqa: E731
                                                   exp_avg_sq=([t(E, 5, HID), t(E, HID, 2 * OBS)], [t(E, 1, HID), t(E, 1, 2 * OBS)]), min_logvar=t(OBS),
                                                   max_logvar=t(OBS), x=t(4, 5), y=t(4, OBS), idx=t(2, E, 3, dtype=torch.int32), rows=t(2, dtype=torch.int32),
                                                   step0=0, lr=1e-3), **kw})
    V, Hp = ValueError, HipetsError
    no_model = "Engine.set_model() has not been called"
    return [
        # _check_dev: device, dtype, contiguity, shape, element count
        ("dev", V, "mu must be a tensor on cpu", lambda e: cs(e, mu=torch.zeros(3, 2, device="meta"))),
        ("not_tensor", V, "mu must be a tensor on cpu", lambda e: cs(e, mu=[0.0] * 6)),
        ("dtype", V, "dispersion must have dtype torch.float32, got torch.float64", lambda e: cs(e, dispersion=t(3, 2, dtype=torch.float64))),
        ("contig", V, "lower must be contiguous", lambda e: cs(e, lower=t(2, 3).t())),
        ("numel", V, "upper must have 6 elements, got 8", lambda e: cs(e, upper=t(4, 2))),
        ("z", V, "z must have 30 elements, got 6", lambda e: cs(e, z=t(3, 2))),
        ("shape", V, "values must have shape (5,), got (5, 1)", lambda e: cr(e, values=t(5, 1))),
        ("elite_idx", V, "elite_idx must have dtype torch.int32, got torch.int64", lambda e: cr(e, elite_idx=t(2, dtype=torch.int64))),
        ("elites_hi", V, "elites must index the population [0, 5): got 1 .. 5", lambda e: cr(e, elites=torch.tensor([5, 1], dtype=torch.int32))),
        ("elites_lo", V, "elites must index the population [0, 5): got -1 .. 2", lambda e: cr(e, elites=torch.tensor([2, -1], dtype=torch.int32))),
        ("icem_small", V, "population buffer too small", lambda e: e.icem_sample(5, 4, 2, 2.0, t(4, 2), t(4, 2), t(4, 2), t(4, 2), t(4, 4, 2))),
        ("icem_normals", V, "normals must have shape (2, 5, 2, 3), got (2, 5, 2, 2)",
         lambda e: e.icem_sample(5, 4, 2, 2.0, t(4, 2), t(4, 2), t(4, 2), t(4, 2), t(5, 4, 2), normals=t(2, 5, 2, 2))),
        ("comm_id", V, "unique_id must be 128 bytes", lambda e: e.comm_init(b"short", 0, 2)),
        ("plan_mode", V, "plan mode must be 'fast' or 'device'", lambda e: e.set_plan_mode("exact")),
        # rollout
        ("r_no_model", Hp, no_model, lambda e: (setattr(e, "spec", None), e.rollout(a, s0, P))),
        ("r_ndim", V, "action_sequences must be [B, H, A]", lambda e: e.rollout(t(POP, ACT), s0, P)),
        ("r_act", V, "action dim 3 != model act_dim 2", lambda e: e.rollout(t(POP, H, 3), s0, P)),
        ("r_s0", V, "initial_state has 4 values, expected n_env x obs_dim = 1 x 3", lambda e: e.rollout(a, np.zeros(4), P)),
        ("r_s0_env", V, "initial_state has 3 values, expected n_env x obs_dim = 2 x 3", lambda e: e.rollout(a, s0, P, n_env=2)),
        ("r_env_mode", V, "batched rollouts (n_env > 1) need mode='fast' or 'device' and a population divisible by n_env",
         lambda e: e.rollout(a, np.zeros(2 * OBS), P, n_env=2, mode="exact")),
        ("r_env_pop", V, "batched rollouts (n_env > 1) need mode='fast' or 'device' and a population divisible by n_env",
         lambda e: e.rollout(a, np.zeros(4 * OBS), P, n_env=4)),
        ("r_mode", V, "mode must be 'exact', 'fast' or 'device'", lambda e: e.rollout(a, s0, P, mode="quick")),
        ("r_device", V, "mode='device' draws its permutations and eps in-kernel: perms / eps / members must be None",
         lambda e: e.rollout(a, s0, P, mode="device", eps=t(H, B, OBS))),
        ("r_members_mode", V, "members= (explicit per-row member maps) is an EXACT-mode input, exclusive with perms=",
         lambda e: e.rollout(a, s0, P, mode="fast", members=t(H, B, dtype=torch.int64))),
        ("r_members_perms", V, "members= (explicit per-row member maps) is an EXACT-mode input, exclusive with perms=",
         lambda e: e.rollout(a, s0, P, mode="exact", members=t(H, B, dtype=torch.int64), perms=t(H, B, dtype=torch.int64))),
        ("r_members_shape", V, f"members must have shape ({H}, {B})", lambda e: e.rollout(a, s0, P, mode="exact", members=t(B, dtype=torch.int64))),
        ("r_perms_shape", V, f"perms must have shape ({H}, {B})", lambda e: e.rollout(a, s0, P, mode="exact", perms=t(B, dtype=torch.int64))),
        ("r_perms_dtype", V, "perms must have dtype torch.int64, got torch.int32", lambda e: e.rollout(a, s0, P, mode="exact", perms=t(H, B, dtype=torch.int32))),
        ("r_eps", V, f"eps must have shape ({H}, {B}, {OBS}), got ({H}, {B})", lambda e: e.rollout(a, s0, P, eps=t(H, B))),
        ("r_trace", V, f"trace_next_obs must have shape ({H}, {B}, {OBS}), got ({B}, {OBS})", lambda e: e.rollout(a, s0, P, trace_next_obs=t(B, OBS))),
        ("r_trace_r", V, f"trace_rewards must have shape ({H}, {B}), got ({B},)", lambda e: e.rollout(a, s0, P, trace_rewards=t(B))),
        ("r_phase", V, "phase_cycles must have shape (8, 16), got (8, 8)", lambda e: e.rollout(a, s0, P, phase_cycles=t(8, 8, dtype=torch.int64))),
        ("r_out", V, f"out must have shape ({POP},), got ({B},)", lambda e: e.rollout(a, s0, P, out=t(B))),
        # step
        ("s_no_model", Hp, no_model, lambda e: (setattr(e, "spec", None), e.step(t(B, OBS), t(B, ACT)))),
        ("s_obs", V, f"obs must have shape ({B}, {OBS}), got ({B}, 4)", lambda e: e.step(t(B, 4), t(B, ACT))),
        ("s_act", V, f"actions must have shape ({B}, {ACT}), got (3, {ACT})", lambda e: e.step(t(B, OBS), t(3, ACT))),
        ("s_mode", V, "mode must be 'exact', 'fast' or 'device'", lambda e: e.step(t(B, OBS), t(B, ACT), mode="quick")),
        ("s_device", V, "mode='device' draws its permutation and eps in-kernel", lambda e: e.step(t(B, OBS), t(B, ACT), mode="device", perm=t(B, dtype=torch.int64))),
        ("s_members", V, "members= must be int64 [B], exclusive with perm=", lambda e: e.step(t(B, OBS), t(B, ACT), mode="exact", members=t(1, B, dtype=torch.int64))),
        ("s_members_perm", V, "members= must be int64 [B], exclusive with perm=",
         lambda e: e.step(t(B, OBS), t(B, ACT), mode="exact", members=t(B, dtype=torch.int64), perm=t(B, dtype=torch.int64))),
        ("s_perm", V, f"perm must have shape ({B},), got (1, {B})", lambda e: e.step(t(B, OBS), t(B, ACT), mode="exact", perm=t(1, B, dtype=torch.int64), sample=False)),
        ("s_eps_missing", V, "EXACT step with sample=True needs eps [B, out_dim]", lambda e: e.step(t(B, OBS), t(B, ACT), mode="exact")),
        ("s_eps", V, f"eps must have {B * OBS} elements, got {B}", lambda e: e.step(t(B, OBS), t(B, ACT), mode="exact", eps=t(B))),
        ("s_fast_eps", V, f"eps must have {B * OBS} elements, got {B}", lambda e: e.step(t(B, OBS), t(B, ACT), eps=t(B))),
        ("s_sched", V, "member_schedule must have dtype torch.int32, got torch.int64", lambda e: e.step(t(B, OBS), t(B, ACT), member_schedule=t(4, dtype=torch.int64))),
        # trajectory_returns
        ("t_ndim", V, "rewards must be a [H, B] tensor", lambda e: e.trajectory_returns(t(B), t(B, dtype=torch.uint8), POP, P)),
        ("t_rows", V, "rewards holds 12 rows per step, pop x num_particles = 4 x 2", lambda e: e.trajectory_returns(t(H, B), t(H, B, dtype=torch.uint8), 4, 2)),
        ("t_dtype", V, "rewards must have dtype torch.float32, got torch.float64", lambda e: e.trajectory_returns(t(H, B, dtype=torch.float64), t(H, B, dtype=torch.uint8), POP, P)),
        ("t_dones", V, "dones must have dtype torch.uint8, got torch.float32", lambda e: e.trajectory_returns(t(H, B), t(H, B), POP, P)),
        ("t_dones_shape", V, f"dones must have shape ({H}, {B}), got ({B},)", lambda e: e.trajectory_returns(t(H, B), t(B, dtype=torch.bool), POP, P)),
        # the plans: the model, the tensors, the start state in the local and the sharded wording
        ("p_no_model", Hp, no_model, lambda e: (setattr(e, "spec", None), e.plan_cem(cem, x0, lo, hi, s0, P))),
        ("p_no_planet", Hp, "Engine.planet_set_model() has not been called", lambda e: e.plan_planet_cem(cem, x0, lo, hi, t(LAT), t(BEL), P)),
        ("pr_no_planet", Hp, "Engine.planet_set_model() has not been called", lambda e: e.planet_rollout(a, t(LAT), t(BEL), P)),
        ("p_x0", V, "x0 must have 6 elements, got 4", lambda e: e.plan_cem(cem, t(2, 2), lo, hi, s0, P)),
        ("p_lower", V, "lower must have shape (3, 2), got (6,)", lambda e: e.plan_cem(cem, x0, t(6), hi, s0, P)),
        ("p_s0", V, "initial_state has 4 values, expected 1 x 3", lambda e: e.plan_cem(cem, x0, lo, hi, np.zeros(4), P)),
        ("p_s0_env", V, "initial_state has 3 values, expected 2 x 3", lambda e: e.plan_mppi(8, H, ACT, 2, 0.9, 0.25, t(2, H, ACT), lo, hi, s0, P, n_env=2)),
        ("p_s0_sharded", V, "initial_state has 4 values, expected 3", lambda e: e.plan_cem_sharded(cem, x0, lo, hi, np.zeros(4), P)),
        ("p_s0_sharded_icem", V, "initial_state has 6 values, expected 3",
         lambda e: e.plan_icem_sharded(icem, x0, lo, hi, t(3, H, ACT), False, np.zeros(6), P)),
        ("p_x0_sharded", V, "x0 must have shape (3, 2), got (1, 3, 2)", lambda e: e.plan_cem_sharded(cem, t(1, H, ACT), lo, hi, s0, P)),
        ("p_mean_sharded", V, "mean must have shape (3, 2), got (6,)", lambda e: e.plan_mppi_sharded(8, H, ACT, 2, 0.9, 0.25, t(6), lo, hi, s0, P)),
        ("p_x0_sharded_icem", V, "x0 must have shape (3, 2), got (6,)", lambda e: e.plan_icem_sharded(icem, t(6), lo, hi, t(3, H, ACT), False, s0, P)),
        ("p_elite", V, "elite must have 18 elements, got 6", lambda e: e.plan_icem(icem, x0, lo, hi, t(H, ACT), False, s0, P)),
        ("p_keep", V, "keep_idx must have dtype torch.int32, got torch.float32", lambda e: e.plan_icem(icem, x0, lo, hi, t(3, H, ACT), False, s0, P, keep_idx=t(2, 2))),
        ("p_keep_n", V, "keep_idx must have 4 elements, got 2", lambda e: e.plan_icem(icem, x0, lo, hi, t(3, H, ACT), False, s0, P, keep_idx=t(2, dtype=torch.int32))),
        # the trainer
        ("d_layers", V, "weights / biases: one tensor of each per linear layer, at least 2 layers", lambda e: td(e, weights=ws[:1], biases=bs[:1])),
        ("d_pairs", V, "weights / biases: one tensor of each per linear layer, at least 2 layers", lambda e: td(e, biases=bs[:1])),
        ("d_w", V, f"weights[1] must have shape ({E}, {HID}, {2 * OBS}), got ({E}, {HID}, {OBS})", lambda e: td(e, weights=[ws[0], t(E, HID, OBS)])),
        ("d_b", V, f"biases[0] must have shape ({E}, 1, {HID}), got ({E}, {HID})", lambda e: td(e, biases=[t(E, HID), bs[1]])),
        ("d_act", V, "unknown activation 'gelu'", lambda e: td(e, activation="gelu")),
        ("d_xy", V, "x / y must be [N, in] / [N, out] with the same N", lambda e: td(e, y=t(5, OBS))),
        ("d_order", V, "order must have 4 elements, got 5", lambda e: td(e, order=t(5, dtype=torch.int32))),
        ("d_adam_len", V, "exp_avg_w: one tensor per layer", lambda e: adam(e, exp_avg=([t(E, 5, HID)], [t(E, 1, HID), t(E, 1, 2 * OBS)]))),
        ("d_adam_shape", V, f"exp_avg_sq_b[1] must have shape ({E}, 1, {2 * OBS}), got ({E}, 1, {OBS})",
         lambda e: adam(e, exp_avg_sq=([t(E, 5, HID), t(E, HID, 2 * OBS)], [t(E, 1, HID), t(E, 1, OBS)]))),
        ("d_logvar", V, f"min_logvar must have {OBS} elements, got 4", lambda e: adam(e, min_logvar=t(4))),
        ("d_idx", V, "idx must be [n_steps, E, max_batch]", lambda e: adam(e, idx=t(2, E, dtype=torch.int32))),
        ("d_members", V, f"idx has 2 members, the model {E}", lambda e: adam(e, idx=t(2, 2, 3, dtype=torch.int32))),
        ("d_rows", V, "rows must have 2 elements, got 3", lambda e: adam(e, rows=t(3, dtype=torch.int32))),
    ]


REFUSALS = refusals()


@pytest.mark.parametrize("label", [r[0] for r in REFUSALS])
def test_python_side_refusals_raise_before_the_library_call(eng, label):
    _, exc, message, refused = next(r for r in REFUSALS if r[0] == label)
    eng.set_model(make_spec())
    eng._lib.calls.clear()
    with pytest.raises(exc) as caught:
        refused(eng)
    assert str(caught.value) == message and type(caught.value) is exc
    assert eng._lib.calls == []


def test_planet_refusals(eng):
    eng.planet_set_model(planet_spec())
    eng._lib.calls.clear()
    for message, refused in (
            ("action_sequences must be [B, H, A]", lambda: eng.planet_rollout(t(POP, ACT), t(LAT), t(BEL), P)),
            ("action dim 3 != model action_size 2", lambda: eng.planet_rollout(t(POP, H, 3), t(LAT), t(BEL), P)),
            ("latent0 must have 4 elements, got 2", lambda: eng.planet_rollout(t(POP, H, ACT), t(LAT), t(2, BEL), P, n_env=2)),
            ("belief0 must have 3 elements, got 2", lambda: eng.planet_rollout(t(POP, H, ACT), t(LAT), t(2), P)),
            (f"eps must have shape ({H}, {B}, {LAT}), got ({H}, {B})", lambda: eng.planet_rollout(t(POP, H, ACT), t(LAT), t(BEL), P, eps=t(H, B))),
            (f"trace_belief must have shape ({H}, {B}, {BEL}), got ({H}, {B})",
             lambda: eng.planet_rollout(t(POP, H, ACT), t(LAT), t(BEL), P, trace_belief=t(H, B))),
            (f"out must have shape ({POP},), got (1,)", lambda: eng.planet_rollout(t(POP, H, ACT), t(LAT), t(BEL), P, out=t(1))),
            ("latent0 must have 2 elements, got 3",
             lambda: eng.plan_planet_cem(Engine.cem_params(8, H, ACT, 2, 3, 0.1), t(H, ACT), t(H, ACT), t(H, ACT), t(3), t(BEL), P))):
        with pytest.raises(ValueError) as caught:
            refused()
        assert str(caught.value) == message
    assert eng._lib.calls == []


def test_the_call_path_refuses_a_wrong_parameter_name(eng):
    """A missing or unknown header parameter name is a TypeError before the C call"""
    with pytest.raises(TypeError):
        eng._call("hipets_gather_rows", rows=1, dim=1, src=None, index=None, out=None)  # the header says dst
    with pytest.raises(TypeError):
        eng._call("hipets_gather_rows", rows=1, dim=1, src=None, index=None)
    assert eng._lib.calls == []
