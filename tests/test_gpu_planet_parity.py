"""The PlaNet latent rollout kernel (planet.hpp) per step against an f64 evaluation of the oracle (tests/planet_f64.py), at the edges of
its segment layout, on the STATIC instance away from conf's exact dimensions, with saturated GRU gates and both softplus branches, at
the widest row that fits LDS, and every refusal of the C ABI's PlaNet entry points.  Every call goes through Engine.planet_set_model /
planet_rollout (the refusals the Python wrapper would catch first: the raw C ABI).  What the comparisons rest on -- the f32 oracle within a
fifth of T1 of f64, the saturation, the tail-length coverage -- is checked on the CPU in tests/test_planet_f64_host.py."""
import ctypes as C

import pytest
import torch

import hipets
import planet_f64 as pf
from hipets import _lib
from test_gpu_planet import engine_normals, to_planet_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("returns", "latent", "belief", "rewards")
MODES = ("eps", "mean", "philox")
SEED, STREAM = 11, 3


def ident(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def gpu_traced(engine, actions, latent0, belief0, P, mode, eps, n_env=1):
    """One Engine.planet_rollout with all three taps: (returns, latent [H, B, L], belief [H, B, Hb], rewards [H, B]) on the CPU."""
    pop, H, _ = actions.shape
    B, L, Hb = pop * P, latent0.shape[-1], belief0.shape[-1]
    tl, tb, tr = torch.zeros(H, B, L, device=DEV), torch.zeros(H, B, Hb, device=DEV), torch.zeros(H, B, device=DEV)
    kw = {"eps": eps.to(DEV)} if mode == "eps" else {"sample": False} if mode == "mean" else {"seed": SEED, "stream_id": STREAM}
    out = engine.planet_rollout(actions.to(DEV), latent0.to(DEV).contiguous(), belief0.to(DEV).contiguous(), P, trace_latent=tl, trace_belief=tb,
                                trace_rewards=tr, n_env=n_env, **kw)
    return tuple(t.cpu() for t in (out, tl, tb, tr))


def reference_eps(engine, mode, eps):
    """The draws the f64 reference is fed: the injected ones, zeros for sample=False, the kernel's own exported Philox normals."""
    if mode == "eps":
        return eps
    if mode == "mean":
        return torch.zeros_like(eps)
    # (normal d of (row, step) does not depend on how many are drawn; the exporting PETS model wants at least 3 observation dims)
    got = engine_normals(engine, eps.shape[0], eps.shape[1], max(eps.shape[2], 3), SEED, STREAM)[..., :eps.shape[2]].contiguous()
    assert got.shape == eps.shape and torch.isfinite(got).all()
    return got


def assert_t1(got, ref, what):
    for name, a, b in zip(NAMES, got, ref):
        assert torch.isfinite(a).all(), (what, name)
        x = pf.t1_excess(a, b)
        assert x <= 1.0, f"{what} {name}: max |gpu - f64| = {(a.double() - b).abs().max():.3e}, {x:.2f} x T1"


def parity_all_modes(engine, dims, H, P=2):
    """Per-step parity with f64 under T1 in the three modes; returns the GPU results per mode.  The model must be set already."""
    pm, actions, latent0, belief0, eps = pf.free_case(dims, H)
    pm64 = pf.to_f64(pm)
    out = {}
    for mode in MODES:
        out[mode] = gpu_traced(engine, actions, latent0, belief0, P, mode, eps)
        ref = pf.rollout_traced(pm64, actions, latent0, belief0, P, reference_eps(engine, mode, eps))
        assert_t1(out[mode], ref, f"{dims} {mode}")
    assert not torch.equal(out["eps"][1], out["philox"][1]) and not torch.equal(out["eps"][1], out["mean"][1])  # three different rollouts
    return out


# ---- a. per-step parity at the edges of the segment layout (generic instance) ------------------------------------------------
@pytest.mark.parametrize("dims", pf.EDGE_SHAPES, ids=ident)
def test_per_step_parity_at_shape_edges(engine, dims):
    """38 rows (two full row tiles and a ragged one of 6), H 8: latent, belief and reward at EVERY step and the returns against f64 under
    T1, with injected eps, with sample=False and with the in-kernel Philox draws."""
    pm = pf.free_case(dims, 8)[0]
    engine.planet_set_model(to_planet_spec(pm))
    assert engine.planet_kernel_class() == "generic"
    parity_all_modes(engine, dims, 8)


# ---- b. models near conf: the STATIC instance away from conf's own dimensions -----------------------------------------------
@pytest.mark.parametrize("dims", pf.STATIC_SHAPES, ids=ident)
def test_static_instance_near_conf(engine, monkeypatch, dims):
    """The STATIC instance is selected by tile counts and row stride: these models run it with tail lengths, widths and padding other than
    conf's.  It is what runs, it gives the generic instance's bits in all three modes, and both sit within T1 of f64 at every step."""
    assert pf.runs_static(dims)
    pm = pf.free_case(dims, 4)[0]
    engine.planet_set_model(to_planet_spec(pm))
    assert engine.planet_kernel_class() == "static"
    static = parity_all_modes(engine, dims, 4)
    monkeypatch.setenv("HIPETS_PLANET_GENERIC", "1")
    assert engine.planet_kernel_class() == "generic"
    generic = parity_all_modes(engine, dims, 4)
    for mode in MODES:
        for name, a, b in zip(NAMES, static[mode], generic[mode]):
            assert torch.equal(a, b), (mode, name)


@pytest.mark.parametrize("dims", pf.NEAR_SHAPES, ids=ident)
def test_one_tile_off_conf_runs_the_generic_instance(engine, dims):
    """Conf's row stride with one op one column tile wider: not the STATIC instance's shapes."""
    assert pf.row_floats(dims) == pf.row_floats(pf.CONF) and not pf.runs_static(dims)
    pm = pf.free_case(dims, 4)[0]
    engine.planet_set_model(to_planet_spec(pm))
    assert engine.planet_kernel_class() == "generic"
    parity_all_modes(engine, dims, 4)


# ---- c. saturated gates and both softplus branches, one step ----------------------------------------------------------------
# The bound per tensor is the larger of T1 and SATURATED_MARGIN x e32, e32 = the f32 oracle's own largest deviation from f64 for that
# tensor and case (computed below on the CPU).  The margin covers the MFMA's summation order and ~1e-7 absolute per hardware
# transcendental: the smallest power of two that covers the ratios measured on the MI355X with a factor of two to spare.
#   max |gpu - f64| / e32        belief   latent   reward      (e32: belief 4e-6 .. 6e-6, latent 2e-5 .. 5e-5 at |latent| up to 120,
#   30x6x200x200 (STATIC)        1.19     1.30     1.52         reward 2e-4 .. 5e-4 at |reward| up to 1200)
#   7x2x22x19                    0.39     0.51     0.72
#   17x15x33x65                  0.77     0.64     0.55
# Largest 1.52, twice that 3.04: 4.
SATURATED_MARGIN = 4


@pytest.mark.parametrize("dims", pf.SATURATED_SHAPES, ids=ident)
def test_saturated_gates_and_both_softplus_branches(engine, dims):
    """One step of a scale-4 model from |latent| ~ 3, belief at the rails, raw std biased over [-30, 30]: sigmoid_hw / tanh_hw at large
    arguments, softplus_fast beyond 20 and where log(1 + exp(x)) flushes to 0.  48 rows, one environment each: a tile straddles 16."""
    rows = 48
    pm, actions, latent0, belief0, eps = pf.saturated_case(dims, rows)
    engine.planet_set_model(to_planet_spec(pm))
    _, tl, tb, tr = gpu_traced(engine, actions, latent0, belief0, 1, "eps", eps, n_env=rows)
    ref64 = pf.step_traced(pf.to_f64(pm), actions, latent0, belief0, eps)
    ref32 = pf.step_traced(pm, actions, latent0, belief0, eps)
    failed = []
    for name, got, b64, b32 in zip(("latent", "belief", "reward"), (tl[0], tb[0], tr[0]), ref64, ref32):
        assert torch.isfinite(got).all(), name
        e32 = (b32.double() - b64).abs().max().item()
        err = (got.double() - b64).abs()
        print(f"saturated {ident(dims)} {name}: e32 = {e32:.3e}, max |gpu - f64| = {err.max():.3e}, ratio {err.max() / e32:.2f}, "
              f"{pf.t1_excess(got, b64):.2f} x T1, max |f64| = {b64.abs().max():.1f}")
        lim = torch.clamp(pf.T1["atol"] + pf.T1["rtol"] * b64.abs(), min=SATURATED_MARGIN * e32)
        if not (err <= lim).all():
            failed.append((name, err.max().item(), e32))
    assert not failed, failed


# ---- d. the LDS limit and the refusals ---------------------------------------------------------------------------------------
def device_lds_bytes():
    p = torch.cuda.get_device_properties(0)
    return min(int(getattr(p, "shared_memory_per_block_optin", 0) or pf.LDS_BYTES), pf.LDS_BYTES)  # the library opts in to at most 160 KB


def good_rollout(engine, dims=(7, 2, 22, 19), set_model=False):
    """The engine's (7, 2, 22, 19) model -- set before a refusal, NOT again after it -- still rolls out within T1 of f64."""
    pm, actions, latent0, belief0, eps = pf.free_case(dims, 2)
    if set_model:
        engine.planet_set_model(to_planet_spec(pm))
    ref = pf.rollout_traced(pf.to_f64(pm), actions, latent0, belief0, 2, eps)
    assert_t1(gpu_traced(engine, actions, latent0, belief0, 2, "eps", eps), ref, "after a refusal")


def test_widest_model_that_fits_lds_and_the_first_that_does_not(engine):
    """The profiler's accumulators sit in the last 512 bytes of the dynamic LDS: the widest admissible row is where a layout off by one
    shows.  Both models come from the restated formula; the wider one is refused and leaves the engine's model alone."""
    fits, refused = pf.widest_square_models(device_lds_bytes())
    assert pf.smem_bytes(pf.row_floats(fits)) <= device_lds_bytes() < pf.smem_bytes(pf.row_floats(refused))
    pm = pf.free_case(fits, 2)[0]
    engine.planet_set_model(to_planet_spec(pm))
    assert engine.planet_kernel_class() == "generic"
    parity_all_modes(engine, fits, 2)
    with pytest.raises(hipets.HipetsError, match=f"too wide for LDS \\(row of {pf.row_floats(refused)} floats\\)"):
        engine.planet_set_model(to_planet_spec(pf.free_case(refused, 2)[0]))
    parity_all_modes(engine, fits, 2)  # the refused model replaced nothing


def raw_desc(pm, **override):
    """hipets_planet_desc of a model on the device, with dimensions overridden; returns (desc, tensors to keep alive)."""
    d = _lib.PlanetDesc()
    d.latent_size, d.action_size, d.belief_size, d.hidden_size = pm.latent_size, pm.action_size, pm.belief_size, pm.hidden_size
    d.min_std = pm.min_std
    keep = [getattr(pm, n).to(DEV).contiguous() for n in _lib._PLANET_TENSORS]
    for n, t in zip(_lib._PLANET_TENSORS, keep):
        setattr(d, n, t.data_ptr())
    for k, v in override.items():
        setattr(d, k, v)
    return d, keep


def raw_rollout(engine, handle, pop, P, H, A, L, Hb, n_env):
    """hipets_planet_rollout as a C client calls it (the Python wrapper checks some of these arguments itself)."""
    o = _lib.PlanetOpts()
    o.no_sample, o.n_env = 1, n_env
    rows = max(n_env, 1)
    bufs = [torch.zeros(pop, H, A, device=DEV), torch.zeros(rows, L, device=DEV), torch.zeros(rows, Hb, device=DEV), torch.zeros(pop, device=DEV)]
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = engine._lib.hipets_planet_rollout(handle, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), pop, H, P, C.byref(o),
                                           bufs[3].data_ptr(), stream)
    torch.cuda.synchronize()
    _lib.check(rc)


@pytest.mark.parametrize("field,value", [("latent_size", 0), ("action_size", 0), ("belief_size", -3), ("hidden_size", 0)])
def test_bad_dimensions_are_refused(engine, field, value):
    good_rollout(engine, set_model=True)
    d, keep = raw_desc(pf.free_case((7, 2, 22, 19), 2)[0], **{field: value})
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    with pytest.raises(hipets.HipetsError, match="bad PlaNet dimensions"):
        _lib.check(engine._lib.hipets_planet_set_model(engine._h, C.byref(d), stream))
    del keep
    good_rollout(engine)


@pytest.mark.parametrize("n_env", [-1, 4097])
def test_n_env_out_of_range_is_refused(engine, n_env):
    good_rollout(engine, set_model=True)
    with pytest.raises(hipets.HipetsError, match=f"n_env {n_env} outside \\[0, 4096\\]"):
        raw_rollout(engine, engine._h, max(n_env, 1), 1, 2, 2, 7, 22, n_env)
    good_rollout(engine)


def test_batch_too_large_is_refused_before_anything_is_allocated(engine):
    """pop 1 with 2**27 particles: 2**27 rows x max(belief, 16) columns pass the int32 indices of the traces."""
    good_rollout(engine, set_model=True)
    free_before = torch.cuda.mem_get_info()[0]
    z = torch.zeros(1, 2, 2, device=DEV)
    with pytest.raises(hipets.HipetsError, match="batch too large"):
        engine.planet_rollout(z, torch.zeros(1, 7, device=DEV), torch.zeros(1, 22, device=DEV), 2 ** 27, sample=False)
    assert free_before - torch.cuda.mem_get_info()[0] < 2 ** 27  # (the 2**27 x 4-byte totals buffer was never asked for)
    good_rollout(engine)


def test_engine_without_a_planet_model_refuses_rollout_and_query(engine):
    good_rollout(engine, set_model=True)
    fresh = hipets.Engine(DEV)
    try:
        with pytest.raises(hipets.HipetsError, match="engine has no PlaNet model"):
            fresh.planet_kernel_class()
        with pytest.raises(hipets.HipetsError, match="engine has no PlaNet model"):
            raw_rollout(fresh, fresh._h, 4, 1, 2, 2, 7, 22, 1)
        with pytest.raises(hipets.HipetsError, match="planet_set_model"):  # the wrapper's own refusal, ahead of the library's
            fresh.planet_rollout(torch.zeros(4, 2, 2, device=DEV), torch.zeros(1, 7, device=DEV), torch.zeros(1, 22, device=DEV), 1)
        good_rollout(fresh, set_model=True)  # the refusals left the fresh engine usable
    finally:
        fresh.close()
    good_rollout(engine)
