"""hipets.DeviceReplayBuffer on the GPU: the ring compaction (hipets_ring_compact_transitions) against the restatement's add_batch over
the same kept rows, the gather (hipets_replay_gather) against pack_sac_batch on the host copy of the same storage, the populate into a
device buffer against the populate into a host buffer, SACUpdater.update_many from device buffers against host buffers, and
maybe_replace_sac_buffer.  Everything here is a copy: every comparison is bitwise, there are no tolerances."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import hipets
import policy_restatement as pr
import replay_restatement as rr
import sac_restatement as sr
from conftest import GOLDEN, to_spec
from hipets import _lib, mbpo
from test_gpu_mbpo_populate import ACT, L, OBS, hopper_model, initial_obs
from test_gpu_policy import BarePolicy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rows_of(g, n, od, ad, p_done=0.3):
    return (g.standard_normal((n, od)).astype(np.float32), g.standard_normal((n, ad)).astype(np.float32),
            g.standard_normal((n, od)).astype(np.float32), g.standard_normal(n).astype(np.float32), g.random(n) < p_done, np.zeros(n, dtype=bool))


def pair_of_buffers(engine, capacity, od, ad, n, seed, data_seed=1):
    """A device buffer and the host restatement with equal rows and equal-seeded generators of their own"""
    rows = rows_of(np.random.default_rng(data_seed), n, od, ad)
    dev = hipets.DeviceReplayBuffer(capacity, (od,), (ad,), rng=np.random.default_rng(seed), engine=engine)
    host = rr.HostRingBuffer(capacity, (od,), (ad,), rng=np.random.default_rng(seed))
    dev.add_batch(*rows)
    host.add_batch(*rows)
    return dev, host


# ---- 1. the ring compaction ------------------------------------------------------------------------------------------------------
RING_CASES = [  # name, N, capacity, cur_idx at the start, (obs, act), share of rows done before the first step, share done per step
    ("n1", 1, 5, 4, (11, 3), 0.0, 0.0),
    ("n48_c48_exact_laps", 48, 48, 0, (11, 3), 0.0, 0.0),
    ("n48_c72", 48, 72, 40, (11, 3), 0.25, 0.3),
    ("n48_c72_o1_a1", 48, 72, 60, (1, 1), 0.25, 0.3),
    ("n257_c385_at300", 257, 385, 300, (11, 3), 0.0, 0.3),
    ("n257_c385_at300_o17_a6", 257, 385, 300, (17, 6), 0.0, 0.3),
    ("n300_c300_at299", 300, 300, 299, (11, 3), 0.0, 0.3),
    ("n48_all_done_before", 48, 72, 70, (11, 3), 1.0, 0.3),
]


def sentinel_ring(engine, capacity, od, ad, cur_idx):
    """A device buffer whose storage holds a pattern no transition holds, with its cursor at ``cur_idx``; and the restatement over a
    host copy of that storage (its arrays ARE views of the copy, the done flags as the floats the ring stores)"""
    dev = hipets.DeviceReplayBuffer(capacity, (od,), (ad,), engine=engine)
    dev.storage.copy_(-1000.0 - torch.arange(dev.storage.numel(), dtype=torch.float32) % 977)
    dev._set_cursor(cur_idx, cur_idx)
    flat = dev.storage.cpu().numpy().copy()
    host = rr.HostRingBuffer(1, (od,), (ad,))
    host.capacity, host.cur_idx, host.num_stored = capacity, cur_idx, cur_idx
    host.obs, host.action, host.next_obs, host.reward, host.terminated = mbpo.staging_views(flat, capacity, od, ad)
    host.truncated = np.zeros(capacity, dtype=bool)
    return dev, host, flat


@pytest.mark.parametrize("name,N,cap,cur0,dims,p_before,p_done", RING_CASES, ids=[c[0] for c in RING_CASES])
def test_ring_compaction_is_add_batch_over_the_kept_rows(engine, name, N, cap, cur0, dims, p_before, p_done):
    od, ad = dims
    dev, host, flat = sentinel_ring(engine, cap, od, ad, cur0)
    g = np.random.default_rng(N * 1000 + cap)
    accum = g.random(N) < p_before
    accum_t = torch.from_numpy(accum.astype(np.uint8)).to(DEV)
    count = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    wrapped, total = False, 0
    for step in range(3):  # three steps in a row on one cursor
        o, a, no, r, d, _ = rows_of(g, N, od, ad, p_done)
        keep = ~accum
        before = host.cur_idx
        host.add_batch(o[keep], a[keep], no[keep], r[keep], d[keep], np.zeros(int(keep.sum()), dtype=bool))
        wrapped |= before + int(keep.sum()) >= cap
        total += int(keep.sum())
        engine.ring_compact_transitions(*(torch.from_numpy(v).to(DEV) for v in (o, a, no)), torch.from_numpy(r).to(DEV).reshape(N, 1),
                                        torch.from_numpy(d).to(DEV).reshape(N, 1), accum_t, dev.storage, cap, dev.cursor, count)
        accum |= d
        assert int(count) == int(keep.sum()), f"{name}: count_out of step {step}"
        assert dev.cursor.tolist() == [host.cur_idx, host.num_stored], f"{name}: cursor after step {step}"
        assert np.array_equal(accum_t.cpu().numpy() != 0, accum), f"{name}: accum_dones after step {step}"
        got = dev.storage.cpu().numpy()
        for key, x, y in zip(("obs", "action", "next_obs", "reward", "done"), mbpo.staging_views(got, cap, od, ad), mbpo.staging_views(flat, cap, od, ad)):
            assert np.array_equal(bits(x), bits(y)), f"{name}: {key} after step {step}"  # (the untouched rows keep the pattern)
    assert dev.sync() is dev and (dev.cur_idx, dev.num_stored) == (host.cur_idx, host.num_stored)
    print(f"{name}: cursor {cur0} -> {host.cur_idx}, stored {host.num_stored} of {cap}; wrapped {wrapped}")
    if p_before == 1.0:
        assert (host.cur_idx, host.num_stored) == (cur0, cur0) and (flat < -999).all()  # kept = 0: nothing moved
    else:
        assert wrapped, "the case was written to pass the end of the ring"
        assert (flat < -999).any() == (total < cap)  # (fewer rows written than the ring has: some still hold the pattern)


def test_ring_compaction_refuses_a_step_larger_than_the_ring(engine):
    N, cap, od, ad = 9, 8, 3, 2
    dev, _, flat = sentinel_ring(engine, cap, od, ad, 2)
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=DEV)  # noqa: E731
    with pytest.raises(hipets.HipetsError) as exc:
        engine.ring_compact_transitions(z(N, od), z(N, ad), z(N, od), z(N), z(N, dtype=torch.uint8), z(N, dtype=torch.uint8), dev.storage, cap,
                                        dev.cursor, z(1, dtype=torch.int32))
    assert exc.value.kind == _lib.ERR_INVALID_ARGUMENT
    assert dev.cursor.tolist() == [2, 2] and np.array_equal(bits(dev.storage.cpu().numpy()), bits(flat))


# ---- 2. the gather ---------------------------------------------------------------------------------------------------------------
GATHER_CAP = 97


@pytest.fixture(scope="module", params=[(1, 1), (11, 3), (376, 17)], ids=["w5", "w27", "w771"])
def gather_pair(engine, request):
    od, ad = request.param
    return pair_of_buffers(engine, GATHER_CAP, od, ad, GATHER_CAP, seed=0, data_seed=od)


def some_indices(n):
    idx = np.random.default_rng(n).integers(0, GATHER_CAP, size=n)
    idx[-1] = GATHER_CAP - 1
    if n >= 4:
        idx[0], idx[1], idx[2] = 0, 40, 40
    return idx


@pytest.mark.parametrize("n_rows", [1, 256, 1000])
def test_gather_is_pack_sac_batch_of_the_host_copy(engine, gather_pair, n_rows):
    dev, host = gather_pair
    assert dev.width == 2 * dev.obs_dim + dev.act_dim + 2 and host.terminated.any() and not host.terminated.all()
    idx = some_indices(n_rows)
    for reverse in (False, True):
        want = mbpo.pack_sac_batch(host._batch_from_indices(idx).astuple(), reverse)
        for given in (idx, torch.from_numpy(idx).to(DEV)):  # host indices (checked and uploaded by the engine), device indices
            got = dev.gather(given, reverse_mask=reverse)
            assert got.shape == (n_rows, dev.width) and np.array_equal(bits(got.cpu().numpy()), bits(want)), (n_rows, reverse)
        mask = want[:, -1]
        assert set(np.unique(mask)) <= {0.0, 1.0} and np.array_equal(mask != 0, host.terminated[idx] != reverse)


def test_gather_turns_an_index_outside_the_ring_into_a_row_of_nan(engine, gather_pair):
    dev, host = gather_pair
    idx = some_indices(256)
    want = mbpo.pack_sac_batch(host._batch_from_indices(idx).astuple(), True)
    bad = idx.copy()
    bad[17], bad[200] = GATHER_CAP, -1
    got = dev.gather(torch.from_numpy(bad).to(DEV), reverse_mask=True).cpu().numpy()  # no error is raised
    torch.cuda.synchronize()
    assert np.isnan(got[[17, 200]]).all()
    ok = np.ones(256, dtype=bool)
    ok[[17, 200]] = False
    assert np.array_equal(bits(got[ok]), bits(want[ok]))
    with pytest.raises(ValueError, match="indices must be integers"):
        dev.gather(bad)  # the same indices from the host are refused before anything is launched


def test_device_buffer_on_the_gpu_is_the_recorded_run_of_the_reference(engine):
    """tests/golden/replay_buffer_cases.npz (the reference's own buffer over replay_restatement's script): add / add_batch as slice
    copies on the device, sample / get_all(shuffle) through the gather kernel, save / load, growth and shrink device to device"""
    gold = dict(np.load(os.path.join(GOLDEN, "replay_buffer_cases.npz")))
    rec, bufs = rr.run_script(lambda cap, o, a, rng=None: hipets.DeviceReplayBuffer(cap, o, a, rng=rng, engine=engine),
                              lambda *a: hipets.maybe_replace_sac_buffer(*a, engine=engine))
    assert sorted(rec) == sorted(gold) and all(b.device.type == "cuda" for b in bufs.values())
    for k, want in gold.items():
        got = np.asarray(rec[k])
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert np.array_equal(bits(got), bits(want)) if want.dtype == np.float32 else np.array_equal(got, want), k


# ---- 3. the populate ---------------------------------------------------------------------------------------------------------------
POPULATE_CASES = [("n1", 1, "random_model", False), ("n48", 48, "random_model", False), ("n48_wraps", 48, "random_model", True),
                  ("n257_wraps", 257, "fixed_model", True)]


@pytest.mark.parametrize("name,N,prop,wraps", POPULATE_CASES, ids=[c[0] for c in POPULATE_CASES])
def test_populate_into_a_device_buffer_equals_populate_into_a_host_buffer(engine, name, N, prop, wraps):
    spec = to_spec(hopper_model(prop, None if N % 3 == 0 else [1]), OBS, ACT)
    w, _, _ = pr.make_case("populate", OBS, 64, ACT)
    policy = BarePolicy(w)
    first = initial_obs(N, seed=N)
    cap = N + N // 2 if wraps else 3 * N + 5
    results = []
    for on_device in (True, False):
        torch.manual_seed(3)
        env = hipets.ModelEnv(spec, engine=engine, mode="device", seed=13, generator=torch.Generator().manual_seed(7))
        source = pr.MiniReplayBuffer(N, OBS, ACT, first)
        sac = hipets.DeviceReplayBuffer(cap, (OBS,), (ACT,), engine=engine) if on_device else pr.MiniReplayBuffer(cap, OBS, ACT)
        hipets.rollout_model_and_populate_sac_buffer(env, source, hipets.SACActor(policy, engine=engine, seed=0), sac, True, L, N)
        assert env._return_as_np is True
        results.append((sac, env._steps, env._resets, torch.get_rng_state()))
    (dev, dsteps, dresets, drng), (host, hsteps, hresets, hrng) = results
    assert (dsteps, dresets) == (hsteps, hresets) and dsteps == L and torch.equal(drng, hrng)
    kept = [b[0] for b in host.batches]
    print(f"{name}: kept per step {kept} of {N}; stored {host.num_stored}, cur_idx {host.cur_idx}, capacity {cap}")
    assert len(kept) == L and kept[0] == N and dev.last_populate_counts == kept
    if N >= 48:
        assert 0 < kept[-1] < N, "the mask was never exercised"
    assert wraps == (sum(kept) > cap)
    assert (dev.cur_idx, dev.num_stored, len(dev)) == (host.cur_idx, host.num_stored, host.num_stored) and dev.cursor.tolist() == [host.cur_idx, host.num_stored]
    obs, action, next_obs, reward, done = (v.cpu().numpy() for v in dev.views())  # (both buffers start as zeros: whole arrays)
    for key, got in (("obs", obs), ("action", action), ("next_obs", next_obs), ("reward", reward)):
        assert np.array_equal(bits(got), bits(getattr(host, key))), key
    assert set(np.unique(done)) <= {0.0, 1.0} and np.array_equal(done != 0, host.terminated) and (N < 48 or host.terminated.any())
    for got, want in zip(dev.get_all().astuple(), (host.obs, host.action, host.next_obs, host.reward, host.terminated, host.truncated)):
        assert got.dtype == want.dtype and np.array_equal(got, want[:host.num_stored])


# ---- 4. update_many ----------------------------------------------------------------------------------------------------------------
SAC_CASE, SAC_B, SAC_UPDATES = "s17_6_17_17", 32, 5


def run_updates(engine, route, layout, single=False):
    """Five updates of a fresh TinySAC at the case's parameters, memories laid out by ``layout`` (a string over s / t: two SAC buffers,
    r: the real-data host buffer); ``route`` "device": s and t are DeviceReplayBuffers, "host": the restatement's host buffers of equal
    rows and equal-seeded generators.  Returns everything the two routes must agree on."""
    case = sr.complete_case(SAC_CASE, sr.CASES[SAC_CASE])
    obs, act, _, _ = case["shape"]
    sac, _ = sr.agent_for(case, DEV)
    mem = {}
    for key, (n, seed) in {"s": (200, 11), "t": (131, 12)}.items():
        dev, host = pair_of_buffers(engine, 256, obs, act, n, seed, data_seed=seed)
        mem[key] = dev if route == "device" else host
    mem["r"] = pair_of_buffers(engine, 64, obs, act, 50, 13, data_seed=13)[1]
    memories = [mem[k] for k in layout]
    torch.manual_seed(5)
    eps = [(torch.empty(SAC_B, act, device=DEV).normal_(), torch.empty(SAC_B, act, device=DEV).normal_()) for _ in layout]
    up = hipets.SACUpdater(sac, engine=engine)
    if single:
        res = [up.update_many([m], SAC_B, u, reverse_mask=True, eps=[e]) [0] for u, (m, e) in enumerate(zip(memories, eps))]
        res2 = up.update_parameters(memories[0], SAC_B, len(layout), reverse_mask=True)
        assert len(res2) == 5 and all(isinstance(v, float) for v in res2)
    else:
        res = up.update_many(memories, SAC_B, 0, reverse_mask=True, eps=eps)
    torch.cuda.synchronize()
    state = {n: t.detach().clone() for n, t in sac.params().items()}
    for n in sr.MOMENTS:
        opt_state = sac.optimizer_of(n).state[sac.params()[n]]
        state["m " + n], state["v " + n], state["step " + n] = opt_state["exp_avg"].clone(), opt_state["exp_avg_sq"].clone(), opt_state["step"].clone()
    return res, state, {k: rr.rng_state(m.rng) for k, m in mem.items()}, mem


@pytest.mark.parametrize("layout", ["sssss", "srssr", "ststt"], ids=["one_device_buffer", "real_data_mix", "two_device_buffers"])
def test_update_many_from_device_buffers_equals_host_buffers(engine, layout):
    res_d, state_d, rng_d, mem_d = run_updates(engine, "device", layout)
    res_h, state_h, rng_h, _ = run_updates(engine, "host", layout)
    assert all(isinstance(mem_d[k], hipets.DeviceReplayBuffer) for k in "st") and len(res_d) == SAC_UPDATES
    assert res_d == res_h and all(v == v for r in res_d for v in r)
    assert sorted(state_d) == sorted(state_h) and "log_alpha" in state_d and "m log_alpha" in state_d
    for k in state_d:
        assert torch.equal(state_d[k], state_h[k]), k
    assert rng_d == rng_h  # both routes consumed every generator alike
    fresh = rr.rng_state(np.random.default_rng(12))
    assert (rng_d["t"] == fresh) == ("t" not in layout) and rng_d["s"] != rr.rng_state(np.random.default_rng(11))


def test_update_parameters_equals_update_many_from_a_device_buffer(engine):
    res_m, state_m, rng_m, _ = run_updates(engine, "device", "sssss")
    res_s, state_s, rng_s, _ = run_updates(engine, "device", "sssss", single=True)
    assert res_s == res_m
    res_h, state_h, rng_h, _ = run_updates(engine, "host", "sssss", single=True)
    assert rng_s == rng_h and all(torch.equal(state_s[k], state_h[k]) for k in state_h)  # (six updates on either route)


# ---- 5. maybe_replace_sac_buffer -----------------------------------------------------------------------------------------------------
def test_maybe_replace_grows_and_shrinks_on_the_device(engine, monkeypatch):
    dev, host = pair_of_buffers(engine, 37, 3, 2, 30, seed=4)
    more = rows_of(np.random.default_rng(9), 15, 3, 2)
    dev.add_batch(*more)
    host.add_batch(*more)
    assert hipets.maybe_replace_sac_buffer(dev, (3,), (2,), 37, 0, engine=engine) is dev
    for capacity in (50, 30, 31):
        new_dev = hipets.maybe_replace_sac_buffer(dev, (3,), (2,), capacity, 0, engine=engine)
        new_host = rr.maybe_replace(host, (3,), (2,), capacity, 0)
        assert isinstance(new_dev, hipets.DeviceReplayBuffer) and new_dev is not dev and new_dev.device == dev.device and new_dev.capacity == capacity
        assert new_dev.rng is dev.rng  # the generator object is handed over
        assert (new_dev.cur_idx, new_dev.num_stored) == (new_host.cur_idx, new_host.num_stored) and new_dev.cursor.tolist() == [new_host.cur_idx, new_host.num_stored]
        for got, want in zip(new_dev.get_all().astuple(), new_host.get_all().astuple()):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        dev, host = new_dev, new_host
    first = hipets.maybe_replace_sac_buffer(None, (3,), (2,), 16, 7, engine=engine)
    assert isinstance(first, hipets.DeviceReplayBuffer) and rr.rng_state(first.rng) == rr.rng_state(np.random.default_rng(7)) and len(first) == 0
    # where a device buffer cannot be had: the reference's host buffer (here a stand-in for mbrl.util.ReplayBuffer), ONE warning
    fake, util = types.ModuleType("mbrl"), types.ModuleType("mbrl.util")
    fake.util, util.ReplayBuffer = util, rr.HostRingBuffer
    monkeypatch.setitem(sys.modules, "mbrl", fake)
    monkeypatch.setitem(sys.modules, "mbrl.util", util)
    with pytest.warns(UserWarning, match="on the host") as rec:
        out = hipets.maybe_replace_sac_buffer(None, (3, 3), (2,), 16, 7, engine=engine)
    ours = [str(r.message) for r in rec if "maybe_replace_sac_buffer" in str(r.message)]
    assert len(ours) == 1 and "1-D" in ours[0]
    assert type(out) is rr.HostRingBuffer and out.capacity == 16 and rr.rng_state(out.rng) == rr.rng_state(np.random.default_rng(7))
