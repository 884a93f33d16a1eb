"""hipets.DeviceReplayBuffer on the host, no GPU: the class on its torch route (device="cpu") and the numpy restatement the GPU tests
lean on (tests/replay_restatement.py), both against what the reference's own mbrl.util.ReplayBuffer / maybe_replace_sac_buffer
recorded (tests/golden/replay_buffer_cases.npz, tests/make_replay_golden.py); checkpoints in the stock format both ways; the refusals;
the Engine binding of the two new entry points."""
import os
import warnings

import numpy as np
import pytest
import torch

import hipets
import replay_restatement as rr
from conftest import GOLDEN
from hipets import _lib, mbpo
from oracle import ref_bridge
from test_engine_binding_host import PROTOS, check, eng, take  # noqa: F401  (eng: the Engine over a recording library)

GOLD = dict(np.load(os.path.join(GOLDEN, "replay_buffer_cases.npz")))
C = rr.SCRIPT


def cpu_buffer(capacity, obs_shape, action_shape, rng=None):
    return hipets.DeviceReplayBuffer(capacity, obs_shape, action_shape, rng=rng, device="cpu")


def assert_is_the_recorded_run(rec):
    assert sorted(rec) == sorted(GOLD)
    for k, want in GOLD.items():
        got = np.asarray(rec[k])
        assert got.shape == want.shape, k
        if want.dtype == np.float32:
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        elif want.dtype == np.bool_:
            assert got.dtype == np.bool_ and np.array_equal(got, want), k
        else:  # cur_idx, num_stored, the generator's state
            assert np.array_equal(got, want), k


def test_the_recorded_run_covers_the_script():
    """what the golden's script was written to hit, read off the recording itself"""
    assert [int(GOLD[f"add_batch{i}_num_stored"]) for i in range(4)] == [10, 30, 37, 37]
    assert [int(GOLD[f"add_batch{i}_cur_idx"]) for i in range(4)] == [10, 30, 8, 8]  # a wrap, then an exact lap
    assert int(GOLD["add_cur_idx"]) == 9 and int(GOLD["load_cur_idx"]) == 0 and int(GOLD["load_num_stored"]) == 37
    assert (int(GOLD["grow_cur_idx"]), int(GOLD["grow_num_stored"])) == (37, 37)
    assert (int(GOLD["shrink_cur_idx"]), int(GOLD["shrink_num_stored"])) == (7, 30)  # 37 rows into 30: the copy wraps
    assert GOLD["sample0_batch_reward"].shape == (C["sample"],) and GOLD["add_terminated"].any() and not GOLD["add_terminated"].all()
    assert str(GOLD["sample0_rng"]) != str(GOLD["sample1_rng"]) != str(GOLD["shuffle_rng"]) and str(GOLD["grow_rng"]) == str(GOLD["shuffle_rng"])


def test_restatement_is_the_recorded_run():
    rec, _ = rr.run_script(rr.HostRingBuffer, rr.maybe_replace)
    assert_is_the_recorded_run(rec)


def test_device_replay_buffer_on_the_cpu_is_the_recorded_run():
    rec, bufs = rr.run_script(cpu_buffer, hipets.maybe_replace_sac_buffer)
    assert_is_the_recorded_run(rec)
    assert all(isinstance(b, hipets.DeviceReplayBuffer) and b.device.type == "cpu" for b in bufs.values())
    assert bufs["grown"].rng is bufs["buf"].rng and bufs["shrunk"].rng is bufs["buf"].rng  # the generator object is handed over
    for b in bufs.values():  # the host pair and the device cursor agree
        assert b.cursor.tolist() == [b.cur_idx, b.num_stored] == [b.cur_idx, len(b)]
    assert hipets.maybe_replace_sac_buffer(bufs["buf"], (3,), (2,), C["capacity"], 0) is bufs["buf"]
    batch = bufs["buf"].sample(4)
    assert [np.asarray(v).dtype for v in batch.astuple()] == [np.float32] * 4 + [np.bool_] * 2 and not batch.astuple()[5].any()
    try:
        from mbrl.types import TransitionBatch
    except ImportError:
        return
    assert isinstance(batch, TransitionBatch)


def filled(make, n=25, capacity=C["capacity"], seed=3):
    buf = make(capacity, (C["obs_dim"],), (C["act_dim"],), rng=np.random.default_rng(seed))
    for rows in rr.script_inputs()[:3]:
        buf.add_batch(*(v[:n] for v in rows))
    return buf


def same_rows(a, b):
    for x, y in zip(a.get_all().astuple(), b.get_all().astuple()):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert (a.cur_idx, a.num_stored) == (b.cur_idx, b.num_stored)


def test_checkpoints_interchange_with_a_stock_format_buffer(tmp_path):
    """save -> the reference's replay_buffer.npz (its keys, its dtypes) -> load into a second buffer, in both directions with the
    restatement's stock-format save / load"""
    dev, host = filled(cpu_buffer), filled(rr.HostRingBuffer)
    same_rows(dev, host)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    dev.save(tmp_path / "a")
    host.save(tmp_path / "b")
    fa, fb = np.load(tmp_path / "a" / "replay_buffer.npz"), np.load(tmp_path / "b" / "replay_buffer.npz")
    assert sorted(fa.files) == sorted(fb.files) == sorted(rr.FIELDS + ("trajectory_indices",))
    for k in rr.FIELDS:
        assert fa[k].dtype == fb[k].dtype and np.array_equal(fa[k], fb[k]), k
    into_host, into_dev, again = (make(C["capacity"], (C["obs_dim"],), (C["act_dim"],)) for make in (rr.HostRingBuffer, cpu_buffer, cpu_buffer))
    into_host.load(str(tmp_path / "a"))
    into_dev.load(tmp_path / "b")
    again.load(tmp_path / "a")
    same_rows(into_dev, into_host)
    same_rows(again, into_host)
    assert again.cursor.tolist() == [again.cur_idx, again.num_stored] == [0, C["capacity"]]
    # from_buffer / views: the host buffer's rows, cursor and generator, in the staging area's layout
    moved = hipets.DeviceReplayBuffer.from_buffer(host, device="cpu")
    same_rows(moved, host)
    assert moved.rng is host.rng
    obs, action, next_obs, reward, done = mbpo.staging_views(moved.storage, moved.capacity, C["obs_dim"], C["act_dim"])
    assert all(a.data_ptr() == b.data_ptr() and a.shape == b.shape for a, b in zip(moved.views(), (obs, action, next_obs, reward, done)))
    assert np.array_equal(done.numpy() != 0, host.terminated) and np.array_equal(obs.numpy(), host.obs)


@pytest.mark.skipif(not ref_bridge.reference_available(), reason="needs the reference checkout")
def test_hand_overs_with_the_live_reference_buffer(tmp_path):
    ref_bridge.import_reference()
    from mbrl.util import ReplayBuffer

    stock = filled(ReplayBuffer)
    dev = hipets.DeviceReplayBuffer.from_buffer(stock, device="cpu")
    same_rows(dev, stock)
    assert dev.rng is stock.rng
    back = dev.to_buffer()
    assert type(back) is ReplayBuffer and back.rng is stock.rng and back.capacity == stock.capacity
    same_rows(back, stock)
    dev.save(tmp_path)
    loaded = ReplayBuffer(C["capacity"], (C["obs_dim"],), (C["act_dim"],))
    loaded.load(tmp_path)  # a stock buffer loads the device buffer's checkpoint
    assert (loaded.cur_idx, loaded.num_stored) == (0, C["capacity"])
    for x, y in zip(loaded.get_all().astuple(), stock.get_all().astuple()):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    stock.save(tmp_path)
    again = cpu_buffer(C["capacity"], (C["obs_dim"],), (C["act_dim"],))
    again.load(tmp_path)  # ... and the other way round
    same_rows(again, loaded)


def test_gather_on_the_cpu_is_pack_sac_batch():
    dev, host = filled(cpu_buffer), filled(rr.HostRingBuffer)
    idx = np.array([0, C["capacity"] - 1, 5, 5, 17])
    for reverse in (False, True):
        want = mbpo.pack_sac_batch(host._batch_from_indices(idx).astuple(), reverse)
        assert np.array_equal(dev.gather(idx, reverse).numpy().view(np.uint32), want.view(np.uint32))
    a, b = filled(cpu_buffer), filled(rr.HostRingBuffer)
    assert np.array_equal(a.sample_indices(6), b.rng.choice(b.num_stored, size=6)) and rr.rng_state(a.rng) == rr.rng_state(b.rng)
    with pytest.raises(ValueError, match="indices"):
        dev.gather([C["capacity"]])


def test_refusals():
    with pytest.raises(hipets.UnsupportedModelError, match="1-D"):
        hipets.DeviceReplayBuffer(8, (3, 3), (2,), device="cpu")
    with pytest.raises(hipets.UnsupportedModelError, match="1-D"):
        hipets.DeviceReplayBuffer(8, (3,), (), device="cpu")
    with pytest.raises(hipets.UnsupportedModelError, match="float32"):
        hipets.DeviceReplayBuffer(8, (3,), (2,), device="cpu", obs_type=np.float64)
    with pytest.raises(hipets.UnsupportedModelError, match="trajectory"):
        hipets.DeviceReplayBuffer(8, (3,), (2,), device="cpu", max_trajectory_length=10)
    # a batch that cannot fit: the reference fills the rows up to the end and fails on the remainder (np.copyto) when that is
    # longer than the buffer; here nothing is written
    buf = cpu_buffer(8, (3,), (2,))
    g = np.random.default_rng(0)
    rows = lambda n: (g.standard_normal((n, 3)).astype(np.float32), g.standard_normal((n, 2)).astype(np.float32),  # noqa: E731
                      g.standard_normal((n, 3)).astype(np.float32), g.standard_normal(n).astype(np.float32), g.random(n) < 0.5, np.zeros(n, bool))
    buf.add_batch(*rows(3))
    before = buf.storage.clone()
    for make in (lambda: buf, lambda: filled(rr.HostRingBuffer, n=1, capacity=8)):
        with pytest.raises(ValueError):
            make().add_batch(*rows(2 * 8 + 1))
    assert torch.equal(buf.storage, before) and (buf.cur_idx, buf.num_stored) == (3, 3)
    bad = list(rows(2))
    bad[5] = np.array([False, True])
    with pytest.raises(ValueError, match="truncated"):
        buf.add_batch(*bad)
    with pytest.raises(ValueError, match="shape"):
        buf.add_batch(*[v[:, :2] if v.ndim == 2 else v for v in rows(2)])
    # maybe_replace_sac_buffer where a device buffer cannot be had: the UnsupportedModelError itself without mbrl, the reference's
    # host buffer with ONE warning with it
    try:
        import mbrl.util  # noqa: F401
    except ImportError:
        with pytest.raises(hipets.UnsupportedModelError, match="1-D"):
            hipets.maybe_replace_sac_buffer(buf, (3, 3), (2,), 16, 0)
    else:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out = hipets.maybe_replace_sac_buffer(None, (3, 3), (2,), 16, 0)
        assert isinstance(out, mbrl.util.ReplayBuffer) and len(rec) == 1 and "1-D" in str(rec[0].message)


def test_header_and_binding_agree_on_the_new_entry_points():
    for name in ("hipets_ring_compact_transitions", "hipets_replay_gather"):
        assert [n for _, n in PROTOS[name][1]] == [n for n, _ in _lib.SYMBOLS[name][1]], name
    assert [n for _, n in PROTOS["hipets_ring_compact_transitions"][1]] == \
        [{"staging": "ring", "cap": "capacity", "offset": "cursor"}.get(n, n) for _, n in PROTOS["hipets_compact_transitions"][1]]
    assert _lib.ABI_VERSION == 9


def test_engine_binding_of_the_ring_compaction_and_the_gather(eng):  # noqa: F811
    t = dict(obs=torch.zeros(6, 5), action=torch.zeros(6, 2), next_obs=torch.zeros(6, 5), rewards=torch.zeros(6, 1), dones=torch.zeros(6, 1, dtype=torch.bool),
             accum_dones=torch.zeros(6, dtype=torch.uint8), ring=torch.zeros(18 * 14), capacity=18, cursor=torch.zeros(2, dtype=torch.int64),
             count_out=torch.zeros(1, dtype=torch.int32))
    eng.ring_compact_transitions(*t.values())
    check(take(eng, "hipets_ring_compact_transitions"), "hipets_ring_compact_transitions", n=6, obs_dim=5, act_dim=2, **t)
    with pytest.raises(ValueError, match="ring must hold"):
        eng.ring_compact_transitions(*{**t, "ring": torch.zeros(18 * 14 - 1)}.values())
    with pytest.raises(ValueError, match="cursor must have 2 elements"):
        eng.ring_compact_transitions(*{**t, "cursor": torch.zeros(1, dtype=torch.int64)}.values())
    with pytest.raises(ValueError, match="next_obs must have shape"):
        eng.ring_compact_transitions(*{**t, "next_obs": torch.zeros(6, 4)}.values())
    idx = torch.tensor([3, 17, 3], dtype=torch.int64)
    out = eng.replay_gather(t["ring"], 18, 5, 2, idx, reverse_mask=True)
    assert out.shape == (3, 14) and out.dtype == torch.float32
    check(take(eng, "hipets_replay_gather"), "hipets_replay_gather", ring=t["ring"], capacity=18, obs_dim=5, act_dim=2, indices=idx, n_rows=3,
          reverse_mask=1, out=out)
    mine = torch.zeros(2, 14)
    assert eng.replay_gather(t["ring"], 18, 5, 2, np.array([0, 17]), out=mine) is mine  # host indices: checked, uploaded
    rec = take(eng, "hipets_replay_gather")
    assert (rec["n_rows"], rec["reverse_mask"], rec["out"]) == (2, 0, mine.data_ptr()) and rec["indices"] not in (None, idx.data_ptr())
    for bad in ([18], [-1], [0.5]):
        with pytest.raises(ValueError, match="indices must be integers"):
            eng.replay_gather(t["ring"], 18, 5, 2, np.array(bad))
    with pytest.raises(ValueError, match="ring must hold"):
        eng.replay_gather(torch.zeros(18 * 14 - 1), 18, 5, 2, idx)
    assert eng.replay_gather(t["ring"], 18, 5, 2, np.zeros(0, dtype=np.int64)).shape == (0, 14)  # no rows: no launch
    assert eng._lib.calls == []
