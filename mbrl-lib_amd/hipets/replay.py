"""MBPO's SAC replay buffer on the device (mbrl/util/replay_buffer.py:404-707, the part mbrl/algorithms/mbpo.py touches): the rows the
model rollouts write are the rows SAC's updates read, so they stay where both are.

    sac_buffer = hipets.maybe_replace_sac_buffer(sac_buffer, obs_shape, act_shape, capacity, seed)   # a DeviceReplayBuffer
    hipets.rollout_model_and_populate_sac_buffer(model_env, replay_buffer, agent, sac_buffer, ...)   # compacts straight into its ring
    updater.update_parameters(sac_buffer, batch_size, updates_made, logger, reverse_mask=True)        # gathers its batch on the device

Every index is drawn on the host by the buffer's own numpy generator, as the reference draws it; every stored and sampled float is a
plain copy.
"""
from __future__ import annotations

import pathlib
import warnings
from types import SimpleNamespace
from typing import Optional, Sequence

import numpy as np
import torch

from ._pack import row_columns, row_width, staging_views
from .model import UnsupportedModelError


def _transition_batch(obs, act, next_obs, rewards, terminateds, truncateds):
    try:
        from mbrl.types import TransitionBatch
    except ImportError:
        tup = (obs, act, next_obs, rewards, terminateds, truncateds)
        return SimpleNamespace(obs=obs, act=act, next_obs=next_obs, rewards=rewards, terminateds=terminateds, truncateds=truncateds,
                               astuple=lambda: tup)
    return TransitionBatch(obs, act, next_obs, rewards, terminateds, truncateds)


class DeviceReplayBuffer:
    """``mbrl.util.ReplayBuffer`` as MBPO uses it for its SAC buffer, stored on the device: ``capacity``, ``cur_idx``, ``num_stored``,
    ``len()``, ``rng``, ``add``, ``add_batch``, ``sample``, ``get_all``, ``save`` / ``load`` with that class's semantics and its
    ``replay_buffer.npz`` format, plus what the device seams use: ``sample_indices``, ``gather``, ``views``, ``cursor``, ``sync``.

    The storage is ONE float32 tensor of ``capacity * (2 obs + act + 2) * 4`` bytes (``mbpo_halfcheetah``'s largest buffer, 2 M rows of
    obs 17 / act 6: 336 MB), five arrays one behind the other -- obs, action, next_obs, reward, done as 0.0 / 1.0 (:meth:`views`).
    1-D ``obs_shape`` / ``action_shape`` and float32 only, no trajectory bookkeeping; anything else, and a failed allocation, raises
    UnsupportedModelError.  The truncated flags are not stored: MBPO's are all False, and so are the ones handed out; a host batch
    with a flag set is refused.

    ``engine``: a ``hipets.Engine`` (default: the one of ``device``, default the current GPU).  With ``device="cpu"`` and no engine the
    same class runs every storage operation as torch indexing on the host.

    ``cur_idx`` / ``num_stored`` live on the host AND in ``cursor`` (int64 [2] on the device, what the populate's ring compaction
    advances).  Every method here keeps both; after device work that advanced ``cursor`` alone, :meth:`sync` reads it back (one 16-byte
    copy; ``hipets.rollout_model_and_populate_sac_buffer`` sets the host pair itself)."""

    def __init__(self, capacity: int, obs_shape: Sequence[int], action_shape: Sequence[int], rng: Optional[np.random.Generator] = None,
                 engine=None, device=None, *, obs_type=np.float32, action_type=np.float32, reward_type=np.float32,
                 max_trajectory_length: Optional[int] = None):
        obs_shape, action_shape = tuple(int(v) for v in obs_shape), tuple(int(v) for v in action_shape)
        if len(obs_shape) != 1 or len(action_shape) != 1 or obs_shape[0] < 1 or action_shape[0] < 1:
            raise UnsupportedModelError(f"a device replay buffer stores 1-D observations and actions, got {obs_shape} / {action_shape}")
        if any(np.dtype(t) != np.float32 for t in (obs_type, action_type, reward_type)):
            raise UnsupportedModelError("a device replay buffer stores float32 only")
        if max_trajectory_length:
            raise UnsupportedModelError("a device replay buffer keeps no trajectory information")
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1")
        if engine is None and (device is None or torch.device(device).type == "cuda"):
            from .engine import get_engine

            engine = get_engine("cuda" if device is None else device)
        self.engine = engine
        self.device = engine.device if engine is not None else torch.device(device)
        self.capacity, self.obs_dim, self.act_dim = int(capacity), obs_shape[0], action_shape[0]
        self.width = row_width(self.obs_dim, self.act_dim)
        try:
            self.storage = torch.zeros(self.capacity * self.width, dtype=torch.float32, device=self.device)
            self.cursor = torch.zeros(2, dtype=torch.int64, device=self.device)
        except RuntimeError as exc:  # (torch.cuda.OutOfMemoryError is one)
            raise UnsupportedModelError(f"no room on {self.device} for a replay buffer of {self.capacity * self.width * 4} bytes ({exc})") from None
        self.cur_idx, self.num_stored = 0, 0
        self._rng = np.random.default_rng() if rng is None else rng

    # ---- the cursor ---------------------------------------------------------------------------------------------------------------
    def _set_cursor(self, cur_idx: int, num_stored: int):
        self.cur_idx, self.num_stored = int(cur_idx), int(num_stored)
        self.cursor.copy_(torch.tensor([self.cur_idx, self.num_stored], dtype=torch.int64))

    def sync(self):
        """Read ``cursor`` back into ``cur_idx`` / ``num_stored`` (the one small device -> host copy): after ring compactions that
        were queued on this buffer directly."""
        self.cur_idx, self.num_stored = (int(v) for v in self.cursor.cpu())
        return self

    def __len__(self):
        return self.num_stored

    @property
    def rng(self) -> np.random.Generator:
        return self._rng

    def views(self):
        """(obs [capacity, obs], action [capacity, act], next_obs [capacity, obs], reward [capacity], done [capacity] as 0.0 / 1.0):
        views of the storage, on the device (``hipets._pack.staging_views`` of it)"""
        return staging_views(self.storage, self.capacity, self.obs_dim, self.act_dim)

    # ---- writing ------------------------------------------------------------------------------------------------------------------
    def _rows(self, v, n, dim, name):
        """``v`` as a float32 tensor [n] or [n, dim] on the buffer's device"""
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.ascontiguousarray(np.asarray(v), dtype=np.float32))
        v = v.to(device=self.device, dtype=torch.float32)
        want = (n,) if dim is None else (n, dim)
        if tuple(v.shape) != want:
            raise ValueError(f"{name} must have shape {want}, got {tuple(v.shape)}")
        return v

    def add_batch(self, obs, action, next_obs, reward, terminated, truncated=None):
        """``ReplayBuffer.add_batch`` (replay_buffer.py:553-599) for host arrays or tensors on any device: one upload each and at most
        two slice copies, the reference's wrap-around -- a batch that passes the end fills the rows up to it, then continues at row 0
        -- and its ValueError for a batch whose remainder does not fit (``cur_idx + n > 2 capacity``; raised here before anything is
        written)."""
        n = len(obs)
        if truncated is not None and not isinstance(truncated, torch.Tensor) and np.any(truncated):
            raise ValueError("a device replay buffer does not store truncated flags")
        rows = (self._rows(obs, n, self.obs_dim, "obs"), self._rows(action, n, self.act_dim, "action"),
                self._rows(next_obs, n, self.obs_dim, "next_obs"), self._rows(reward, n, None, "reward"),
                self._rows(terminated, n, None, "terminated"))
        cur, stored, cap = self.cur_idx, self.num_stored, self.capacity
        first = cap - cur if cur + n > cap else 0
        if n - first > cap:
            raise ValueError(f"a batch of {n} rows does not fit a buffer of {cap} rows at row {cur}")
        views = self.views()

        def copy_from_to(buffer_start, batch_start, how_many):
            for dst, src in zip(views, rows):
                dst[buffer_start:buffer_start + how_many].copy_(src[batch_start:batch_start + how_many])

        if first:
            copy_from_to(cur, 0, first)
            cur, stored = 0, cap
        how_many = n - first
        copy_from_to(cur, first, how_many)
        self._set_cursor((cur + how_many) % cap, min(stored + how_many, cap))

    def add(self, obs, action, next_obs, reward, terminated, truncated=False):
        """``ReplayBuffer.add``: one transition"""
        def one(v):
            return v.reshape(1, -1) if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float32).reshape(1, -1)

        self.add_batch(one(obs), one(action), one(next_obs), np.asarray([reward], dtype=np.float32), np.asarray([bool(terminated)]),
                       np.asarray([bool(truncated)]))

    # ---- reading ------------------------------------------------------------------------------------------------------------------
    def sample_indices(self, batch_size: int) -> np.ndarray:
        """The draw of :meth:`sample` (replay_buffer.py:613) without the gather: it consumes the generator exactly as ``sample`` does"""
        return self._rng.choice(self.num_stored, size=batch_size)

    def gather(self, indices, reverse_mask: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """f32 [n, 2 obs + act + 2] on the device: row j = (obs, action, next_obs, reward, mask) of row ``indices[j]``, ``mask`` the
        done flag or, under ``reverse_mask``, its negation -- ``hipets._pack.pack_sac_batch``'s layout.  One launch
        (``Engine.replay_gather``).  Host indices are range-checked (ValueError)."""
        if self.engine is not None:
            return self.engine.replay_gather(self.storage, self.capacity, self.obs_dim, self.act_dim, indices, reverse_mask, out)
        idx = torch.as_tensor(np.asarray(indices) if not isinstance(indices, torch.Tensor) else indices, dtype=torch.int64).reshape(-1)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.capacity):
            raise ValueError(f"indices must be integers in [0, {self.capacity})")
        obs, action, next_obs, reward, done = (v[idx] for v in self.views())
        mask = (done == 0).to(torch.float32) if reverse_mask else done
        rows = torch.cat([obs, action, next_obs, reward[:, None], mask[:, None]], dim=1)
        return rows if out is None else out.copy_(rows)

    def _batch(self, rows: np.ndarray):
        a, s2, r, m = row_columns(self.obs_dim, self.act_dim)
        return _transition_batch(rows[:, :a].copy(), rows[:, a:s2].copy(), rows[:, s2:r].copy(), rows[:, r].copy(), rows[:, m] != 0,
                                 np.zeros(len(rows), dtype=bool))

    def _batch_from_indices(self, indices):
        return self._batch(self.gather(indices).cpu().numpy())

    def sample(self, batch_size: int):
        """``ReplayBuffer.sample``: rows ``rng.choice(num_stored, size=batch_size)`` on the HOST -- an ``mbrl.types.TransitionBatch``
        where mbrl imports (an object with the same six fields and ``astuple()`` otherwise): obs / act / next_obs float32, rewards
        (B,) float32, terminateds bool, truncateds all False."""
        return self._batch_from_indices(self.sample_indices(batch_size))

    def get_all(self, shuffle: bool = False):
        """``ReplayBuffer.get_all``: the ``num_stored`` rows in storage order, or in ``rng.permutation`` order, on the host"""
        if shuffle:
            return self._batch_from_indices(self._rng.permutation(self.num_stored))
        obs, action, next_obs, reward, done = (v[:self.num_stored].cpu().numpy() for v in self.views())
        return _transition_batch(obs, action, next_obs, reward, done != 0, np.zeros(self.num_stored, dtype=bool))

    # ---- checkpoints and hand-overs -----------------------------------------------------------------------------------------------
    def save(self, save_dir):
        """``ReplayBuffer.save``: ``<save_dir>/replay_buffer.npz`` in the reference's format (a stock buffer loads it)"""
        obs, action, next_obs, reward, terminated, truncated = self.get_all().astuple()
        np.savez(pathlib.Path(save_dir) / "replay_buffer.npz", obs=obs, next_obs=next_obs, action=action, reward=reward, terminated=terminated,
                 truncated=truncated, trajectory_indices=[])

    def load(self, load_dir):
        """``ReplayBuffer.load``: a ``replay_buffer.npz`` of this class or of a stock buffer; ``cur_idx = num_stored % capacity``"""
        data = np.load(pathlib.Path(load_dir) / "replay_buffer.npz")
        n = len(data["obs"])
        if n > self.capacity:
            raise ValueError(f"the file holds {n} rows, the buffer {self.capacity}")
        if np.any(data["truncated"]):
            raise ValueError("a device replay buffer does not store truncated flags")
        for dst, key, dim in zip(self.views(), ("obs", "action", "next_obs", "reward", "terminated"),
                                 (self.obs_dim, self.act_dim, self.obs_dim, None, None)):
            dst[:n].copy_(self._rows(data[key], n, dim, key))
        self._set_cursor(n % self.capacity, n)

    @classmethod
    def from_buffer(cls, host_buffer, engine=None, device=None):
        """A device buffer with a host ``ReplayBuffer``'s capacity, rows, ``cur_idx`` / ``num_stored`` and generator (the object itself)"""
        if getattr(host_buffer, "trajectory_indices", None) is not None:
            raise UnsupportedModelError("a device replay buffer keeps no trajectory information")
        n = int(host_buffer.num_stored)
        if np.any(host_buffer.truncated[:n]):
            raise UnsupportedModelError("a device replay buffer does not store truncated flags")
        new = cls(host_buffer.capacity, host_buffer.obs.shape[1:], host_buffer.action.shape[1:], rng=host_buffer.rng, engine=engine, device=device,
                  obs_type=host_buffer.obs.dtype, action_type=host_buffer.action.dtype, reward_type=host_buffer.reward.dtype)
        for dst, src, dim in zip(new.views(), (host_buffer.obs, host_buffer.action, host_buffer.next_obs, host_buffer.reward, host_buffer.terminated),
                                 (new.obs_dim, new.act_dim, new.obs_dim, None, None)):
            dst[:n].copy_(new._rows(src[:n], n, dim, "rows"))
        new._set_cursor(host_buffer.cur_idx, n)
        return new

    def to_buffer(self):
        """An ``mbrl.util.ReplayBuffer`` with this buffer's capacity, rows, ``cur_idx`` / ``num_stored`` and generator (needs mbrl)"""
        from mbrl.util import ReplayBuffer

        host = ReplayBuffer(self.capacity, (self.obs_dim,), (self.act_dim,), rng=self._rng)
        n = self.num_stored
        obs, action, next_obs, reward, terminated, truncated = self.get_all().astuple()
        host.obs[:n], host.action[:n], host.next_obs[:n], host.reward[:n] = obs, action, next_obs, reward
        host.terminated[:n], host.truncated[:n] = terminated, truncated
        host.cur_idx, host.num_stored = self.cur_idx, n
        return host


def maybe_replace_sac_buffer(sac_buffer, obs_shape: Sequence[int], act_shape: Sequence[int], new_capacity: int, seed: int, engine=None):
    """``mbrl.algorithms.mbpo.maybe_replace_sac_buffer`` (mbpo.py:88-113), same signature and generator hand-over, returning a
    :class:`DeviceReplayBuffer`: a new one where there was none or the capacity changed, the ``num_stored`` rows of the old one moved
    in storage order through ``add_batch`` (device to device from a DeviceReplayBuffer).  Where a DeviceReplayBuffer cannot be had
    (UnsupportedModelError) the reference's host buffer, with ONE warning that names the reason -- or, where mbrl cannot be imported,
    the UnsupportedModelError itself."""
    if sac_buffer is not None and new_capacity == sac_buffer.capacity:
        return sac_buffer
    rng = np.random.default_rng(seed=seed) if sac_buffer is None else sac_buffer.rng
    try:
        device = "cpu" if engine is None and isinstance(sac_buffer, DeviceReplayBuffer) and sac_buffer.engine is None else None
        new_buffer = DeviceReplayBuffer(new_capacity, obs_shape, act_shape, rng=rng, engine=engine, device=device)
    except UnsupportedModelError as exc:
        try:
            from mbrl.util import ReplayBuffer
        except ImportError:
            raise exc from None
        warnings.warn(f"hipets.maybe_replace_sac_buffer: keeping the SAC buffer on the host ({exc})", stacklevel=2)
        new_buffer = ReplayBuffer(new_capacity, obs_shape, act_shape, rng=rng)
    if sac_buffer is None:
        return new_buffer
    if isinstance(sac_buffer, DeviceReplayBuffer) and isinstance(new_buffer, DeviceReplayBuffer):
        n = sac_buffer.num_stored
        obs, action, next_obs, reward, done = (v[:n] for v in sac_buffer.views())
        new_buffer.add_batch(obs, action, next_obs, reward, done, None)
    else:
        new_buffer.add_batch(*sac_buffer.get_all().astuple())
    return new_buffer
