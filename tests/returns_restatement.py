"""numpy float32 restatement of hipets_trajectory_returns (include/hipets.h; model_env.py:186-191 over a finished trajectory), shared by
tests/test_callable_objective_host.py and tests/test_gpu_callable_objective.py.  Per row, in step order:
    r = terminated ? 0 : rewards[t][row];  terminated |= dones[t][row] != 0;  total += r
then, per candidate, the particle mean as particle_mean_kernel forms it: a sequential float32 sum over p = 0 .. P-1, one division by
float32(P).  Every operation is a single correctly rounded float32 operation, so the result is the kernel's bit for bit."""
import numpy as np


def trajectory_returns_np(rewards, dones, pop, P):
    """(returns [pop], row_totals [B], first_done [B]) of rewards f32 [H, B] / dones [H, B] (any dtype, non-zero = done)."""
    rewards = np.asarray(rewards, np.float32)
    dones = np.asarray(dones) != 0
    H, B = rewards.shape
    assert B == pop * P and dones.shape == (H, B)
    tot = np.zeros(B, np.float32)
    term = np.zeros(B, bool)
    first = np.full(B, H, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(H):
            r = np.where(term, np.float32(0.0), rewards[t])  # a select: a NaN behind the termination adds exactly 0
            first = np.where(dones[t] & ~term, np.int32(t), first)
            term = term | dones[t]
            tot = (tot + r).astype(np.float32)
        s = np.zeros(pop, np.float32)
        per = tot.reshape(pop, P)
        for p in range(P):
            s = (s + per[:, p]).astype(np.float32)
        returns = (s / np.float32(P)).astype(np.float32)
    return returns, tot, first


def same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN standing for any NaN at the same position."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int32), b[ok].view(np.int32))
