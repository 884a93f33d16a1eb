"""TEST INFRASTRUCTURE: restatements of what hipets/value.py adds, and the cases the critic tests share.

  critic_f64             QNetwork.forward (mbrl/third_party/pytorch_sac_pranz24/model.py:36-61) in float64 from explicit weight arrays: the
                         GPU tests' reference.
  critic_f32_torch       the same forward through torch CPU's float32 kernels (F.linear, relu): what a QNetwork-shaped module computes on
                         the CPU.  Its distance from critic_f64 in units of T1 is `u`, the yardstick of the tests' bound T1 x max(1, 4 u)
                         (tests/test_gpu_policy.py's rule) -- computed on the CPU, never taken from the kernel.
  discounted_returns_np  hipets_discounted_returns (include/hipets.h) in numpy float32, one correctly rounded operation per line, with
                         the particle reduction of tests/particle_reduce_restatement.py: the kernel's result bit for bit.
  CRITIC_CASES / make_critic_case   the shapes of tests/test_gpu_value.py and their seeded weights.  Q1 and Q2 are independent draws, and
                         building a case asserts that exchanging the two networks' layers moves q1 by more than the test's bound, so
                         parity refuses a kernel that indexes the wrong network.
"""
import numpy as np

import particle_reduce_restatement as prr
from policy_restatement import T1, t1_share  # noqa: F401  (T1 = rtol 1e-5, atol 2e-6)

LAYERS = tuple(f"c{k}{i}" for i in range(1, 7) for k in "wb")  # cw1, cb1, .. cw6, cb6 (1-3 = Q1, 4-6 = Q2), nn.Linear's [out, in]


def critic_f64(w, obs, act):
    """(q1, q2) float64 [B]; `w` = dict of cw1 cb1 .. cw6 cb6"""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    xu = np.concatenate([f(obs), f(act)], axis=1)
    out = []
    for j in (1, 4):
        h1 = np.maximum(xu @ f(w[f"cw{j}"]).T + f(w[f"cb{j}"]), 0.0)
        h2 = np.maximum(h1 @ f(w[f"cw{j + 1}"]).T + f(w[f"cb{j + 1}"]), 0.0)
        out.append((h2 @ f(w[f"cw{j + 2}"]).T + f(w[f"cb{j + 2}"]))[:, 0])
    return out[0], out[1]


def critic_f32_torch(w, obs, act):
    """(q1, q2) float32 [B] as torch CPU computes a QNetwork-shaped forward: cat, F.linear, F.relu"""
    import torch
    import torch.nn.functional as F

    c = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    xu = torch.cat([c(obs), c(act)], 1)
    out = []
    for j in (1, 4):
        h1 = F.relu(F.linear(xu, c(w[f"cw{j}"]), c(w[f"cb{j}"])))
        h2 = F.relu(F.linear(h1, c(w[f"cw{j + 1}"]), c(w[f"cb{j + 1}"])))
        out.append(F.linear(h2, c(w[f"cw{j + 2}"]), c(w[f"cb{j + 2}"]))[:, 0].numpy())
    return out[0], out[1]


def torch_cpu_share(w, obs, act):
    """per row, the larger share of T1 that torch CPU's float32 forward uses against critic_f64, of q1 and q2; a test's u is the
    largest over the rows it runs"""
    r1, r2 = critic_f64(w, obs, act)
    g1, g2 = critic_f32_torch(w, obs, act)
    return np.maximum(t1_share(g1, r1), t1_share(g2, r2))


def bound_factor(u):
    return max(1.0, 4.0 * u)


def allowance(ref64, u):
    """per element, what the rule allows: T1 x max(1, 4 u)"""
    return (T1["atol"] + T1["rtol"] * np.abs(np.asarray(ref64, dtype=np.float64))) * bound_factor(u)


def exchanged(w, layers=(1, 2, 3)):
    """`w` with the given layers of Q1 and Q2 exchanged (layer i of Q1 is linear i, of Q2 linear i + 3)"""
    out = dict(w)
    for i in layers:
        for k in "wb":
            out[f"c{k}{i}"], out[f"c{k}{i + 3}"] = w[f"c{k}{i + 3}"], w[f"c{k}{i}"]
    return out


# ---- the critic cases of the GPU tests: (name, obs, act, hidden, batches); a batch "R-1" / "R+1" is 16 R -/+ 1 with R the row tiles per
# workgroup of that critic (Engine.critic_geometry) ----
CRITIC_CASES = [
    ("k14_h20", 11, 3, 20, (1, "R-1", "R+1")),  # K = 14 under one k-block, hidden pads to 32
    ("k16_h16", 12, 4, 16, (33,)),              # no padding anywhere
    ("k35_h64", 27, 8, 64, (257,)),             # Ant's K crosses 32
    ("k23_h256", 17, 6, 256, (1000,)),          # many workgroups, a ragged last one
    ("k23_h512", 17, 6, 512, ("R+1",)),         # the middle R
    ("k393_h1024", 376, 17, 1024, (40,)),       # Humanoid's K at the LDS limit
    # the two-source input staging: the obs / act boundary at k = 1 with everything padded (hidden 2: with a one-wide hidden layer a
    # relu that is off leaves the first layers without influence on 37% of the rows, and the separation below cannot hold) ...
    ("k2_h2", 1, 1, 2, (1, 17)),
    ("k17_h16", 16, 1, 16, (16,)),              # ... and exactly on a k-block edge, K one past it
]
CASE_ROWS = 1000
_BUILT = {}


def make_critic_case(name, obs_dim, act_dim, hidden, rows=CASE_ROWS):
    """(weights dict, obs [rows, obs], act [rows, act], u [rows]) of a case, built once: xavier-uniform weights (gain 1) from a
    generator seeded by the case's name, one draw after the other so that Q1 and Q2 share nothing; small biases; obs ~ N(0, 1), act ~
    U(-1, 1); u = torch_cpu_share per row.  Asserts the separation of the two networks (module docstring) under the bound of ALL rows,
    which is at least the bound of any batch a test takes from them."""
    if name in _BUILT:
        return _BUILT[name]
    rng = np.random.default_rng([ord(c) for c in name])
    K = obs_dim + act_dim

    def xavier(n_out, n_in):
        a = np.sqrt(6.0 / (n_in + n_out))
        return rng.uniform(-a, a, (n_out, n_in)).astype(np.float32)

    bias = lambda n: rng.uniform(-0.1, 0.1, n).astype(np.float32)  # noqa: E731
    w = {}
    for j in (1, 4):
        for i, (n_out, n_in) in enumerate(((hidden, K), (hidden, hidden), (1, hidden))):
            w[f"cw{j + i}"], w[f"cb{j + i}"] = xavier(n_out, n_in), bias(n_out)
    obs = rng.standard_normal((rows, obs_dim)).astype(np.float32)
    act = rng.uniform(-1.0, 1.0, (rows, act_dim)).astype(np.float32)
    u = torch_cpu_share(w, obs, act)
    assert_networks_separate(w, obs, act, float(u.max()))
    _BUILT[name] = (w, obs, act, u)
    return _BUILT[name]


def assert_networks_separate(w, obs, act, u):
    """Exchanging Q1's and Q2's layers -- all three, or any single one -- moves q1 by more than the rule's allowance at share `u` on at
    least nine rows in ten and on row 0"""
    q1 = critic_f64(w, obs, act)[0]
    allow = allowance(q1, u)
    for layers in ((1, 2, 3), (1,), (2,), (3,)):
        moved = np.abs(critic_f64(exchanged(w, layers), obs, act)[0] - q1) > allow
        assert moved[0] and moved.mean() >= 0.9, f"exchanging layers {layers} of Q1 and Q2 moves q1 on {moved.mean():.0%} of the rows only"


# ---- hipets_discounted_returns ---------------------------------------------------------------------------------------------------
def discounted_returns_np(rewards, dones, pop, P, gamma=1.0, values=None, reduce=("mean", 0.0, 0)):
    """(returns [pop], row_totals [B], first_done [B]) of rewards f32 [H, B] / dones [H, B] (any dtype, non-zero = done), `values` f32
    [B] or None, `reduce` = (kind, kappa, worst_k) of tests/particle_reduce_restatement.py.  Per row, in step order:
        r = terminated ? 0 : rewards[t][row];  terminated |= dones[t][row] != 0;  total = total + disc * r;  disc = disc * gamma
    and with values:  total = total + (terminated ? 0 : disc * values[row])"""
    F = np.float32
    rewards = np.asarray(rewards, F)
    dones = np.asarray(dones) != 0
    H, B = rewards.shape
    assert B == pop * P and dones.shape == (H, B)
    g = F(gamma)
    tot = np.zeros(B, F)
    disc = F(1.0)  # (the same for every row)
    term = np.zeros(B, bool)
    first = np.full(B, H, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(H):
            r = np.where(term, F(0.0), rewards[t])  # a select: a NaN behind the termination adds exactly 0
            first = np.where(dones[t] & ~term, np.int32(t), first)
            term = term | dones[t]
            dr = (disc * r).astype(F)
            tot = (tot + dr).astype(F)
            disc = F(disc * g)
        if values is not None:
            dv = (disc * np.asarray(values, F).reshape(B)).astype(F)
            tot = (tot + np.where(term, F(0.0), dv)).astype(F)
    kind, kappa, k = reduce
    return prr.particle_reduce(tot, pop, P, kind, kappa, k), tot, first


def discounted_returns_f64(rewards, dones, pop, P, gamma, values=None):
    """the same chain in float64 with the particle MEAN: (returns [pop], row_totals [B]) -- for margins, not for bits"""
    rewards = np.asarray(rewards, np.float64)
    dones = np.asarray(dones) != 0
    H, B = rewards.shape
    tot, term = np.zeros(B), np.zeros(B, bool)
    for t in range(H):
        tot = tot + gamma ** t * np.where(term, 0.0, rewards[t])
        term = term | dones[t]
    if values is not None:
        tot = tot + np.where(term, 0.0, gamma ** H * np.asarray(values, np.float64))
    return tot.reshape(pop, P).mean(axis=1), tot
