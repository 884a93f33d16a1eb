"""TEST INFRASTRUCTURE ONLY -- the PlaNet oracle (oracle/planet_oracle.py) evaluated in float64, the cases of the per-step parity tests
(tests/test_gpu_planet_parity.py) and a Python restatement of the kernel's LDS row layout (hipets_planet_set_model in model.hip).

The oracle computes in the dtype of its tensors: a copy of a PlaNetOracleModel with every tensor cast to double, fed double inputs, is
the f64 evaluation of the same rollout.  tests/test_planet_f64_host.py checks on the CPU what the GPU tests rest on: that the f32 oracle
sits well inside T1 of this reference for the free-running cases, that the saturated case really saturates, and that the chosen shapes
reach every tail length of every op."""
import dataclasses

import torch

from oracle import planet_oracle as pl

T1 = dict(rtol=1e-5, atol=2e-6)  # the project's per-step tolerance (tests/test_gpu_step.py)
CONF = (30, 6, 200, 200)  # conf/dynamics_model/planet.yaml: latent, action, belief, hidden

# (latent, action, belief, hidden): every max() of the segment layout decided by each of its arguments at least once, dimensions of 1,
# exact tiles, one past a tile; over all of them every op sees every tail length 1..4 (test_planet_f64_host.py)
EDGE_SHAPES = [
    (1, 1, 1, 1),        # every dimension 1; widD decided by its floor of 16
    (3, 1, 5, 40),       # hidden > 3 * belief
    (40, 2, 8, 12),      # 2 * latent > 3 * belief
    (16, 16, 16, 16),    # every K and N an exact tile
    (17, 15, 33, 65),    # one past a tile everywhere
    (5, 3, 64, 130),     # belief < hidden < 3 * belief
    (7, 2, 22, 19),      # ragged, belief > hidden
    (14, 3, 28, 44),     # three k-steps in the last chunk of the belief, hidden and belief + latent ops
]
# conf's tile counts and row stride without conf's dimensions: these run the STATIC instance
STATIC_SHAPES = [(31, 5, 199, 203), (29, 7, 202, 193), (32, 16, 198, 208), (25, 8, 202, 193)]
# conf's row stride, one tile off in one op: the generic instance
NEAR_SHAPES = [(30, 6, 200, 209),   # 14 hidden tiles
               (33, 6, 200, 200)]   # 5 prior-output tiles
SATURATED_SHAPES = [CONF, (7, 2, 22, 19), (17, 15, 33, 65)]

TILE = 16
LDS_BYTES = 160 * 1024        # the dynamic LDS a workgroup of the kernel may opt in to on gfx950
PLANET_OP_BYTES = 72          # sizeof(PlanetOp): a 56-byte LayerMeta and four ints
N_OPS = 8


def up16(x):
    return (x + 15) // 16 * 16


def op_dims(dims):
    """(K, N) of the eight linear ops in the order embed, input gates, hidden gates, prior 1, prior 2, reward 1, 2, 3."""
    L, A, Hb, F = dims
    return [(L + A, Hb), (Hb, 3 * Hb), (Hb, 3 * Hb), (Hb, F), (F, 2 * L), (Hb + L, F), (F, F), (F, 1)]


def tail_steps(K):
    """Real k-steps (of 4) in an op's last k chunk of 16."""
    return (K - 1) % 16 // 4 + 1


def row_floats(dims):
    """LDS row stride of a model in floats: five segments of padded widths, then the next value that is 8 modulo 64."""
    L, A, Hb, F = dims
    wid = [up16(L + A), up16(max(Hb, F)), up16(max(3 * Hb, F)), up16(max(3 * Hb, 2 * L, 16)), up16(Hb + L)]
    ld = sum(wid)
    while ld % 64 != 8:
        ld += 4
    return ld


def smem_bytes(ld):
    """planet_smem_bytes: 16 rows, 16 totals, 16 row ids, the op table, rounded up to 8, and the profiler's 512 bytes at the end."""
    n = TILE * ld * 4 + 2 * TILE * 4 + PLANET_OP_BYTES * N_OPS
    return (n + 7) // 8 * 8 + 8 * 16 * 8


def tile_counts(dims):
    """Per op (column tiles, k chunks): what selects the STATIC instance together with the row stride."""
    return [(up16(N) // TILE, up16(K) // TILE) for K, N in op_dims(dims)]


def runs_static(dims):
    return row_floats(dims) == row_floats(CONF) and tile_counts(dims) == tile_counts(CONF)


def widest_square_models(lds_bytes=LDS_BYTES):
    """((30, 6, n, n) with the widest row that fits lds_bytes, the next n whose row does not fit): n in steps of 8."""
    n = 8
    while smem_bytes(row_floats((30, 6, n + 8, n + 8))) <= lds_bytes:
        n += 8
    return (30, 6, n, n), (30, 6, n + 8, n + 8)


def to_f64(pm):
    """A copy of the model with every tensor in PLANET_TENSORS cast to double."""
    return dataclasses.replace(pm, **{k: getattr(pm, k).double() for k in pl.PLANET_TENSORS})


def rollout_traced(pm, actions, latent0, belief0, P, eps):
    """pl.planet_rollout in the dtype of pm's tensors: (returns [pop], latent [H, B, L], belief [H, B, Hb], rewards [H, B]).  The returns are
    summed here from the traced rewards in that dtype (the oracle's own running total is a float32 tensor whatever the model's dtype)."""
    dt = pm.w_embed.dtype
    tr = {}
    pl.planet_rollout(pm, actions.to(dt), latent0.to(dt), belief0.to(dt), P, eps=eps.to(dt), trace=tr)
    rewards = torch.stack(tr["rewards"]).squeeze(-1)
    returns = rewards.sum(0).reshape(-1, P).mean(dim=1)
    return returns, torch.stack(tr["latent"]), torch.stack(tr["belief"]), rewards


def free_case(dims, H, pop=19, P=2, seed=None):
    """A free-running rollout of a Xavier-initialised model: 19 candidates x 2 particles = two full row tiles and a ragged one of 6."""
    L, A, Hb, F = dims
    seed = sum(dims) if seed is None else seed
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    latent0, belief0 = torch.randn(1, L, generator=g) * 0.3, torch.randn(1, Hb, generator=g) * 0.3
    actions = torch.rand(pop, H, A, generator=g) * 2 - 1
    eps = torch.randn(H, pop * P, L, generator=g)
    return pm, actions, latent0, belief0, eps


def saturated_case(dims, rows=48, seed=None):
    """One step of a large-weight model from large start states, one start state per row: GRU gates at both rails, raw std values from
    where softplus flushes to 0 to beyond its x > 20 branch."""
    L, A, Hb, F = dims
    seed = sum(dims) + 100 if seed is None else seed
    pm = pl.make_synthetic_planet(L, A, Hb, F, seed=seed, scale=4.0)
    pm.b_prior2[L:] += torch.linspace(-30, 30, L)
    g = torch.Generator().manual_seed(seed + 1)
    latent0 = torch.randn(rows, L, generator=g) * 3
    belief0 = torch.tanh(torch.randn(rows, Hb, generator=g) * 3)
    actions = torch.rand(rows, 1, A, generator=g) * 2 - 1
    eps = torch.randn(1, rows, L, generator=g)
    return pm, actions, latent0, belief0, eps


def step_traced(pm, actions, latent0, belief0, eps):
    """One pl.planet_step from per-row start states in the dtype of pm's tensors: (next latent, next belief, reward [rows], raw std)."""
    dt = pm.w_embed.dtype
    latent, reward, belief = pl.planet_step(pm, latent0.to(dt), belief0.to(dt), actions[:, 0].to(dt), eps[0].to(dt))
    hid = torch.relu(torch.nn.functional.linear(belief, pm.w_prior1, pm.b_prior1))
    raw_std = torch.nn.functional.linear(hid, pm.w_prior2, pm.b_prior2)[:, pm.latent_size:]
    return latent, belief, reward.squeeze(-1), raw_std


def t1_excess(got, ref, frac=1.0):
    """max over entries of |got - ref| / (frac * (atol + rtol |ref|)): <= 1 means inside that fraction of T1."""
    ref = ref.double()
    return ((got.double() - ref).abs() / (frac * (T1["atol"] + T1["rtol"] * ref.abs()))).max().item()
