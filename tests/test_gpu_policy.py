"""The SAC actor kernel (hipets_policy_set / _act / _normals) and the transition compaction (hipets_compact_transitions) on the GPU.

Actor: every case of policy_restatement.GPU_CASES against the float64 restatement -- the mean / log_std taps and the actions of
evaluate, sample with an injected eps, and sample with in-kernel eps replayed through policy_normals.  The bound of a case is
T1 x max(1, 4 u): u = the share of T1 that torch CPU's own float32 forward of the reference's GaussianPolicy uses on the case's rows
against the same restatement (recorded per row in tests/golden/sac_policy_cases.npz by tests/make_policy_golden.py; a case takes the
largest over the rows it runs), the factor 4 for another, equally valid float32 summation order.  Compaction: numpy's boolean indexing, bit for bit."""
import os

import numpy as np
import pytest
import torch

import hipets
import policy_restatement as pr
from conftest import GOLDEN
from hipets import mbpo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_GOLD = {}


def gold():
    if not _GOLD:
        _GOLD.update(np.load(os.path.join(GOLDEN, "sac_policy_cases.npz")))
    return _GOLD


class BarePolicy(torch.nn.Module):
    """A module shaped like GaussianPolicy (pytorch_sac_pranz24/model.py:66-86) holding a case's weights"""

    def __init__(self, w, device=DEV):
        super().__init__()
        hid, obs = w["w1"].shape
        act = w["wm"].shape[0]
        self.linear1, self.linear2 = torch.nn.Linear(obs, hid), torch.nn.Linear(hid, hid)
        self.mean_linear, self.log_std_linear = torch.nn.Linear(hid, act), torch.nn.Linear(hid, act)
        with torch.no_grad():
            for lin, k in ((self.linear1, "1"), (self.linear2, "2"), (self.mean_linear, "m"), (self.log_std_linear, "s")):
                lin.weight.copy_(torch.from_numpy(w["w" + k]))
                lin.bias.copy_(torch.from_numpy(w["b" + k]))
        self.action_scale, self.action_bias = torch.from_numpy(w["action_scale"]).to(device), torch.from_numpy(w["action_bias"]).to(device)
        self.to(device)


def assert_within(got, ref64, u_rows, what):
    """|got - ref| <= T1 x max(1, 4 u), u = the largest share of T1 torch CPU's float32 forward uses on the rows of this case; prints
    the worst share of plain T1"""
    share = pr.t1_share(got.cpu().numpy(), ref64)
    u = float(np.max(u_rows))
    factor = max(1.0, 4.0 * u)
    print(f"  {what}: {float(share.max()):.3f} of T1 at worst (torch CPU f32 itself: u = {u:.3f}; bound {factor:.2f} x T1)")
    assert np.isfinite(share).all() and (share <= factor).all(), f"{what}: {float(share.max()):.3f} of T1, bound {factor:.2f}"


@pytest.mark.parametrize("name,obs_dim,hid,act,batch", pr.GPU_CASES, ids=[c[0] for c in pr.GPU_CASES])
def test_actor_matches_the_f64_restatement(engine, name, obs_dim, hid, act, batch):
    w, obs, eps = pr.make_case(name, obs_dim, hid, act)
    assert engine.policy_set(BarePolicy(w)) == (obs_dim, hid, act)
    R = engine.policy_geometry(10 ** 6)[0]
    assert R in (1, 2, 4) and engine.policy_geometry(10 ** 6)[1] <= 160 * 1024
    B = {"R-1": 16 * R - 1, "R+1": 16 * R + 1}.get(batch, batch)
    assert engine.policy_geometry(B)[0] == min(R, next((r for r in (1, 2, 4) if 16 * r >= B), 4))  # no more tiles than the batch fills
    obs, eps, u = obs[:B], eps[:B], gold()["u_" + name][:B]
    x, e = torch.from_numpy(obs).to(DEV), torch.from_numpy(eps).to(DEV)
    print(f"{name}: B {B}, row tiles {R}")
    r_eval, r_mean, r_ls = pr.actor_f64(w, obs)
    a, mean, ls = engine.policy_act(x, taps=True)
    assert_within(mean, r_mean, u, "mean tap")
    assert_within(ls, r_ls, u, "log_std tap")
    assert_within(a, r_eval, u, "evaluate")
    assert_within(engine.policy_act(x, sample=True, eps=e), pr.actor_f64(w, obs, True, eps)[0], u, "sample, injected eps")
    got = engine.policy_act(x, sample=True, seed=11, stream_id=5)
    drawn = engine.policy_normals(B, act, 11, 5)
    assert_within(got, pr.actor_f64(w, obs, True, drawn.cpu().numpy())[0], u, "sample, in-kernel eps")
    # the draws: standard normals, another table for another stream, independent of the rollouts' table of the same (seed, stream)
    assert torch.isfinite(drawn).all() and not torch.equal(drawn, engine.policy_normals(B, act, 11, 6))
    # determinism: the same call twice gives the same bits
    assert torch.equal(got, engine.policy_act(x, sample=True, seed=11, stream_id=5))
    assert torch.equal(a, engine.policy_act(x))


def test_policy_normals_are_standard_and_their_own_key_domain(engine):
    n = engine.policy_normals(20000, 6, 3, 9).cpu()
    assert abs(float(n.mean())) < 0.02 and abs(float(n.std()) - 1.0) < 0.02
    from oracle import pets_oracle as po
    from conftest import to_spec

    engine.set_model(to_spec(po.make_synthetic_model(17, 6, ensemble_size=3, hid=16, seed=0), 17, 6))
    model = engine.fast_normals(1, 20000, 3, 9).cpu()[0][:, :6]
    assert not torch.equal(n, model) and abs(float((n * model).mean())) < 0.02


def test_sac_actor_act_is_row_zero_of_the_batched_call(engine):
    """SACActor.act, numpy in and out: batched=False equals row 0 of the batched call; evaluate and sample; a policy on the CPU"""
    w, obs, _ = pr.make_case("o17_h200_a6_b1000", 17, 200, 6)
    for device in (DEV, "cpu"):
        actor = hipets.SACActor(BarePolicy(w, device), engine=engine, seed=3)
        one = actor.act(obs[0])
        many = actor.act(obs[:50], batched=True)
        assert one.shape == (6,) and many.shape == (50, 6) and one.dtype == np.float32
        assert np.array_equal(one, many[0])
        share = pr.t1_share(many, pr.actor_f64(w, obs[:50])[0])
        assert (share <= max(1.0, 4.0 * float(gold()["u_o17_h200_a6_b1000"][:50].max()))).all()
        s1 = actor.act(obs[:50], sample=True, batched=True)
        assert actor.last_draw == (3, 1) and not np.array_equal(s1, many)
        assert not np.array_equal(s1, actor.act(obs[:50], sample=True, batched=True)) and actor.last_draw == (3, 2)
        again = hipets.SACActor(BarePolicy(w, device), engine=engine, seed=3)
        assert np.array_equal(s1, again.act(obs[:50], sample=True, batched=True))
        assert np.array_equal(s1[0], hipets.SACActor(BarePolicy(w, device), engine=engine, seed=3).act(obs[0], sample=True))


def test_refresh_picks_up_new_weights_and_actors_share_an_engine(engine):
    w, obs, _ = pr.make_case("o5_h16_a2_b16", 5, 16, 2)
    w2, _, _ = pr.make_case("o5_h16_a2_b16_other", 5, 16, 2)
    pa, pb = BarePolicy(w), BarePolicy(w2)
    a, b = hipets.SACActor(pa, engine=engine), hipets.SACActor(pb, engine=engine)
    ra, rb = a.act(obs[:16], batched=True), b.act(obs[:16], batched=True)
    assert not np.array_equal(ra, rb) and np.array_equal(ra, a.act(obs[:16], batched=True))
    with torch.no_grad():
        pa.mean_linear.bias.add_(0.5)
    assert np.array_equal(ra, a.act(obs[:16], batched=True))  # a snapshot ...
    a.refresh()
    assert not np.array_equal(ra, a.act(obs[:16], batched=True))  # ... until refresh


def test_policy_argument_refusal(engine):
    w, obs, _ = pr.make_case("o5_h16_a2_b16", 5, 16, 2)
    engine.policy_set(BarePolicy(w))
    with pytest.raises(ValueError):
        engine.policy_act(torch.zeros(4, 6, device=DEV))
    with pytest.raises(ValueError):
        engine.policy_act(torch.zeros(4, 5, device=DEV), sample=True, eps=torch.zeros(4, 3, device=DEV))
    z = torch.zeros(8, device=DEV)
    for bad in (dict(obs_dim=0), dict(obs_dim=513), dict(hidden=0), dict(hidden=1025), dict(act_dim=0), dict(act_dim=33)):
        kw = dict(obs_dim=5, hidden=16, act_dim=2, **{n: z for n in ("w1", "b1", "w2", "b2", "wm", "bm", "ws", "bs", "action_scale", "action_bias")})
        kw.update(bad)
        with pytest.raises(hipets.HipetsError) as err:
            engine._call("hipets_policy_set", **kw)
        assert err.value.kind == hipets.ERR_INVALID_ARGUMENT
    with pytest.raises(hipets.HipetsError) as err:
        engine._call("hipets_policy_act", obs=z, batch=0, sample=0, seed=0, stream_id=0, eps=None, actions=z, mean_out=None, log_std_out=None)
    assert err.value.kind == hipets.ERR_INVALID_ARGUMENT
    engine.policy_set(BarePolicy(w))  # (a refused set leaves the engine without a policy: set one for whoever comes next)


# ---- compaction ----------------------------------------------------------------------------------------------------------------------
def _masks(N, kind, rng):
    if kind == "all":
        return np.zeros(N, bool)
    if kind == "none":
        return np.ones(N, bool)
    if kind == "last":
        m = np.ones(N, bool)
        m[-1] = False
        return m
    return rng.random(N) < 0.4


SCAN_WIDTH_ROWS = 256 * 1024  # rows one pass of the scan covers (256-row blocks, 1024 of them)


@pytest.mark.parametrize("kind", ["all", "none", "last", "random"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000, SCAN_WIDTH_ROWS + 257])
def test_compaction_is_numpy_boolean_indexing(engine, N, kind):
    """three consecutive steps into one staging area: rows, offsets, counts and accum_dones"""
    od, ad = (3, 2) if N > 1000 else (11, 3)
    rng = np.random.default_rng(N + len(kind))
    W = 2 * od + ad + 2
    accum = _masks(N, kind, rng)
    steps = []
    for _ in range(3):
        f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
        steps.append((f(N, od), f(N, ad), f(N, od), f(N), rng.random(N) < 0.3))
    steps[1][3][0] = np.float32("nan")  # (a copy keeps a NaN's bits)
    cap = 3 * N
    staging = torch.full((cap * W,), -7.0, device=DEV)
    offset, counts = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV)
    acc_t = torch.from_numpy(accum.astype(np.uint8)).to(DEV)
    want, want_counts = [], []
    for i, (o, a, no, r, d) in enumerate(steps):
        t = [torch.from_numpy(v).to(DEV) for v in (o, a, no, r)]
        engine.compact_transitions(t[0], t[1], t[2], t[3], torch.from_numpy(d).to(DEV), acc_t, staging, cap, offset, counts[i:i + 1])
        keep = ~accum
        want.append((o[keep], a[keep], no[keep], r[keep], d[keep].astype(np.float32)))
        want_counts.append(int(keep.sum()))
        accum = accum | d
        assert np.array_equal(acc_t.cpu().numpy().astype(bool), accum)
        assert int(offset.item()) == sum(want_counts)
    assert counts.cpu().tolist() == want_counts
    total = sum(want_counts)
    for got, parts in zip(mbpo.staging_views(staging.cpu().numpy(), cap, od, ad), zip(*want)):  # obs, action, next_obs, reward, done
        want_rows = np.concatenate(parts)
        assert np.array_equal(got[:total].view(np.uint32), want_rows.view(np.uint32))
        assert (got[total:] == -7.0).all()


def test_compaction_drops_rows_past_the_capacity(engine):
    N, od, ad = 300, 4, 2
    rng = np.random.default_rng(0)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)  # noqa: E731
    W, cap = 2 * od + ad + 2, 100
    staging = torch.full((cap * W + 64,), -7.0, device=DEV)
    offset, count = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    o, r = f(N, od), f(N)
    engine.compact_transitions(o, f(N, ad), f(N, od), r, torch.zeros(N, dtype=torch.bool, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV),
                               staging, cap, offset, count)
    assert int(count.item()) == N and int(offset.item()) == N
    views = mbpo.staging_views(staging[:cap * W], cap, od, ad)
    assert torch.equal(views[0], o[:cap]) and torch.equal(views[3], r[:cap]) and (views[4] == 0).all() and (staging[cap * W:] == -7.0).all()
