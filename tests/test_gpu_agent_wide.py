"""kernel="wide" (csrc/agent_wide.hip, hipets_set_agent_kernel) on the MI355X: the actor's and the critic's forward at 64 rows per
workgroup against the float64 restatements under the tile kernels' rule -- T1 x max(1, 4 u), u = torch CPU's own float32 share of T1
on the case's rows --, batch independence and repeatability bit for bit, the switch, and the in-kernel draws.  Shapes: fewer column
tiles than waves (hidden 20), tiles dealt unevenly over the 8 waves in a chunk that is not full (136), the full accumulator file over
several chunks (1024); a first-layer K below 16 (3) and off a multiple of 16 (35, 393); heads in one tile and in several (act 1, 17);
batches around the 64-row block."""
import numpy as np
import pytest
import torch

import hipets
import policy_restatement as pr
import value_restatement as vr
from hipets import _lib
from test_gpu_policy import BarePolicy, assert_within
from test_gpu_value import bare_critic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (who, first-layer K, act, hidden, batch); the critic's K = obs + act
CASES = [("actor", 3, 1, 20, 1), ("actor", 35, 17, 136, 65), ("actor", 17, 6, 1024, 130), ("actor", 393, 17, 1024, 63),
         ("actor", 3, 1, 136, 64), ("actor", 35, 17, 20, 130),
         ("critic", 3, 1, 20, 1), ("critic", 35, 17, 136, 130), ("critic", 393, 17, 1024, 65), ("critic", 23, 6, 1024, 63),
         ("critic", 3, 1, 136, 64), ("critic", 35, 17, 20, 130)]
ROWS = 130
_ACTOR = {}


def actor_case(K, act, hid):
    """(weights, obs, eps, u per row) of an actor shape, built once: u as tests/make_policy_golden.py records it"""
    key = (K, act, hid)
    if key not in _ACTOR:
        w, obs, eps = pr.make_case(f"wide_o{K}_h{hid}_a{act}", K, hid, act, rows=ROWS)
        ref = pr.actor_f64(w, obs) + (pr.actor_f64(w, obs, True, eps)[0],)
        f32 = pr.actor_f32(w, obs) + (pr.actor_f32(w, obs, True, eps)[0],)
        _ACTOR[key] = (w, obs, eps, np.max(np.concatenate([pr.t1_share(g, r) for g, r in zip(f32, ref)], axis=1), axis=1))
    return _ACTOR[key]


def critic_case(K, act, hid):
    return vr.make_critic_case(f"wide_k{K}_h{hid}", K - act, act, hid, rows=ROWS)


@pytest.mark.parametrize("who,K,act,hid,B", CASES, ids=[f"{c[0]}_k{c[1]}_a{c[2]}_h{c[3]}_b{c[4]}" for c in CASES])
def test_wide_matches_the_f64_restatement(engine, who, K, act, hid, B):
    if who == "actor":
        w, obs, eps, u = actor_case(K, act, hid)
        actor = hipets.SACActor(BarePolicy(w), engine=engine, kernel="wide")
        x, e = torch.from_numpy(obs[:B]).to(DEV), torch.from_numpy(eps[:B]).to(DEV)
        r_eval, r_mean, r_ls = pr.actor_f64(w, obs[:B])
        a, mean, ls = engine.policy_act(x, taps=True, kernel="wide")
        assert_within(mean, r_mean, u[:B], "mean tap")
        assert_within(ls, r_ls, u[:B], "log_std tap")
        assert_within(a, r_eval, u[:B], "evaluate")
        assert torch.equal(a, actor.act_device(x))
        assert_within(actor.act_device(x, sample=True, eps=e), pr.actor_f64(w, obs[:B], True, eps[:B])[0], u[:B], "sample, injected eps")
    else:
        w, obs, actions, u = critic_case(K, act, hid)
        critic = hipets.SACCritic(bare_critic(w), engine=engine, obs_dim=K - act, kernel="wide")
        r1, r2 = vr.critic_f64(w, obs[:B], actions[:B])
        q1, q2, qmin = critic.q(torch.from_numpy(obs[:B]).to(DEV), torch.from_numpy(actions[:B]).to(DEV))
        assert_within(q1, r1, u[:B], "q1")
        assert_within(q2, r2, u[:B], "q2")
        assert torch.equal(qmin, torch.where(q1 < q2, q1, q2))


@pytest.mark.parametrize("hid", [136, 1024])
def test_a_row_does_not_depend_on_its_batch(engine, hid):
    """row r of a 130-row call equals the one-row call on that row, on both sides of a block edge and in the ragged third block; a
    repeated call gives the same bits"""
    w, obs, eps, _ = actor_case(35, 17, hid)
    actor = hipets.SACActor(BarePolicy(w), engine=engine, kernel="wide")
    cw, cobs, cact, _ = critic_case(35, 17, hid)
    critic = hipets.SACCritic(bare_critic(cw), engine=engine, obs_dim=18, kernel="wide")
    x, e = torch.from_numpy(obs).to(DEV), torch.from_numpy(eps).to(DEV)
    s, a = torch.from_numpy(cobs).to(DEV), torch.from_numpy(cact).to(DEV)
    acts, (q1, q2, _) = actor.act_device(x, sample=True, eps=e), critic.q(s, a)
    assert torch.equal(acts, actor.act_device(x, sample=True, eps=e)) and torch.equal(q1, critic.q(s, a)[0])
    for r in (0, 63, 64, 129):
        assert torch.equal(actor.act_device(x[r:r + 1].contiguous(), sample=True, eps=e[r:r + 1].contiguous())[0], acts[r]), f"actor row {r}"
        o1, o2, _ = critic.q(s[r:r + 1].contiguous(), a[r:r + 1].contiguous())
        assert torch.equal(o1[0], q1[r]) and torch.equal(o2[0], q2[r]), f"critic row {r}"


def test_the_switch(engine):
    """the tile form's bits do not move across a switch to the wide form and back; an unknown kind is refused and changes nothing; the
    geometry queries follow the setting"""
    w, obs, _, _ = actor_case(17, 6, 1024)
    cw, cobs, cact, _ = critic_case(23, 6, 1024)
    engine.policy_set(BarePolicy(w))
    engine.critic_set(bare_critic(cw), 17, 6)
    x, s, a = (torch.from_numpy(v).to(DEV) for v in (obs, cobs, cact))
    tile = (engine.policy_act(x), engine.policy_act(x, kernel="tile")) + engine.critic_q(s, a)
    assert engine.policy_geometry(10 ** 6)[0] == engine.critic_geometry(10 ** 6)[0] == 1
    engine.set_agent_kernel("wide")
    try:
        with pytest.raises(hipets.HipetsError) as err:
            engine._query("hipets_set_agent_kernel", kind=2)
        assert err.value.kind == hipets.ERR_INVALID_ARGUMENT
        # still wide: 4 row tiles whatever the batch, the rule's LDS
        assert engine.policy_geometry(10 ** 6) == engine.policy_geometry(1) == (4, hipets.sac.agent_wide_geometry(17, 1024, 12)[2])
        assert engine.critic_geometry(10 ** 6) == (4, hipets.sac.agent_wide_geometry(23, 1024, 1)[2])
        assert engine.policy_geometry(10 ** 6, kernel="tile")[0] == 1
        wide = engine.policy_act(x)
        assert torch.equal(wide, engine.policy_act(x, kernel="wide")) and not torch.equal(wide, tile[0])
    finally:
        engine.set_agent_kernel("tile")
    with pytest.raises(ValueError):
        engine.policy_act(x, kernel="neither")
    assert engine.policy_geometry(10 ** 6)[0] == 1 and engine.policy_geometry(10 ** 6, kernel="wide")[0] == 4
    again = (engine.policy_act(x), engine.policy_act(x, kernel="tile")) + engine.critic_q(s, a)
    assert all(torch.equal(g, h) for g, h in zip(tile, again))


def test_in_kernel_draws_are_the_tile_forms_table(engine):
    w, obs, _, u = actor_case(35, 17, 136)
    actor = hipets.SACActor(BarePolicy(w), engine=engine, seed=11, kernel="wide")
    got = actor.act_device(torch.from_numpy(obs).to(DEV), sample=True)
    drawn = engine.policy_normals(ROWS, 17, *actor.last_draw)
    assert_within(got, pr.actor_f64(w, obs, True, drawn.cpu().numpy())[0], u, "sample, in-kernel eps")
    assert _lib.AGENT_KERNEL == {"tile": 0, "wide": 1}
