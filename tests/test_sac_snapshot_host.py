"""The two rules the SAC agent side keeps in one place each, on the host (no GPU):
  * WHEN the engine's snapshot of an actor / a critic is re-taken -- the ordered library calls of a scripted sequence over the recording
    engine of test_engine_binding_host, against the list the parent of this rule's refactoring recorded for the same script;
  * WHERE a transition's floats live -- a row written through ``pack_sac_batch`` against the row read through ``staging_views`` of a
    ``DeviceReplayBuffer`` holding the same transition."""
import numpy as np
import pytest
import torch

import hipets
import sac_restatement as sr
from hipets import mbpo
from test_engine_binding_host import ACT, OBS, eng, make_spec  # noqa: F401  (eng: the fixture)

WATCHED = ("hipets_policy_set", "hipets_critic_set", "hipets_policy_act", "hipets_critic_q")


def snapshot_script(eng):
    """Two actors alternating on one engine; a critic and a target critic alternating; the objective's refresh_agent(force=False) before
    and after a parameter ``_version`` bump, an ``engine.sac_updates`` bump and a foreign owner in either slot.  Returns the recorded
    WATCHED symbols, a "--" between the steps."""
    eng.sac_updates = 0  # (Engine.__init__'s)
    log = []

    def step():
        log.extend(s for s, _ in eng._lib.calls if s in WATCHED)
        log.append("--")
        eng._lib.calls.clear()

    sac, other = sr.TinySAC(OBS, ACT, 4), sr.TinySAC(OBS, ACT, 4)
    obs, act = torch.zeros(5, OBS), torch.zeros(5, ACT)
    a1, a2 = hipets.SACActor(sac, engine=eng), hipets.SACActor(other, engine=eng)
    step()  # two constructions
    for actor in (a1, a1, a2, a2, a1):  # an actor re-sets only when the other one sits in the slot
        actor.act_device(obs)
    step()
    a1.act_device(obs, sample=True)
    a1.refresh()
    a1.act_device(obs)
    step()
    c, ct = hipets.SACCritic(sac, engine=eng), hipets.SACCritic(sac, engine=eng, target=True)
    step()
    for critic in (c, c, ct, ct, c):
        critic.q(obs, act)
    step()
    assert ct.stale() and not c.stale()
    fn = hipets.ValueTrajectoryEvalFn(make_spec(), 2, agent=sac, engine=eng, mode="fast")
    step()  # the objective's own actor and critic
    fn.refresh_agent(force=False)
    step()  # nothing moved
    fn._terminal(torch.zeros(1, 5, OBS))
    step()
    with torch.no_grad():
        sac.policy.linear1.weight.add_(1.0)  # a parameter's _version
    fn.refresh_agent(force=False)
    fn.refresh_agent(force=False)
    step()
    with torch.no_grad():
        sac.critic.linear4.bias.add_(1.0)
    fn.refresh_agent(force=False)
    fn.refresh_agent(force=False)
    step()
    eng.sac_updates += 1  # what Engine.sac_update leaves behind: no version moved
    fn.refresh_agent(force=False)
    fn.refresh_agent(force=False)
    step()
    a2.act_device(obs)  # foreign owners in both slots
    ct.q(obs, act)
    step()
    fn._terminal(torch.zeros(1, 5, OBS))
    step()
    fn.refresh_agent()  # forced
    step()
    tfn = hipets.ValueTrajectoryEvalFn(make_spec(), 2, agent=sac, engine=eng, mode="fast", target_critic=True)
    step()
    with torch.no_grad():
        sac.critic.linear1.weight.add_(1.0)  # the target's snapshot watches the live critic
    tfn.refresh_agent(force=False)
    step()
    fn.refresh_agent(force=False)  # ... and the first objective lost both slots to the second, and saw the critic move
    step()
    return log


# recorded by running snapshot_script at the parent commit of the refactoring that introduced hipets.sac's one snapshot rule
PS, CS, PA, CQ = WATCHED
RECORDED_STEPS = [
    [PS, PS],
    [PS, PA, PA, PS, PA, PA, PS, PA],
    [PA, PS, PA],
    [CS, CS],
    [CS, CQ, CQ, CS, CQ, CQ, CS, CQ],
    [PS, CS],
    [],
    [PA, CQ],
    [PS],
    [CS],
    [PS, CS],
    [PS, PA, CS, CQ],
    [PS, CS, PA, CQ],
    [PS, CS],
    [PS, CS],
    [CS],
    [PS, CS],
]
RECORDED = [s for step in RECORDED_STEPS for s in step + ["--"]]


def test_resnapshots_are_the_recorded_sequence(eng):  # noqa: F811
    assert snapshot_script(eng) == RECORDED


@pytest.mark.parametrize("cap", (1, 5))
@pytest.mark.parametrize("obs_dim,act_dim", ((1, 1), (3, 2), (17, 6)))
def test_one_transition_layout(obs_dim, act_dim, cap):
    g = np.random.default_rng(obs_dim * 100 + act_dim * 10 + cap)
    for done in (False, True):
        tr = (g.normal(size=(1, obs_dim)).astype(np.float32), g.normal(size=(1, act_dim)).astype(np.float32),
              g.normal(size=(1, obs_dim)).astype(np.float32), g.normal(size=1).astype(np.float32), np.array([done]), np.array([False]))
        buf = hipets.DeviceReplayBuffer(cap, (obs_dim,), (act_dim,), device="cpu")
        for _ in range(cap):  # (the transition ends up in the last row written: row cap - 1)
            buf.add_batch(*tr)
        i = cap - 1
        obs, action, next_obs, reward, flag = (v[i] for v in mbpo.staging_views(buf.storage, cap, obs_dim, act_dim))
        assert buf.storage.numel() == cap * buf.width
        for reverse in (False, True):
            row = mbpo.pack_sac_batch(tr, reverse)[0]
            assert row.shape == (buf.width,)
            mask = (flag == 0).to(torch.float32) if reverse else flag
            read = torch.cat([obs, action, next_obs, reward[None], mask[None]]).numpy()
            assert np.array_equal(row, read)  # column for column
            assert np.array_equal(row, buf.gather([i], reverse)[0].numpy())
