"""hipets.SACUpdater / hipets_sac_update on the MI355X against our float64 / float32 restatement of one SAC update
(tests/sac_restatement.py).  Tolerances are the suite's self-calibrated rule (train_restatement.check): the kernels' distance from the
float64 restatement may be at most 4x the float32 restatement's own distance, plus a 1e-7 floor.  Every case's inputs meet
sac_restatement.check_kinks (asserted when the case is built): no ReLU, min(q1, q2) or clamp argument within 1e-4 of its kink."""
import pytest
import torch

import hipets
import sac_restatement as sr
import train_restatement as tr
from hipets import _lib, mbpo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = sr.HP["lr"]


def _run(engine, case, route="many"):
    """The case's updates on the GPU with the case's own normal tables: (agent, updater, [5-tuples])"""
    sac, memory = sr.agent_for(case, DEV)
    up = hipets.SACUpdater(sac, engine=engine)
    B = case["shape"][3]
    eps = [(b["eps_next"].float().to(DEV), b["eps_cur"].float().to(DEV)) for b in case["inputs"][1]]
    if route == "many":
        res = up.update_many([memory] * len(eps), B, case["first_update"], reverse_mask=True, eps=eps)
    else:
        res = [up.update_many([memory], B, case["first_update"] + i, reverse_mask=True, eps=[e])[0] for i, e in enumerate(eps)]
    torch.cuda.synchronize()
    return sac, up, res


def _state(sac, n, key):
    return sac.optimizer_of(n).state[sac.params()[n]][key]


@pytest.mark.parametrize("name", sr.ONE_UPDATE + ["fixed_alpha", "clamp"])
def test_one_update_matches_restatement(engine, name):
    case = sr.build_case(name)
    sac, up, res = _run(engine, case)
    f32, f64, o32, o64 = case["f32"], case["f64"], case["out32"][0], case["out64"][0]
    f32r, o32r = case["f32r"], case["out32r"][0]  # the float32 restatement with the batch summed in the other order
    taps = up.forward_taps(case["shape"][3])
    for k in ("q1", "q2", "y", "log_pi_next", "log_pi"):
        tr.check(taps[k], o32[k], o64[k], f"{name}: {k}", [o32r[k]])
    for i, k in enumerate(("qf1_loss", "qf2_loss", "policy_loss", "alpha_loss", "alpha")):
        tr.check(torch.tensor(res[0][i], dtype=torch.float64), o32["losses"][i], o64["losses"][i], f"{name}: {k}", [o32r["losses"][i]])
    # the gradients, through the first-step moments m = (1 - b1) g and v = (1 - b2) g^2
    trained = sr.POLICY + sr.CRITIC + (("log_alpha",) if case["tuning"] else ())
    for n in trained:
        tr.check(_state(sac, n, "exp_avg"), f32["m"][n], f64["m"][n], f"{name}: m {n}", [f32r["m"][n]])
        tr.check(_state(sac, n, "exp_avg_sq"), f32["v"][n], f64["v"][n], f"{name}: v {n}", [f32r["v"][n]])
    # the parameters, pinned to Adam's formula on the kernels' OWN moments (tests/test_gpu_trainer.py:39-53): a gradient that cancels
    # to rounding moves a parameter anywhere in [-lr, lr], whatever the summation order
    p0 = case["inputs"][0]
    bc2s = (1 - 0.999) ** 0.5
    live = sac.params()
    for n in trained:
        m, v = _state(sac, n, "exp_avg").double().cpu(), _state(sac, n, "exp_avg_sq").double().cpu()
        expect = p0[n].float().double() - (LR / (1 - 0.9)) * m / (v.sqrt() / bc2s + 1e-8)
        assert (live[n].detach().double().cpu() - expect).abs().max().item() <= 1e-7, f"{name}: {n}: Adam step off its own moments"
        assert float(_state(sac, n, "step")) == 1.0
    # the soft update, with the critic's NEW values (utils.soft_update): two float32 products and their sum, each rounded once -- at most
    # three half-ulps of the largest operand away from the same expression in double
    for c, t in zip(sr.CRITIC, sr.TARGET):
        new = live[c].detach().double().cpu()
        expect = p0[t].float().double() * float(torch.tensor(1.0 - sr.HP["tau"], dtype=torch.float32)) + \
            new * float(torch.tensor(sr.HP["tau"], dtype=torch.float32))
        bound = 3 * 2.0 ** -24 * max(1.0, new.abs().max().item(), p0[t].abs().max().item())
        assert (live[t].detach().double().cpu() - expect).abs().max().item() <= bound, f"{name}: target {t}"
    if case["tuning"]:
        assert sac.alpha is up._alpha and abs(float(sac.alpha) - float(sac.log_alpha.detach().exp())) <= 1e-6
    else:
        assert sac.alpha == sr.HP["alpha"] and res[0][3] == 0.0 and abs(res[0][4] - sr.HP["alpha"]) < 1e-7


@pytest.mark.parametrize("name", ["twenty_i1", "twenty_i3"])
def test_twenty_updates_two_routes(engine, name):
    case = sr.build_case(name)
    sac, up, res = _run(engine, case, "many")
    f32, f64, f32r = case["f32"], case["f64"], case["f32r"]
    live = sac.params()
    for n in sr.POLICY + sr.CRITIC + sr.TARGET + ("log_alpha",):
        tr.check(live[n].detach(), f32["p"][n], f64["p"][n], f"{name}: {n} after 20 updates", [f32r["p"][n]])
    l32, l64, l32r = (torch.stack([o["losses"] for o in case[k]]) for k in ("out32", "out64", "out32r"))
    for i, k in enumerate(("qf1_loss", "qf2_loss", "policy_loss", "alpha_loss", "alpha")):
        tr.check(torch.tensor(res, dtype=torch.float64)[:, i], l32[:, i], l64[:, i], f"{name}: {k} of the 20 updates", [l32r[:, i]])
    # update_many and 20 single calls agree to the bit, and so does a repeated run
    for route in ("single", "many"):
        sac2, _, res2 = _run(engine, case, route)
        assert res2 == res, f"{name}: results of route {route}"
        for n, t in sac2.params().items():
            assert torch.equal(t.detach(), live[n].detach()), f"{name}: {n} differs on route {route}"
        for n in sr.POLICY + sr.CRITIC + ("log_alpha",):
            assert torch.equal(_state(sac2, n, "exp_avg_sq"), _state(sac, n, "exp_avg_sq")) and float(_state(sac2, n, "step")) == 20.0


class _Logger:
    def __init__(self):
        self.rows = []

    def log(self, key, value, step):
        self.rows.append((key, float(value), step))


def test_state_hand_over_logger_and_seeded_draws(engine):
    case = sr.build_case("s17_6_17_17")
    obs, act, hid, B = case["shape"]
    sac, memory = sr.agent_for(case, DEV)
    up = hipets.SACUpdater(sac, engine=engine)
    actor = hipets.SACActor(sac, engine=engine)
    probe = case["inputs"][1][0]["state"].float().to(DEV)
    before = actor.act_device(probe).clone()
    K, log = 3, _Logger()
    torch.manual_seed(5)
    res = [up.update_parameters(memory, B, u, log, reverse_mask=True) for u in range(K)]
    assert [r[0] for r in log.rows] == list(mbpo.LOG_KEYS) * K and [r[2] for r in log.rows] == [u for u in range(K) for _ in mbpo.LOG_KEYS]
    assert all(len(r) == 5 and all(isinstance(v, float) for v in r) for r in res)
    # a seeded run sees the reference's stream: the next-state table first, then the state table, drawn as Normal.rsample draws them
    torch.manual_seed(5)
    eps = [(torch.empty(B, act, device=DEV).normal_(), torch.empty(B, act, device=DEV).normal_()) for _ in range(K)]
    sac2, memory2 = sr.agent_for(case, DEV)
    res2 = hipets.SACUpdater(sac2, engine=engine).update_many([memory2] * K, B, 0, reverse_mask=True, eps=eps)
    assert res2 == res
    # the optimizers' state is torch's own: step counts the updates, the moments are the storage the kernels wrote
    for opt in (sac.critic_optim, sac.policy_optim, sac.alpha_optim):
        sd = opt.state_dict()["state"]
        assert len(sd) == len(opt.param_groups[0]["params"])
        for i, p in enumerate(opt.param_groups[0]["params"]):
            assert float(sd[i]["step"]) == K and sd[i]["exp_avg"].data_ptr() == opt.state[p]["exp_avg"].data_ptr()
            assert sd[i]["exp_avg"].data_ptr() in up._bound[0] and sd[i]["exp_avg_sq"].data_ptr() in up._bound[0]
            assert sd[i]["exp_avg_sq"].abs().sum().item() > 0
    # SACActor.refresh() sees the new policy without any call on the updater
    actor.refresh()
    after = actor.act_device(probe)
    with torch.no_grad():
        h = torch.relu(sac.policy.linear2(torch.relu(sac.policy.linear1(probe))))
        want = torch.tanh(sac.policy.mean_linear(h)) * sac.policy.action_scale + sac.policy.action_bias
    assert (after - want).abs().max().item() < 1e-5 and (after - before).abs().max().item() > 1e-5
    # one stock torch update afterwards runs, on the same tensors
    out = sac.update_parameters(memory, B, K, None, reverse_mask=True)
    assert all(v == v for v in out) and float(sac.critic_optim.state[sac.critic.linear1.weight]["step"]) == K + 1
    # ... and the updater carries on from there (the stock update left a new alpha tensor behind)
    more = up.update_parameters(memory, B, K + 1, None, reverse_mask=True)
    assert all(v == v for v in more) and float(sac.critic_optim.state[sac.critic.linear1.weight]["step"]) == K + 2


def test_argument_refusal_through_the_abi(engine):
    case = sr.build_case("s5_2_15_15")
    obs, act, hid, B = case["shape"]
    sac, memory = sr.agent_for(case, DEV)
    up = hipets.SACUpdater(sac, engine=engine)
    up.update_parameters(memory, B, 0, reverse_mask=True)  # (binds the engine)
    width = 2 * obs + act + 2
    big = _lib.SAC_MAX_BATCH + 1
    with pytest.raises(hipets.HipetsError) as exc:
        engine.sac_update(torch.zeros(big, width, device=DEV), torch.zeros(big, act, device=DEV), torch.zeros(big, act, device=DEV), 0, (0, 0, 0),
                          (LR, LR, LR), torch.zeros(8, device=DEV))
    assert exc.value.kind == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(hipets.HipetsError) as exc:
        engine.sac_forward_taps(B + 1)
    assert exc.value.kind == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(hipets.HipetsError) as exc:
        engine.sac_bind((obs, act, hid), True, 0.99, 0.005, -2.0, 1, [0.9, 0.999, 1e-8] * 3, [1] * 5)
    assert exc.value.kind == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(hipets.UnsupportedModelError):
        up.update_parameters(memory, big, 1, reverse_mask=True)
    up.update_parameters(memory, B, 1, reverse_mask=True)  # the refused bind left no agent in the engine: the updater binds again
    torch.cuda.synchronize()
