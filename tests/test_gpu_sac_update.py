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
# the hand-over test's generator seeds: its first K updates, its stock torch update, the kernels' update behind that.  Searched, as
# the cases' seeds are (tests/make_sac_update_golden.py --search-hand-over): with these device draws the K + 2 updates meet
# sr.check_kinks, which the test asserts before it compares
HAND_OVER_SEEDS = (0, 2, 1)


def _optimizers(sac):
    return (sac.critic_optim, sac.policy_optim) + ((sac.alpha_optim,) if sac.automatic_entropy_tuning else ())


def _run(engine, case, route="many", schedule=True):
    """The case's updates on the GPU with the case's own normal tables: (agent, updater, [5-tuples]).  Route "many" queues the updates
    in one update_many call (one call per stretch of equal learning rates where the case has a schedule), "single" makes a call per
    update; a schedule is applied as a scheduler applies it, through ``param_groups[0]["lr"]`` between calls (``schedule=False``: not)."""
    sac, memory = sr.agent_for(case, DEV)
    up = hipets.SACUpdater(sac, engine=engine)
    B = case["shape"][3]
    eps = [(b["eps_next"].float().to(DEV), b["eps_cur"].float().to(DEV)) for b in case["inputs"][1]]
    n, lrs = len(eps), case["lrs"] if schedule else None
    cuts = [0] + [u for u in range(1, n) if route != "many" or (lrs is not None and lrs[u] != lrs[u - 1])] + [n]
    res = []
    for a, b in zip(cuts, cuts[1:]):
        if lrs is not None:
            for opt, lr in zip(_optimizers(sac), lrs[a]):
                opt.param_groups[0]["lr"] = lr
        res += up.update_many([memory] * (b - a), B, case["first_update"] + a, reverse_mask=True, eps=eps[a:b])
    torch.cuda.synchronize()
    return sac, up, res


def _state(sac, n, key):
    return sac.optimizer_of(n).state[sac.params()[n]][key]


def _which(n):
    return "alpha" if n == "log_alpha" else ("policy" if n[0] == "p" else "critic")


def _check_one_update(case, sac, up, res, parameters_too):
    """One update against the restatements: taps, 5-tuple and both moments under tr.check, the parameters on Adam's formula over the
    kernels' own moments (and, ``parameters_too``, under tr.check), the step counts, the soft update, alpha."""
    name = case["name"]
    f32, f64, o32, o64 = case["f32"], case["f64"], case["out32"][0], case["out64"][0]
    f32r, o32r = case["f32r"], case["out32r"][0]  # the float32 restatement with the batch summed in the other order
    taps = up.forward_taps(case["shape"][3])
    for k in ("q1", "q2", "y", "log_pi_next", "log_pi"):
        tr.check(taps[k], o32[k], o64[k], f"{name}: {k}", [o32r[k]])
    for i, k in enumerate(("qf1_loss", "qf2_loss", "policy_loss", "alpha_loss", "alpha")):
        tr.check(torch.tensor(res[0][i], dtype=torch.float64), o32["losses"][i], o64["losses"][i], f"{name}: {k}", [o32r["losses"][i]])
    # the gradients, through the moments (from a new optimizer m = (1 - b1) g and v = (1 - b2) g^2)
    trained = sr.POLICY + sr.CRITIC + (("log_alpha",) if case["tuning"] else ())
    for n in trained:
        tr.check(_state(sac, n, "exp_avg"), f32["m"][n], f64["m"][n], f"{name}: m {n}", [f32r["m"][n]])
        tr.check(_state(sac, n, "exp_avg_sq"), f32["v"][n], f64["v"][n], f"{name}: v {n}", [f32r["v"][n]])
    # the parameters, pinned to Adam's formula on the kernels' OWN moments (tests/test_gpu_trainer.py:39-53), with the optimizer's own
    # lr, betas, eps and step: from zero moments a gradient that cancels to rounding moves a parameter anywhere in [-lr, lr],
    # whatever the summation order
    p0 = case["inputs"][0]
    adam = sr.adam_settings(case["adam"])
    before = case["start"]["steps"] if case["start"] is not None else dict(critic=0, policy=0, alpha=0)
    live = sac.params()
    for n in trained:
        own, step = adam[_which(n)], before[_which(n)] + 1
        bc1, bc2s = 1 - own["betas"][0] ** step, (1 - own["betas"][1] ** step) ** 0.5
        m, v = _state(sac, n, "exp_avg").double().cpu(), _state(sac, n, "exp_avg_sq").double().cpu()
        expect = p0[n].float().double() - (own["lr"] / bc1) * m / (v.sqrt() / bc2s + own["eps"])
        assert (live[n].detach().double().cpu() - expect).abs().max().item() <= 1e-7, f"{name}: {n}: Adam step off its own moments"
        assert float(_state(sac, n, "step")) == float(step)
        if parameters_too:  # from non-zero moments the step is smooth in the gradient
            tr.check(live[n].detach(), f32["p"][n], f64["p"][n], f"{name}: {n}", [f32r["p"][n]])
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


@pytest.mark.parametrize("name", sr.ONE_UPDATE + ["fixed_alpha", "clamp"])
def test_one_update_matches_restatement(engine, name):
    case = sr.build_case(name)
    sac, up, res = _run(engine, case)
    _check_one_update(case, sac, up, res, parameters_too=False)


def test_resumed_state_with_distinct_optimizers(engine):
    """Three optimizers that share no learning rate, beta, eps or step count, resumed from non-zero moments: the case is built so that
    exchanging any one of those between two optimizers moves a parameter or moment by more than twice the rule's allowance
    (sr.build_case asserts it; tests/test_sac_update_host.py lists the exchanges), so parity here pins the per-optimizer indexing."""
    case = sr.build_case("resumed")
    assert set(case["swaps"]) == set(sr.SWAPS) and all(ratio > 2.0 for _, ratio in case["swaps"].values())
    sac, up, res = _run(engine, case)
    _check_one_update(case, sac, up, res, parameters_too=True)
    steps = [float(_state(sac, n, "step")) for n in ("cw1", "pw1", "log_alpha")]
    assert steps == [8.0, 4.0, 12.0]


def test_resumed_three_updates_with_a_schedule(engine):
    case = sr.build_case("resumed_three")
    name = case["name"]
    sac, up, res = _run(engine, case, "many")
    f32, f64, f32r = case["f32"], case["f64"], case["f32r"]
    live = sac.params()
    for n in sr.POLICY + sr.CRITIC + sr.TARGET + ("log_alpha",):
        tr.check(live[n].detach(), f32["p"][n], f64["p"][n], f"{name}: {n} after 3 updates", [f32r["p"][n]])
    l32, l64, l32r = (torch.stack([o["losses"] for o in case[k]]) for k in ("out32", "out64", "out32r"))
    for i, k in enumerate(("qf1_loss", "qf2_loss", "policy_loss", "alpha_loss", "alpha")):
        tr.check(torch.tensor(res, dtype=torch.float64)[:, i], l32[:, i], l64[:, i], f"{name}: {k} of the 3 updates", [l32r[:, i]])
    for route in ("single", "many"):
        sac2, _, res2 = _run(engine, case, route)
        assert res2 == res, f"{name}: results of route {route}"
        for n, t in sac2.params().items():
            assert torch.equal(t.detach(), live[n].detach()), f"{name}: {n} differs on route {route}"
        for n in sr.MOMENTS:
            assert torch.equal(_state(sac2, n, "exp_avg"), _state(sac, n, "exp_avg")), f"{name}: m {n} differs on route {route}"
            assert torch.equal(_state(sac2, n, "exp_avg_sq"), _state(sac, n, "exp_avg_sq")), f"{name}: v {n} differs on route {route}"
            assert float(_state(sac2, n, "step")) == sr.RESUMED_STEPS[_which(n)] + 3.0
    # the updater read the learning rate a scheduler wrote between two calls: without the schedule the policy ends elsewhere, further
    # from the scheduled float64 restatement than the rule allows (a condition on the case, asserted first), and the GPU run agrees
    (flat64, _), (flat32, _) = (sr.restate(dict(case, lrs=None), dtype) for dtype in (torch.float64, torch.float32))
    n = max(sr.POLICY, key=lambda n: tr.dist(flat64["p"][n], f64["p"][n]))
    assert tr.dist(flat64["p"][n], f64["p"][n]) > 2 * sr.allowance(f32["p"][n], f64["p"][n], [f32r["p"][n]])
    sac3, _, _ = _run(engine, case, "single", schedule=False)
    tr.check(sac3.params()[n].detach(), flat32["p"][n], flat64["p"][n], f"{name}: {n} without the schedule")


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
    torch.manual_seed(HAND_OVER_SEEDS[0])
    res = [up.update_parameters(memory, B, u, log, reverse_mask=True) for u in range(K)]
    assert [r[0] for r in log.rows] == list(mbpo.LOG_KEYS) * K and [r[2] for r in log.rows] == [u for u in range(K) for _ in mbpo.LOG_KEYS]
    assert all(len(r) == 5 and all(isinstance(v, float) for v in r) for r in res)
    # a seeded run sees the reference's stream: the next-state table first, then the state table, drawn as Normal.rsample draws them
    torch.manual_seed(HAND_OVER_SEEDS[0])
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
    torch.manual_seed(HAND_OVER_SEEDS[1])
    out = sac.update_parameters(memory, B, K, None, reverse_mask=True)
    assert all(v == v for v in out) and float(sac.critic_optim.state[sac.critic.linear1.weight]["step"]) == K + 1
    # ... and the updater carries on from there (the stock update left a new alpha tensor behind)
    torch.manual_seed(HAND_OVER_SEEDS[2])
    more = up.update_parameters(memory, B, K + 1, None, reverse_mask=True)
    assert all(v == v for v in more) and float(sac.critic_optim.state[sac.critic.linear1.weight]["step"]) == K + 2
    # all K + 2 updates are the restatement's: the draws of the last two replayed like the first K, the one batch K + 2 times
    for seed in HAND_OVER_SEEDS[1:]:
        torch.manual_seed(seed)
        eps.append((torch.empty(B, act, device=DEV).normal_(), torch.empty(B, act, device=DEV).normal_()))
    p, batches, scale, bias = case["inputs"]
    chain = dict(case, inputs=(p, batches * (K + 2), scale, bias))
    host = [(a.cpu(), b.cpu()) for a, b in eps]
    (f64, o64), (f32, o32), (f32r, o32r) = (sr.restate(chain, dtype, eps=host, reverse_rows=rev) for dtype, rev in
                                            ((torch.float64, False), (torch.float32, False), (torch.float32, True)))
    sr.check_kinks(o32, o64, "hand-over")  # (the seeds were searched for it, like the cases')
    live = sac.params()
    for n in sr.POLICY + sr.CRITIC + sr.TARGET + ("log_alpha",):
        tr.check(live[n].detach(), f32["p"][n], f64["p"][n], f"hand-over: {n} after {K} + 2 updates", [f32r["p"][n]])
    for u, got in list(enumerate(res)) + [(K, out), (K + 1, more)]:
        for i, k in enumerate(("qf1_loss", "qf2_loss", "policy_loss", "alpha_loss", "alpha")):
            tr.check(torch.tensor(got[i], dtype=torch.float64), o32[u]["losses"][i], o64[u]["losses"][i], f"hand-over: {k} of update {u}", [o32r[u]["losses"][i]])


@pytest.mark.parametrize("name", ["s3_4_20_273", "resumed"])
def test_logger_values(engine, name):
    """What the result slot holds past the 5-tuple (the batch's mean reward, the entropy) and what update_many derives for the logger"""
    case = sr.build_case(name)
    sac, memory = sr.agent_for(case, DEV)
    B, b = case["shape"][3], case["inputs"][1][0]
    log = _Logger()
    res = hipets.SACUpdater(sac, engine=engine).update_many([memory], B, 0, log, reverse_mask=True, eps=[(b["eps_next"].float().to(DEV), b["eps_cur"].float().to(DEV))])
    rows = {r[0]: r[1] for r in log.rows}
    assert list(rows) == list(mbpo.LOG_KEYS)
    o32, o64, o32r = case["out32"][0], case["out64"][0], case["out32r"][0]
    as64 = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    tr.check(as64(rows["train/batch_reward"]), b["reward"].float().mean(), b["reward"].mean(), f"{name}: batch reward", [b["reward"].float().flip(0).mean()])
    tr.check(as64(rows["train_actor/entropy"]), -o32["log_pi"].mean(), -o64["log_pi"].mean(), f"{name}: entropy", [-o32r["log_pi"].flip(0).mean()])
    assert rows["train_critic/loss"] == float(torch.tensor(res[0][0], dtype=torch.float32) + torch.tensor(res[0][1], dtype=torch.float32))
    assert rows["train_actor/target_entropy"] == sac.target_entropy == case["target_entropy"]
    assert (rows["train_actor/loss"], rows["train_alpha/loss"], rows["train_alpha/value"]) == res[0][2:]


def test_misaligned_batch_takes_scalar_loads_of_the_same_operands(engine):
    """sac_ld4 loads 16 bytes where the row stride is a multiple of 4 floats and the base is 16-byte aligned (s27_8_64_257: W = 64, the
    state rows; K = 27 leaves a ragged tail), scalars otherwise -- the same operands to the same MFMAs.  The same update with the batch
    and both normal tables one float into a larger allocation must therefore come out bit for bit."""
    case = sr.build_case("s27_8_64_257")
    obs, act, hid, B = case["shape"]
    b = case["inputs"][1][0]

    def run(offset):
        def place(t):
            whole = torch.zeros(t.numel() + 8, dtype=torch.float32, device=DEV)
            view = whole[offset:offset + t.numel()].view(t.shape)
            view.copy_(t)
            assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
            return view

        sac, memory = sr.agent_for(case, DEV)
        up = hipets.SACUpdater(sac, engine=engine)
        steps = up._bind()
        up._sync_alpha()
        batch = place(torch.from_numpy(mbpo.pack_sac_batch(memory.sample(B).astuple(), True)))
        result = torch.empty(8, dtype=torch.float32, device=DEV)
        engine.sac_update(batch, place(b["eps_next"].float()), place(b["eps_cur"].float()), 0, [int(s[0]) for s in steps], [LR] * 3, result)
        taps = engine.sac_forward_taps(B)
        torch.cuda.synchronize()
        out = {"result": result.clone()}
        out.update({f"tap {k}": v.clone() for k, v in taps.items()})
        out.update({f"p {n}": t.detach().clone() for n, t in sac.params().items()})
        for n in sr.MOMENTS:
            out[f"m {n}"], out[f"v {n}"] = _state(sac, n, "exp_avg").clone(), _state(sac, n, "exp_avg_sq").clone()
        return out

    assert (2 * obs + act + 2) % 4 == 0 and obs % 4 != 0
    aligned, shifted = run(0), run(1)
    for k, v in aligned.items():
        assert torch.equal(v, shifted[k]), f"{k} differs between the aligned and the misaligned batch"
    # ... and it is the update of the case (the aligned run is test_one_update_matches_restatement's)
    o32, o64, o32r = case["out32"][0], case["out64"][0], case["out32r"][0]
    for i, k in enumerate(("qf1_loss", "qf2_loss", "policy_loss", "alpha_loss", "alpha")):
        tr.check(shifted["result"][i], o32["losses"][i], o64["losses"][i], f"misaligned: {k}", [o32r["losses"][i]])


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
