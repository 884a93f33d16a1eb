"""hipets_policy_rollout, hipets.PolicyRollout / PolicyPrior and the optimizers' extra_candidates seam on the GPU.

The kernel is checked PER STEP ON THE DEVICE'S OWN STATES, two ways:
  bits    actions[:, t] equals SACActor.act_device(states[t]) and states[t + 1] equals policy_rollout_restatement.compose_np of
          EnsemblePredictor.predict(states[t], actions[:, t]): the fused kernel runs the layer functions of its two siblings, whose row
          bits depend neither on the row tiles nor on the batch (tests/test_gpu_policy.py, tests/test_gpu_ensemble.py assert that).
  parity  actions and next states within T1 x bound_factor of the float64 restatement of that step, bound_factor =
          ensemble_restatement.bound_factor of the float32 torch restatement against float64 on the same inputs (computed here).
Model cases: ensemble_restatement.GPU_CASES; actor widths below, at and above the model's hidden width (PAIRS)."""
import functools

import numpy as np
import pytest
import torch

import ensemble_restatement as er
import hipets
import policy_restatement as pr
import policy_rollout_restatement as rr
import sac_restatement as sr
from hipets import _pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_MAX = 160 * 1024
# (model case, actor hidden width): 15 / 16 against hid 20 (below), 16 against 16 and 200 against 200 (at), 72 against 32 and 1024
# against 200 (above: the actor's buffers decide the LDS need)
PAIRS = [("small_silu", 15), ("small_silu", 16), ("exact16", 16), ("columns_f32", 15), ("det_relu", 16), ("basic_tanh", 16), ("head9tiles", 72),
         ("stock", 200), ("humanoid_fit", 1024)]


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


@functools.lru_cache(maxsize=None)
def setup(name, hidden):
    """(model case, actor weights, eps [4, 80, A]) -- built once per pair and shared, never changed"""
    case = er.make_case(name)
    w, eps = rr.make_actor(f"{name}_actor{hidden}", case, hidden, rows=4 * 80)
    return case, w, eps.reshape(4, 80, case["act_dim"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def build(engine, name, hidden, only_elite=True, seed=0, **rule):
    case, w, eps = setup(name, hidden)
    spec = er.case_spec(case, **rule)
    return hipets.PolicyRollout(spec, BarePolicy(w), engine=engine, only_elite=only_elite, seed=seed), case, w, eps, spec


def check_steps(ro, case, w, spec, s0, H, eps, mean_rows, parity=True, what=""):
    """the two per-step checks of the module docstring; returns (actions, states)"""
    n = len(s0)
    e = dev(eps[:H, :n])
    actions, states = ro.sequences(dev(s0), horizon=H, mean_rows=mean_rows, eps=e, return_states=True)
    assert actions.shape == (n, H, case["act_dim"]) and states.shape == (H + 1, n, case["obs_dim"])
    assert torch.equal(bits(states[0]), bits(dev(s0)))
    for t in range(H):
        st = states[t].contiguous()
        want = ro.actor.act_device(st, sample=False)
        if mean_rows < n:
            want[mean_rows:] = ro.actor.act_device(st, sample=True, eps=e[t].contiguous())[mean_rows:]
        assert torch.equal(bits(actions[:, t]), bits(want)), f"{what} step {t}: actions differ from hipets_policy_act's"
        means = ro.predictor.predict(st, actions[:, t].contiguous(), only_elite=ro.only_elite)[0]
        composed = rr.compose_np(st.cpu().numpy(), means.cpu().numpy(), spec)
        assert np.array_equal(composed.view(np.int32), states[t + 1].cpu().numpy().view(np.int32)), f"{what} step {t}: next state differs from the composition"
        if parity:
            s_np, e_np = st.cpu().numpy(), eps[t, :n]
            a64, s64 = rr.step_f64(case, w, s_np, e_np, mean_rows, ro.only_elite, spec)
            a32, s32 = rr.step_f32(case, w, s_np, e_np, mean_rows, ro.only_elite, spec)
            fa, fs = er.bound_factor(a32, a64), er.bound_factor(s32, s64)
            sa, ss = er.t1_share(actions[:, t].cpu().numpy(), a64).max(), er.t1_share(states[t + 1].cpu().numpy(), s64).max()
            print(f"{what} step {t}: actions {sa:.3f} of T1 (bound {fa:.2f}), next states {ss:.3f} of T1 (bound {fs:.2f})")
            assert sa <= fa and ss <= fs, (what, t, float(sa), fa, float(ss), fs)
    return actions, states


@pytest.mark.parametrize("name,hidden", PAIRS, ids=[f"{n}_h{h}" for n, h in PAIRS])
def test_steps_match_the_shipped_kernels_and_the_float64_restatement(engine, name, hidden):
    ro, case, w, eps, spec = build(engine, name, hidden)
    R, lds = ro.geometry(10 ** 6)
    assert R in (1, 2, 4) and lds <= LDS_MAX
    assert lds == _pack.policy_rollout_lds_bytes(case["obs_dim"], case["act_dim"], hidden, case["in_dim"], case["hid"], case["out_dim"],
                                                 case["deterministic"], len(case["weights"]), R)
    if name == "stock":
        shapes = [(17, 3, 1)]
    elif name == "humanoid_fit":
        assert R == 1 and lds > LDS_MAX - 8 * 1024  # one row tile, at the LDS edge
        shapes = [(16, 2, 1)]
    elif (name, hidden) == ("small_silu", 15):
        shapes = [(1, 4, 0), (15, 2, 1), (16, 1, 16), (17, 4, 1), (16 * R - 1, 2, 0), (16 * R + 1, 2, 1)]
    else:
        shapes = [(1, 4, 0), (17, 2, 1)]
    for n, H, mean_rows in shapes:
        actions, _ = check_steps(ro, case, w, spec, case["obs"][:n], H, eps, mean_rows, what=f"{name} h{hidden} n={n} H={H} mean_rows={mean_rows}")
        if H == 1 or name in ("stock", "humanoid_fit"):  # states=None: the same actions
            alone = ro.sequences(dev(case["obs"][:n]), horizon=H, mean_rows=mean_rows, eps=dev(eps[:H, :n]))
            assert torch.equal(bits(alone), bits(actions))


@pytest.mark.parametrize("rule", [dict(target_is_delta=False), dict(no_delta_list=[0, 2])], ids=["absolute", "no_delta_first_and_last"])
def test_delta_rules(engine, rule):
    ro, case, w, eps, spec = build(engine, "small_silu", 16, **rule)
    assert rule.get("no_delta_list", [0, case["obs_dim"] - 1]) == [0, case["obs_dim"] - 1]
    _, states = check_steps(ro, case, w, spec, case["obs"][:17], 2, eps, 1, what=f"small_silu {rule}")
    ro2, _, _, _, spec2 = build(engine, "small_silu", 16)
    _, plain = check_steps(ro2, case, w, spec2, case["obs"][:17], 2, eps, 1, parity=False)
    assert not torch.equal(states[1], plain[1])  # (the rule is read)


def test_all_members_and_elites_differ(engine):
    ro, case, w, eps, spec = build(engine, "stock", 200, only_elite=False)
    _, all_states = check_steps(ro, case, w, spec, case["obs"][:5], 1, eps, 5, what="stock all members")
    ro2, _, _, _, _ = build(engine, "stock", 200, only_elite=True)
    elite_states = ro2.sequences(dev(case["obs"][:5]), horizon=1, mean_rows=5, return_states=True)[1]
    assert not torch.equal(all_states[1], elite_states[1])


def test_in_kernel_draws_equal_injected_draws(engine):
    ro, case, w, eps, spec = build(engine, "small_silu", 16, seed=11)
    n, H = 17, 4
    s0 = dev(case["obs"][:n])
    table = engine.policy_normals(H * n, case["act_dim"], 11, 5).reshape(H, n, case["act_dim"]).contiguous()
    drawn = ro.sequences(s0, horizon=H, mean_rows=1, stream_id=5, return_states=True)
    injected = ro.sequences(s0, horizon=H, mean_rows=1, eps=table, return_states=True)
    for a, b in zip(drawn, injected):
        assert torch.equal(bits(a), bits(b))
    other = ro.sequences(s0, horizon=H, mean_rows=1, stream_id=6)
    assert not torch.equal(other[1:], drawn[0][1:]) and torch.equal(bits(other[0]), bits(drawn[0][0]))  # (row 0 is the mean policy)


def test_rows_do_not_depend_on_the_batch_and_a_nan_row_stays_alone(engine):
    ro, case, w, eps, spec = build(engine, "small_silu", 16)
    R = ro.geometry(10 ** 6)[0]
    H, big = 4, 16 * R + 1
    assert [ro.geometry(n)[0] for n in (1, 17, big)] == [1, 2, R]
    s0 = case["obs"][:big]
    e = np.ascontiguousarray(eps[:, :big])
    full = ro.sequences(dev(s0), horizon=H, mean_rows=0, eps=dev(e), return_states=True)
    for n in (1, 17):
        part = ro.sequences(dev(s0[:n]), horizon=H, mean_rows=0, eps=dev(e[:, :n]), return_states=True)
        assert torch.equal(bits(part[0]), bits(full[0][:n])) and torch.equal(bits(part[1]), bits(full[1][:, :n]))
    bad = s0.copy()
    bad[3, 1] = np.nan
    got = ro.sequences(dev(bad), horizon=H, mean_rows=0, eps=dev(e), return_states=True)
    keep = [i for i in range(big) if i != 3]
    assert torch.isnan(got[1][1:, 3]).all()  # (the row stays NaN; its actions need not: the actor's relu is a select)
    assert torch.equal(bits(got[0][keep]), bits(full[0][keep])) and torch.equal(bits(got[1][:, keep]), bits(full[1][:, keep]))


def _too_wide_spec():
    """the narrowest model over act_dim 8 whose rollout with a 1024-wide actor needs more than LDS_MAX at one row tile, while the
    ensemble kernel itself still takes it"""
    act, hid, layers = 8, 16, 2
    obs = next(o for o in range(16, 505) if _pack.policy_rollout_lds_bytes(o, act, 1024, o + act, hid, o, True, layers) > LDS_MAX)
    assert _pack.policy_rollout_lds_bytes(obs - 1, act, 1024, obs - 1 + act, hid, obs - 1, True, layers) <= LDS_MAX
    assert obs + act <= 512 and _pack.ensemble_lds_bytes(obs + act, hid, obs, True, layers) <= LDS_MAX
    g = torch.Generator().manual_seed(0)
    ws = [torch.randn(1, obs + act, hid, generator=g) * 0.05, torch.randn(1, hid, obs, generator=g) * 0.05]
    bs = [torch.zeros(1, 1, hid), torch.zeros(1, 1, obs)]
    spec = hipets.ModelSpec(weights=ws, biases=bs, obs_dim=obs, act_dim=act, min_logvar=None, max_logvar=None, deterministic=True, reward="none")
    return spec, obs, act, _pack.policy_rollout_lds_bytes(obs, act, 1024, obs + act, hid, obs, True, layers)


def test_refusals(engine):
    case, w, eps = setup("small_silu", 16)
    fresh = hipets.Engine(DEV)  # an engine of its own: empty slots
    s0 = dev(case["obs"][:4])
    out = torch.empty(4, 2, case["act_dim"], device=DEV)
    call = lambda eng, **kw: eng._call("hipets_policy_rollout", **{**dict(s0=s0, n=4, horizon=2, mean_rows=1, only_elite=1, seed=0, stream_id=0,  # noqa: E731
                                                                          eps=None, actions=out, states=None), **kw})

    def refused(eng, word, **kw):
        with pytest.raises(hipets.HipetsError, match=word) as exc:
            call(eng, **kw)
        assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT

    refused(fresh, "no policy")
    fresh.policy_set(BarePolicy(w))
    refused(fresh, "no ensemble")
    with pytest.raises(hipets.HipetsError, match="no ensemble"):
        fresh.policy_rollout_geometry(4)
    fresh.ensemble_set(er.case_spec(case))
    call(fresh)
    for kw, word in ((dict(n=0), "bad n"), (dict(horizon=0), "bad horizon"), (dict(mean_rows=-1), "mean_rows"), (dict(mean_rows=5), "mean_rows")):
        refused(fresh, word, **kw)
    other, w2, _ = setup("exact16", 16)  # another (obs, act)
    fresh.policy_set(BarePolicy(w2))
    refused(fresh, "differs")
    # a BasicEnsemble has no elite subset: only_elite averages all of its members
    basic = build(fresh, "basic_tanh", 16)
    b_case = basic[1]
    a1 = fresh.policy_rollout(dev(b_case["obs"][:4]), 2, mean_rows=4, only_elite=True)
    a0 = fresh.policy_rollout(dev(b_case["obs"][:4]), 2, mean_rows=4, only_elite=False)
    assert torch.equal(bits(a1), bits(a0))
    # too wide for LDS: the message names the bytes
    spec, obs, act, need = _too_wide_spec()
    wide, _, _ = pr.make_case("too_wide_actor", obs, 1024, act, rows=1)
    fresh.policy_set(BarePolicy(wide))
    fresh.ensemble_set(spec)
    big = torch.zeros(1, obs, device=DEV)
    with pytest.raises(hipets.HipetsError, match=f"too wide for LDS.*{need} bytes") as exc:
        fresh._call("hipets_policy_rollout", s0=big, n=1, horizon=1, mean_rows=0, only_elite=1, seed=0, stream_id=0, eps=None,
                    actions=torch.empty(1, 1, act, device=DEV), states=None)
    assert exc.value.kind == hipets.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="differs"):  # the Python front end, before any launch
        hipets.PolicyRollout(er.case_spec(case), BarePolicy(w2), engine=fresh)
    fresh.close()


# ---- the optimizers' seam -----------------------------------------------------------------------------------------------------------
H_, A_, POP, NUM = 3, 2, 32, 5
LOWER, UPPER = [[-1.0] * A_] * H_, [[1.0] * A_] * H_


def _optimizer(kind):
    if kind == "cem":
        return hipets.CEMOptimizer(2, 0.25, POP, LOWER, UPPER, 0.1, DEV, seed=7)
    if kind == "mppi":
        return hipets.MPPIOptimizer(2, POP, 0.9, 0.5, 0.6, LOWER, UPPER, DEV, seed=7)
    return hipets.ICEMOptimizer(2, 0.25, POP, 1.25, 2.0, LOWER, UPPER, 0.5, 0.1, DEV, seed=7)


def _objective(pop):
    return -(pop ** 2).sum(dim=(1, 2))


def _first_population(opt, **kw):
    seen = []
    torch.manual_seed(0)  # (iCEM's kept-elite permutation is torch's)
    opt.optimize(_objective, x0=torch.zeros(H_, A_), callback=lambda p, v, i: seen.append(p.clone()) if i == 0 else None, **kw)
    return seen[0]


@pytest.mark.parametrize("kind", ["cem", "mppi", "icem"])
def test_extra_candidates_enter_the_sampled_rows(engine, kind):
    g = torch.Generator().manual_seed(1)
    extra = (torch.rand(NUM, H_, A_, generator=g) * 3 - 1.5).to(DEV)  # (some outside the bounds)
    extra[2, 1, 0] = float("nan")
    extra[4, 0, 1] = float("inf")
    plain_opt, seam_opt = _optimizer(kind), _optimizer(kind)
    rounds = 2 if kind == "icem" else 1  # (iCEM: the second plan starts with elites, whose shifted rows follow the sampled part)
    for _ in range(rounds):
        plain = _first_population(plain_opt)
        seam = _first_population(seam_opt, extra_candidates=extra)
        fine = [0, 1, 3]
        assert torch.equal(bits(seam[fine]), bits(extra[fine].clamp(-1.0, 1.0)))
        assert torch.equal(bits(seam[[2, 4]]), bits(plain[[2, 4]]))  # a non-finite candidate row keeps its sampled bits
        assert torch.equal(bits(seam[NUM:]), bits(plain[NUM:]))
        if kind == "icem":
            seam_opt.elite = plain_opt.elite.clone()  # (the two plans' elites differ after a plan with candidates: start the next alike)
    if kind == "icem":
        assert plain.shape[0] > POP  # (the kept rows were there, and untouched)


def test_extra_candidates_refusals(engine):
    opt = _optimizer("cem")
    x0 = torch.zeros(H_, A_)
    for bad, word in ((torch.zeros(POP + 1, H_, A_), "smallest iteration"), (torch.zeros(NUM, H_, A_, dtype=torch.float64), "float32"),
                      (torch.zeros(NUM, H_ + 1, A_), "float32 tensor"), (np.zeros((NUM, H_, A_), np.float32), "float32 tensor")):
        calls = opt.calls
        with pytest.raises(ValueError, match=word):
            opt.optimize(_objective, x0=x0, extra_candidates=bad)
        assert opt.calls == calls  # (refused before anything ran: the plan counter, hence the streams, did not move)
    icem = _optimizer("icem")
    smallest = min(icem._iteration_size(i) for i in range(2))
    with pytest.raises(ValueError, match=f"samples {smallest}"):
        icem.optimize(_objective, x0=x0, extra_candidates=torch.zeros(smallest + 1, H_, A_))


def test_the_best_candidate_wins(engine):
    g = torch.Generator().manual_seed(3)
    star = (torch.rand(H_, A_, generator=g) * 1.8 - 0.9).to(DEV)
    best = _optimizer("cem").optimize(lambda pop: -((pop - star) ** 2).sum(dim=(1, 2)), x0=torch.zeros(H_, A_), extra_candidates=star[None].clone())
    assert torch.equal(bits(best), bits(star))


# ---- the agent seam -----------------------------------------------------------------------------------------------------------------
def _agent(seed=5):
    cfg = {"_target_": "hipets.CEMOptimizer", "num_iterations": 2, "elite_ratio": 0.25, "population_size": POP, "alpha": 0.1, "device": DEV,
           "seed": seed}
    return hipets.TrajectoryOptimizerAgent(cfg, [-1.0] * A_, [1.0] * A_, planning_horizon=H_)


def test_policy_prior_through_the_agent(engine, monkeypatch):
    case, w, _ = setup("small_silu", 16)
    spec = er.case_spec(case)
    policy = BarePolicy(w)
    obs = case["obs"][0]
    fused_calls = []
    import hipets.optimizers as ho

    real = ho._run_fused_plan
    monkeypatch.setattr(ho, "_run_fused_plan", lambda *a, **k: (fused_calls.append(1), real(*a, **k))[1])
    plain, seamed = _agent(), _agent()
    for a in (plain, seamed):
        a.set_trajectory_eval_fn(hipets.make_eval_fn(spec, 3, engine=engine))
    prior = hipets.PolicyPrior(spec, policy, num=NUM, mean_rows=1, seed=9, engine=engine)
    # no change without a prior: set and taken away again, the plan is the fused one-call plan with the bits of an agent that never had one
    seamed.set_policy_prior(prior)
    seamed.set_policy_prior(None)
    p0, p1 = plain.plan(obs), seamed.plan(obs)
    assert len(fused_calls) == 2 and np.array_equal(p0.view(np.int32), p1.view(np.int32)) and prior.plans == 0
    # with the prior: the per-iteration loop, its sequences computed once, in rows [0, NUM) of iteration 0
    seamed.set_policy_prior(prior)
    seen = []
    seamed.actions_to_use = []
    seamed.act(obs, optimizer_callback=lambda p, v, i: seen.append(p.clone()))
    assert len(fused_calls) == 2 and prior.plans == 1 and len(seen) == 2
    twin = hipets.PolicyPrior(spec, policy, num=NUM, mean_rows=1, seed=9, engine=engine)
    want = twin.sequences(obs, horizon=H_)
    assert want.shape == (NUM, H_, A_)
    for pop in seen:
        assert torch.equal(bits(pop[:NUM]), bits(want.clamp(-1.0, 1.0)))
    # a stock-shaped optimizer, whose **kwargs would swallow the rows, says so

    class Stock(hipets.Optimizer):
        device = torch.device(DEV)

        def optimize(self, obj_fun, x0=None, callback=None, **kwargs):
            return x0

    seamed.optimizer.optimizer = Stock()
    with pytest.raises(TypeError, match="extra_candidates"):
        seamed.plan(obs)
    with pytest.raises(TypeError, match="sequences"):
        plain.set_policy_prior(object())


def test_sequences_follow_a_sac_update(engine):
    """after one SACUpdater update the prior's sequences change and equal a freshly built prior's"""
    case, _, _ = setup("small_silu", 16)
    spec = er.case_spec(case)
    obs_dim, act_dim, B = case["obs_dim"], case["act_dim"], 8
    torch.manual_seed(4)
    sac = sr.TinySAC(obs_dim, act_dim, 16, device=DEV)
    g = torch.Generator().manual_seed(5)
    batch = dict(state=torch.randn(B, obs_dim, generator=g), action=torch.rand(B, act_dim, generator=g) * 2 - 1,
                 next_state=torch.randn(B, obs_dim, generator=g), reward=torch.randn(B, 1, generator=g), terminated=torch.zeros(B, 1))
    prior = hipets.PolicyPrior(spec, sac, num=NUM, seed=2, engine=engine)
    ask = lambda p: p.rollout.sequences(case["obs"][1], n=NUM, horizon=H_, mean_rows=1, stream_id=3)  # noqa: E731
    before = ask(prior).clone()
    assert torch.equal(bits(before), bits(ask(prior)))
    hipets.SACUpdater(sac, engine=engine).update_parameters(sr.FixedMemory([batch]), B, 1)
    after = ask(prior)
    assert not torch.equal(after, before)
    assert torch.equal(bits(after), bits(ask(hipets.PolicyPrior(spec, sac, num=NUM, seed=2, engine=engine))))
