"""hipets.PlaNetPosterior on the GPU against the float64 restatement (tests/planet_posterior_f64.py) under the per-step tolerance T1:
the conv encoder at its shape edges, the posterior step, batch independence bit for bit, and the seams to the rest of the library."""
import copy

import numpy as np
import pytest
import torch

import hipets
import planet_posterior_f64 as pp

pytestmark = pytest.mark.gpu


def inside_t1(got, ref, what):
    x = pp.t1_excess(got.cpu(), ref)
    print(f"{what}: {x:.3f} of T1")
    assert x <= 1.0, (what, x)


# every edge shape at n_env 1, 2 and 17 (images share and straddle row tiles), conf shape at 1 and 4
ENCODE = [(case, n) for case in pp.ENCODER_CASES[:-1] for n in (1, 2, 17)] + [(pp.ENCODER_CASES[-1], n) for n in (1, 4)]


@pytest.mark.parametrize("case,n_env", ENCODE, ids=lambda v: pp.case_id(v) if isinstance(v, tuple) else f"n{v}")
def test_encoder_against_f64(engine, case, n_env):
    model, obs, _, _ = pp.make_case(case, n_env)
    got = hipets.PlaNetPosterior(model, n_env=n_env, engine=engine).encode(obs[0])
    inside_t1(got, pp.encode(model, obs[0]), f"{pp.case_id(case)} n_env {n_env} encoding")


@pytest.mark.parametrize("sample", [True, False], ids=["eps", "mean"])
@pytest.mark.parametrize("n_env", [1, 17])
@pytest.mark.parametrize("case", pp.STEP_CASES, ids=pp.case_id)
def test_posterior_steps_against_f64(engine, case, n_env, sample):
    """reset -> update(action=None) -> two update(action); every step's reference starts from the GPU's own previous output"""
    model, obs, actions, eps = pp.make_case(case, n_env)
    post = hipets.PlaNetPosterior(copy.deepcopy(model), n_env=n_env, engine=engine)
    post.reset()
    got = []
    for t in range(3):
        out = post.update(obs[t], action=None if t == 0 else actions[t - 1], eps=eps[t], sample=sample)
        got.append((out["latent"].cpu(), out["belief"].cpu()))
    ref = pp.episode(case, n_env, sample, states=got)
    for t in range(3):
        for name, a, b in zip(("latent", "belief"), got[t], ref[t]):
            inside_t1(a, b, f"{pp.case_id(case)} n_env {n_env} step {t} {name}")


@pytest.mark.parametrize("case", [pp.ENCODER_CASES[2], pp.ENCODER_CASES[5], pp.STEP_CASES[1]], ids=pp.case_id)
def test_batch_independence_bit_for_bit(engine, case):
    """image i of an n_env = 17 batch == the same image alone; uint8 == the same pixels as float32; a repeated call == the first"""
    model, obs, actions, eps = pp.make_case(case, 17)
    many, one = (hipets.PlaNetPosterior(model, n_env=n, engine=engine) for n in (17, 1))
    enc = many.encode(obs[0])
    assert torch.equal(enc, many.encode(obs[0])) and torch.equal(enc, many.encode(obs[0].float().numpy()))
    many.reset()
    first = many.update(obs[0], eps=eps[0])
    second = many.update(obs[1].to("cuda:0"), action=actions[0], eps=eps[1])
    for i in (0, 5, 16):
        assert torch.equal(one.encode(obs[0, i]), enc[i:i + 1])
        one.reset()
        assert torch.equal(one.update(obs[0, i], eps=eps[0, i:i + 1])["latent"], first["latent"][i:i + 1])
        out = one.update(obs[1, i].float(), action=actions[0, i], eps=eps[1, i:i + 1])
        assert torch.equal(out["latent"], second["latent"][i:i + 1]) and torch.equal(out["belief"], second["belief"][i:i + 1])


def test_live_model_seam_and_generator(engine):
    """n_env == 1 on a live model: the results land where the reference keeps them, PlaNetTrajectoryEvalFn.prepare() picks them up, the
    generator advances by exactly one randn([1, L]), and a parameter edited in place is re-packed before the next call"""
    case = pp.STEP_CASES[2]
    model = copy.deepcopy(pp.make_case(case, 1)[0])
    _, obs, actions, _ = pp.make_case(case, 1)
    post = hipets.PlaNetPosterior(model, engine=engine)
    with pytest.raises(ValueError, match="straight after reset"):
        post.update(obs[0])
    post.reset()
    rng, twin = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    out = post.update(obs[0], rng=rng)
    eps0 = torch.randn([1, case[3][0]], generator=twin)
    assert torch.equal(rng.get_state(), twin.get_state())
    assert model._current_posterior_sample is out["latent"] and model._current_belief is out["belief"]
    ref = pp.step(model, obs[0], torch.zeros(1, case[3][1]), torch.zeros(1, case[3][0]), torch.zeros(1, case[3][2]), eps0)
    inside_t1(out["latent"], ref[0], "seeded latent")
    with pytest.raises(ValueError, match="straight after reset"):
        post.update(obs[1])
    fn = hipets.PlaNetTrajectoryEvalFn(model, 1, engine=engine)
    latent0, belief0 = fn.prepare()
    assert torch.equal(latent0, out["latent"].reshape(-1)) and torch.equal(belief0, out["belief"].reshape(-1))
    with torch.no_grad():
        model.encoder.convs[0][0].weight.mul_(0.5)
    out2 = post.update(obs[1], action=actions[0, 0], sample=False)
    ref2 = pp.step(model, obs[1], actions[0], out["latent"].cpu(), out["belief"].cpu(), None)
    inside_t1(out2["latent"], ref2[0], "latent after an in-place edit")
    post.reset()
    assert model._current_posterior_sample is None and model._current_belief is None


def test_partial_reset_and_batched_agent(engine):
    """reset(env_ids=[k]) zeroes only environment k's next step; the batched results are BatchedCEMAgent.plan's start states"""
    case, n_env, k = (pp.CONF_IMAGE, pp.CONF_CONVS, None, pp.CONF), 4, 2
    model, obs, actions, eps = pp.make_case(case, n_env)
    post = hipets.PlaNetPosterior(model, n_env=n_env, engine=engine)
    post.reset()
    s0 = post.update(obs[0], eps=eps[0])
    post.reset(env_ids=[k])
    s1 = post.update(obs[1], action=actions[0], eps=eps[1])
    latent, belief, action = s0["latent"].cpu().clone(), s0["belief"].cpu().clone(), actions[0].clone()
    latent[k], belief[k], action[k] = 0, 0, 0
    ref = pp.step(model, obs[1], action, latent, belief, eps[1])
    inside_t1(s1["latent"], ref[0], "latent after a partial reset")
    inside_t1(s1["belief"], ref[1], "belief after a partial reset")
    with pytest.raises(ValueError, match="obs has shape"):
        post.update(obs[2, :3], action=actions[1], eps=eps[2])  # a wrong n_env
    A, H = pp.CONF[1], 4
    fn = hipets.PlaNetTrajectoryEvalFn(hipets.spec_from_planet_model(model), 1, engine=engine, seed=2)
    agent = hipets.BatchedCEMAgent(fn, n_env, [-1.0] * A, [1.0] * A, H, 2, 0.1, 100, 0.0, return_mean_elites=True, clipped_normal=True, seed=7)
    plans = agent.plan(np.zeros((n_env,) + pp.CONF_IMAGE, np.float32), latent=s1["latent"], belief=s1["belief"])
    assert plans.shape == (n_env, H, A) and np.isfinite(plans).all()
