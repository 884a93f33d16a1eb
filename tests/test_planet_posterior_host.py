"""What tests/test_gpu_planet_posterior.py rests on, checked on the CPU: for every shape it uses, the float32 evaluation of the
restatement lies within a fifth of T1 of the float64 one (the rule of test_planet_f64_host.py), so T1 against float64 is a fair bound
for an fp32 kernel; and the refusals that need no GPU."""
import dataclasses

import pytest
import torch

import planet_posterior_f64 as pp


@pytest.mark.parametrize("n_env", [1, 17])
@pytest.mark.parametrize("case", pp.ENCODER_CASES, ids=pp.case_id)
def test_f32_encoder_is_within_a_fifth_of_t1_of_f64(case, n_env):
    model, obs, _, _ = pp.make_case(case, n_env)
    x = pp.t1_excess(pp.encode(model, obs[0], torch.float32), pp.encode(model, obs[0]), frac=0.2)
    print(f"{pp.case_id(case)} n_env {n_env}: {x:.2f} of T1 / 5")
    assert x <= 1.0


@pytest.mark.parametrize("sample", [True, False], ids=["eps", "mean"])
@pytest.mark.parametrize("case", pp.STEP_CASES, ids=pp.case_id)
def test_f32_posterior_step_is_within_a_fifth_of_t1_of_f64(case, sample):
    ref = pp.episode(case, 17, sample)
    got = pp.episode(case, 17, sample, torch.float32, states=ref)
    for t, (a, b) in enumerate(zip(got, ref)):
        for name, u, v in zip(("latent", "belief"), a, b):
            x = pp.t1_excess(u, v, frac=0.2)
            print(f"{pp.case_id(case)} step {t} {name}: {x:.2f} of T1 / 5")
            assert x <= 1.0, (t, name)


def _spec(case=pp.STEP_CASES[0]):
    import hipets

    return hipets.spec_from_planet_posterior(pp.make_case(case, 1)[0])


def test_spec_reads_the_stand_in():
    spec = _spec(pp.ENCODER_CASES[5])
    assert spec.layer_shapes == [(17, 13, 12), (8, 5, 4), (16, 4, 3), (5, 2, 1)] and spec.w_fc is None and spec.encoding_size == 10
    assert (spec.latent_size, spec.action_size, spec.belief_size, spec.hidden_size) == pp.SMALL_HEAD


@pytest.mark.parametrize("edit", ["padding", "dilation", "groups", "activation", "head_activation"])
def test_unsupported_modules_are_refused(edit):
    import copy

    import hipets

    model = copy.deepcopy(pp.make_case(pp.STEP_CASES[2], 1)[0])
    conv = model.encoder.convs[0][0]
    if edit == "padding":
        conv.padding = (1, 1)
    elif edit == "dilation":
        conv.dilation = (2, 2)
    elif edit == "groups":
        conv.groups = 3
    elif edit == "activation":
        model.encoder.convs[0][1] = torch.nn.ELU()
    else:
        model.posterior_transition_model[1] = torch.nn.Tanh()
    with pytest.raises(hipets.UnsupportedModelError, match="keep the stock route"):
        hipets.spec_from_planet_posterior(model)


@pytest.mark.parametrize("field,value,what", [
    ("image_shape", (3, 129, 8), "image height"), ("strides", [5], "stride"), ("conv_weights", [torch.zeros(8, 3, 9, 9)], "kernel"),
    ("conv_weights", [torch.zeros(8, 3, 3, 4)], "non-square"), ("image_shape", (513, 8, 8), "image channels")])
def test_over_limit_shapes_are_refused(field, value, what):
    import hipets

    spec = dataclasses.replace(_spec(), **{field: value})
    with pytest.raises(hipets.UnsupportedModelError, match=what):
        spec.validate()


def test_head_too_wide_for_lds_is_refused():
    import hipets

    Hb, enc, L, A, F = 400, 72, 1, 1, 1
    z = torch.zeros
    spec = dataclasses.replace(_spec(), w_embed=z(Hb, L + A), b_embed=z(Hb), w_ih=z(3 * Hb, Hb), b_ih=z(3 * Hb), w_hh=z(3 * Hb, Hb), b_hh=z(3 * Hb),
                               w_post1=z(F, Hb + enc), b_post1=z(F), w_post2=z(2 * L, F), b_post2=z(2 * L))
    with pytest.raises(hipets.UnsupportedModelError, match="LDS"):
        spec.validate()
