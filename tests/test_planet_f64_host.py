"""What tests/test_gpu_planet_parity.py rests on, checked on the reference alone (CPU): the f32 oracle stays well inside the per-step
tolerance T1 of its own f64 evaluation for every free-running case, the saturated case saturates, the chosen shapes reach every tail
length of every op and every argument of the segment layout's maxima, and the restated layout (row stride, tile counts, LDS bytes) puts
the near-conf models on the STATIC instance and the widest admissible row at (30, 6, 296, 296)."""
import pytest
import torch

import planet_f64 as pf


def _free_running():
    return ([(d, 8) for d in pf.EDGE_SHAPES] + [(d, 4) for d in pf.STATIC_SHAPES + pf.NEAR_SHAPES] + [(pf.widest_square_models()[0], 2)])


@pytest.mark.parametrize("dims,H", _free_running(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"H{v}")
@pytest.mark.parametrize("sample", [True, False], ids=["eps", "mean"])
def test_f32_oracle_is_within_a_fifth_of_t1_of_f64(dims, H, sample):
    """Per-step latent / belief / reward and the returns of the f32 oracle against the f64 evaluation of the same rollout: a GPU kernel
    held to T1 of the f64 reference is held to at most 1.2 x T1 of the f32 oracle and the other way round."""
    pm, actions, latent0, belief0, eps = pf.free_case(dims, H)
    if not sample:
        eps = torch.zeros_like(eps)
    r32 = pf.rollout_traced(pm, actions, latent0, belief0, 2, eps)
    r64 = pf.rollout_traced(pf.to_f64(pm), actions, latent0, belief0, 2, eps)
    assert r64[0].dtype == torch.float64 and r32[0].dtype == torch.float32
    for name, a, b in zip(("returns", "latent", "belief", "rewards"), r32, r64):
        assert torch.isfinite(b).all(), name
        x = pf.t1_excess(a, b, frac=0.2)
        print(f"{dims} H {H} {name}: max |f32 - f64| = {(a.double() - b).abs().max():.2e}, {x:.2f} of T1 / 5")
        assert x <= 1.0, (name, x)


@pytest.mark.parametrize("dims", pf.SATURATED_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_saturated_case_saturates(dims):
    pm, actions, latent0, belief0, eps = pf.saturated_case(dims)
    latent, belief, reward, raw_std = pf.step_traced(pf.to_f64(pm), actions, latent0, belief0, eps)
    assert all(torch.isfinite(t).all() for t in (latent, belief, reward, raw_std))
    frac = (belief.abs() > 0.99).double().mean().item()
    print(f"{dims}: {100 * frac:.0f} % of next-belief entries beyond 0.99; raw std in [{raw_std.min():.1f}, {raw_std.max():.1f}]")
    assert frac >= 0.30
    assert raw_std.max() > 20 and raw_std.min() < -15  # softplus' x > 20 branch, and log(1 + exp(x)) flushing to 0 in f32


def test_edge_shapes_reach_every_tail_length_of_every_op():
    for i in range(pf.N_OPS):
        seen = {pf.tail_steps(pf.op_dims(d)[i][0]) for d in pf.EDGE_SHAPES}
        assert seen == {1, 2, 3, 4}, (i, seen)


def test_edge_shapes_decide_every_maximum_of_the_layout_by_each_argument():
    def decided(pick):
        return {pick(*d) for d in pf.EDGE_SHAPES}

    assert {"belief", "hidden"} <= decided(lambda L, A, Hb, F: "belief" if Hb > F else "hidden" if F > Hb else "tie")
    assert {"3belief", "hidden"} <= decided(lambda L, A, Hb, F: "3belief" if 3 * Hb > F else "hidden" if F > 3 * Hb else "tie")
    assert {"3belief", "2latent", "floor"} <= decided(
        lambda L, A, Hb, F: "floor" if max(3 * Hb, 2 * L) < 16 else "3belief" if 3 * Hb > 2 * L else "2latent" if 2 * L > 3 * Hb else "tie")


def test_restated_layout_picks_the_static_family_and_the_lds_limit():
    assert pf.row_floats(pf.CONF) == 1736 and pf.runs_static(pf.CONF)
    assert pf.tile_counts(pf.CONF) == [(13, 3), (38, 13), (38, 13), (13, 13), (4, 13), (13, 15), (13, 13), (1, 13)]
    for d in pf.STATIC_SHAPES:
        assert pf.runs_static(d) and d != pf.CONF, d
    for d in pf.NEAR_SHAPES:  # the same row stride, one op one tile off
        assert pf.row_floats(d) == 1736 and not pf.runs_static(d), d
        assert sum(a != b for a, b in zip(pf.tile_counts(d), pf.tile_counts(pf.CONF))) >= 1
    fits, refused = pf.widest_square_models()
    assert fits == (30, 6, 296, 296) and pf.row_floats(fits) == 2504
    assert refused == (30, 6, 304, 304) and pf.row_floats(refused) == 2568
    assert pf.smem_bytes(2504) <= pf.LDS_BYTES < pf.smem_bytes(2568)
