"""product="blocked" (sac_mm_blocked_kernel, HIPETS_SAC_PRODUCT_BLOCKED) on the MI355X: one update under the restatement rule of
tests/test_gpu_sac_update.py, and every float the update leaves behind equal to the tile route's on raw bytes -- the blocked kernel
issues the tile kernel's MFMAs per tile, in its order, on its operands, and ends in its epilogue, so nothing may differ."""
import pytest
import torch

import hipets
import sac_restatement as sr
import test_gpu_sac_update as base
from hipets import _lib, mbpo

pytestmark = pytest.mark.gpu
DEV = base.DEV


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _left_behind(sac, up, res, B):
    """every parameter and target tensor, log_alpha, both moments of every trained tensor, the five taps, the 5-tuples: name -> bits"""
    out = {f"p {n}": _bits(t) for n, t in sac.params().items()}
    for n in sr.MOMENTS:
        out[f"m {n}"], out[f"v {n}"] = _bits(base._state(sac, n, "exp_avg")), _bits(base._state(sac, n, "exp_avg_sq"))
    out.update({f"tap {k}": _bits(v) for k, v in up.forward_taps(B).items()})
    out["results"] = _bits(torch.tensor(res, dtype=torch.float32))
    return out


def _run(engine, case, product):
    """the case's updates in one update_many call with the case's own normal tables: (agent, updater, [5-tuples])"""
    sac, memory = sr.agent_for(case, DEV)
    up = hipets.SACUpdater(sac, engine=engine, product=product)
    B = case["shape"][3]
    eps = [(b["eps_next"].float().to(DEV), b["eps_cur"].float().to(DEV)) for b in case["inputs"][1]]
    res = up.update_many([memory] * len(eps), B, case["first_update"], reverse_mask=True, eps=eps)
    torch.cuda.synchronize()
    return sac, up, res


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


# every problem below one block with all edge masks | a block plus 8 columns, a chunk plus one row, two-segment first layers | hidden one
# block, B four row blocks plus one and eight chunks plus one, vector rows with a ragged K 27 | K 3 | the width limit, K 512 / 32 / 1024
@pytest.mark.parametrize("name", ["s5_2_15_15", "s23_6_72_33", "s27_8_64_257", "s3_4_20_273", "s512_32_1024_17"])
def test_one_update_matches_restatement_and_the_tile_route(engine, name):
    case = sr.build_case(name)
    sac, up, res = _run(engine, case, "blocked")
    base._check_one_update(case, sac, up, res, parameters_too=False)
    blocked = _left_behind(sac, up, res, case["shape"][3])
    sac, up, res = _run(engine, case, "tile")
    _same(blocked, _left_behind(sac, up, res, case["shape"][3]), f"{name}: blocked against tile")


def test_twenty_updates_bit_for_bit(engine):
    """the soft update every third update and Adam's step progression; the blocked route twice"""
    case = sr.build_case("twenty_i3")
    B = case["shape"][3]
    blocked, again, tile = (_left_behind(*_run(engine, case, product), B) for product in ("blocked", "blocked", "tile"))
    _same(blocked, tile, "twenty_i3: blocked against tile")
    _same(blocked, again, "twenty_i3: blocked against itself")


def test_misaligned_batch_is_staged_float_by_float_from_the_same_operands(engine):
    """tests/test_gpu_sac_update.py's misaligned set-up under "blocked": the batch and both normal tables one float into a larger
    allocation take the scalar staging path, which loads the same operands"""
    case = sr.build_case("s27_8_64_257")
    B, b = case["shape"][3], case["inputs"][1][0]

    def run(offset):
        def place(t):
            whole = torch.zeros(t.numel() + 8, dtype=torch.float32, device=DEV)
            view = whole[offset:offset + t.numel()].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == 4 * offset
            return view

        sac, memory = sr.agent_for(case, DEV)
        up = hipets.SACUpdater(sac, engine=engine, product="blocked")
        steps = up._bind()
        up._sync_alpha()
        batch = place(torch.from_numpy(mbpo.pack_sac_batch(memory.sample(B).astuple(), True)))
        result = torch.empty(8, dtype=torch.float32, device=DEV)
        engine.sac_update(batch, place(b["eps_next"].float()), place(b["eps_cur"].float()), 0, [int(s[0]) for s in steps], [base.LR] * 3, result,
                          product="blocked")
        torch.cuda.synchronize()
        return _left_behind(sac, up, [result.tolist()], B)

    _same(run(0), run(1), "the aligned against the misaligned batch")


def test_unknown_kind_is_refused(engine):
    """kind 2 fails with the invalid-argument class and leaves the setting: the next update is the default route's (the two routes agree
    on every bit, so what can be observed is that the engine still runs an update and gives those bits)"""
    case = sr.build_case("s5_2_15_15")
    before = _left_behind(*_run(engine, case, "tile"), case["shape"][3])
    with pytest.raises(hipets.HipetsError) as exc:
        engine._query("hipets_set_sac_product", kind=2)
    assert exc.value.kind == _lib.ERR_INVALID_ARGUMENT
    _same(before, _left_behind(*_run(engine, case, "tile"), case["shape"][3]), "after the refusal")
    with pytest.raises(ValueError):
        engine.sac_update(None, None, None, 0, (0, 0, 0), (0, 0, 0), None, product="rows")
