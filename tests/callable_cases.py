"""The oracle replays of hipets.CallableTrajectoryEvalFn (tests/test_gpu_callable_objective.py, section C): the cases, their models and
start states, and the replay of one call through the oracle from the draws of the call's (seed, stream).  The draws come from the
engine's exports on the GPU, or from their CPU restatements (oracle/feistel_perm.py, oracle/device_draws.py) in
tests/test_callable_objective_host.py, which checks without a GPU that the seeds chosen here keep the ORACLE ALONE inside the
replay's exclusion cap and the termination firing progressively."""
import numpy as np
import torch

from oracle import device_draws as dd
from oracle import feistel_perm as fp
from oracle import pets_oracle as po
from test_gpu_closed_forms import threshold_margin

ELITE = [0, 2, 3, 5, 6]  # 7 members / 5 elites (conf/dynamics_model/gaussian_mlp_ensemble.yaml)
SEED = 37  # the objectives' seed; call k of an objective runs stream k
MAX_EXCLUDED = 2  # candidates with a row within 1e-4 of a termination threshold: a cap, not a measurement
HOPPER = dict(ensemble_size=5, hid=40, termination="hopper")
REPLAYS = [  # name, obs, act, model kwargs, pop, P, H, mode
    ("hid200_device_random", 17, 6, dict(ensemble_size=7, elite=ELITE, hid=200), 100, 20, 5, "device"),
    ("hid200_device_fixed", 17, 6, dict(ensemble_size=7, elite=ELITE, hid=200, propagation="fixed_model"), 100, 20, 5, "device"),
    ("small_hopper_device", 11, 3, HOPPER, 24, 5, 6, "device"),
    ("small_hopper_basic_fast_fixed", 11, 3, dict(HOPPER, propagation="fixed_model", ensemble_kind="basic_ensemble"), 24, 5, 6, "fast"),
    ("small_hopper_exact", 11, 3, HOPPER, 24, 5, 6, "exact"),
]
REPLAY_IDS = [c[0] for c in REPLAYS]


def make_case(obs, act, mkw, model_seed=8):
    """(oracle model, s0): the hopper cases take smaller, less noisy steps from just above the height threshold, so that rows end at
    every step of the horizon"""
    om = po.make_synthetic_model(obs, act, seed=model_seed, **mkw)
    s0 = (np.random.default_rng(2).standard_normal(obs) * 0.05).astype(np.float32)
    if om.termination == "hopper":
        om.weights[-1] = om.weights[-1] * 0.2
        om.max_logvar = torch.full_like(om.max_logvar, -5.0)
        s0[0], s0[1] = 0.8, 0.0
    return om, s0


def callables(om):
    """the oracle's own closed forms as the Python callables of the objective"""
    return (po.REWARD_FNS[om.reward] if om.reward is not None else None), po.TERMINATION_FNS[om.termination]


def call_actions(act, pop, H, calls=2):
    g = torch.Generator().manual_seed(9)
    return [torch.rand(pop, H, act, generator=g) * 2 - 1 for _ in range(calls)]


def cpu_draws(om, pop, P, H, mode, stream, row_tiles=1):
    """oracle kwargs of the call with stream `stream`, from the CPU restatements of the in-kernel draws"""
    B, M = pop * P, len(om.active_members)
    fixed = om.propagation == "fixed_model"
    eps = torch.from_numpy(dd.fast_normals(H, B, om.out_size, SEED, stream))
    if mode == "device":
        steps = [0xFFFFFFFF] if fixed else range(H)
        perms = torch.stack([torch.from_numpy(fp.permutation(B, SEED, stream, t).astype(np.int64)) for t in steps])
        return dict(perms=perms[0] if fixed else perms, eps=eps)
    nwg = dd.fast_workgroups(B, row_tiles)
    sched = torch.from_numpy(dd.member_schedule(H, nwg, M, SEED, stream, fixed=fixed, iid=om.ensemble_kind == "basic_ensemble"))
    return dict(members=fast_member_map(sched, B, P, row_tiles), eps=eps)


def fast_member_map(sched, B, P, row_tiles):
    """[H, B] member slot of every row from a FAST member schedule [H, nwg]"""
    wg = torch.as_tensor(np.asarray(dd.fast_row_workgroup(torch.arange(B), P, row_tiles))).long()
    return torch.stack([sched[t].long()[wg] for t in range(sched.shape[0])])


def oracle_replay(om, actions, s0, P, draws):
    """(returns [pop], keep [pop], ended [H, B]) of po.rollout fed `draws`: `keep` = the candidates none of whose rows comes within
    1e-4 of a termination threshold (the return is discontinuous there), `ended` = the row has terminated by step t."""
    pop, H, _ = actions.shape
    trace = {}
    ref = po.rollout(om, actions, s0, P, trace=trace, **draws)
    ended = torch.stack(trace["dones"])[..., 0].cummax(0).values
    near = threshold_margin(om.termination, torch.stack(trace["next_obs"])) < 1e-4
    keep = ~near.any(0).view(pop, P).any(1)
    return ref, keep, ended, trace


def assert_replay_is_usable(om, keep, ended):
    """the cap on excluded candidates, and a termination that fires mid-horizon, not all at once"""
    H, B = ended.shape
    assert int((~keep).sum()) <= MAX_EXCLUDED
    if om.termination != "no_termination":
        assert 0 < int(ended[0].sum()) < int(ended[H // 2].sum()) < int(ended[-1].sum()) < B


EXACT_GENERATOR_SEED = 21


def exact_draws(spec, B, H, call, generator):
    """oracle kwargs of call `call` of the 'exact' case: the reference's own draws (hipets.reference_draws.rollout_draws) -- the
    permutations from torch's global generator, seeded per call here, the eps from `generator`, which runs on across the calls"""
    from hipets import reference_draws as rd

    torch.manual_seed(100 + call)
    perms, members, eps = rd.rollout_draws(spec, B, H, generator)
    return dict(perms=perms, eps=eps) if members is None else dict(members=members, eps=eps)
