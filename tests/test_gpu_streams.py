"""The stream contract of include/hipets.h on the MI355X: an engine's calls execute in call order whatever stream each is made on.

Every chain of tests/stream_cases.py runs on two streams, step k on stream k % 2, step k + 1 reading device memory step k writes, with
no torch-level wait between the calls and a gate (tests/stream_gate.py) parked at the head of the first call's stream: a call that
did not wait for its predecessor would run while the gate is still closed and read the poison every intermediate buffer and engine
slot was filled with.  The bits of every output are compared with the same calls made one by one on the default stream.  Only float
and byte data flow between calls: every index, count, cursor or offset a call reads from device memory is written before the gate,
so a missing wait gives wrong numbers, never an access out of range.  Rollouts run FAST and DEVICE mode with persistent launches
off, on an engine of this module's own.

Further cases: snapshot slots under a gate, calls that take no part (launch-only helpers, refused calls) between a gated producer and
its consumer, the pinned staging ring and workspace growth across streams, and the public wrappers on a side stream."""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import callable_cases as cc
import hipets
import stream_cases as sc
import stream_gate as sg
import train_restatement as tr
from conftest import to_spec
from hipets import _lib
from hipets._pack import pack_train_desc, row_width
from oracle import planet_oracle as pl
from sac_restatement import FixedMemory, TinyGaussianPolicy, TinySAC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, ACT = 5, 2            # one (obs_dim, act_dim) for the dynamics model, the ensemble snapshot, actor, critic and SAC agent
POP, P, H = 24, 5, 6       # candidates, particles, horizon of the rollouts and plans
B = POP * P                # 120 rows
ACTOR_HID, CRITIC_HID, SAC_HID, SAC_B = 40, 24, 16, 16
NAN = float("nan")
CHAINS = sc.CHAINS         # the chains ARE the table's (tests/test_stream_contract_host.py checks the identity)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(DEV).contiguous()


def poison(*tensors):
    """NaN into float buffers, 0xFF into every other"""
    for t in tensors:
        if t.dtype.is_floating_point:
            t.fill_(NAN)
        else:
            t.view(torch.uint8).fill_(0xFF)


def take(c, names):
    """{name: [host copies]} of buffers (a tensor or a list of tensors each)"""
    out = {}
    for n in names:
        v = c.bufs[n]
        out[n] = [t.detach().clone().cpu() for t in (v if isinstance(v, (list, tuple)) else [v])]
    return out


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------------------
# the steps: one function per step of the table, bound to ITS symbol (``call`` is Engine._call of the step's symbol and nothing else)
# ---------------------------------------------------------------------------------------------------------------------------------
STEPS = {}


def step(key, *outs):
    def register(fn):
        STEPS[key] = (fn, outs)
        return fn
    return register


def actor_weights(seed, hid=ACTOR_HID, fill=None):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, s: torch.randn(*shape, generator=g) * s  # noqa: E731
    w = dict(w1=r(hid, OBS, s=OBS ** -0.5), b1=r(hid, s=0.1), w2=r(hid, hid, s=hid ** -0.5), b2=r(hid, s=0.1), wm=r(ACT, hid, s=hid ** -0.5),
             bm=r(ACT, s=0.1), ws=r(ACT, hid, s=hid ** -0.5), bs=r(ACT, s=0.1) - 1.0, action_scale=torch.ones(ACT), action_bias=torch.zeros(ACT))
    return {k: dev(v if fill is None else torch.full_like(v, fill)) for k, v in w.items()}


def critic_weights(seed, hid=CRITIC_HID, fill=None):
    """[the 12 tensors of hipets_critic_set's table], nn.Linear's [out, in]"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        for n_out, n_in in ((hid, OBS + ACT), (hid, hid), (1, hid)):
            out += [torch.randn(n_out, n_in, generator=g) * n_in ** -0.5, torch.randn(n_out, generator=g) * 0.1]
    return [dev(v if fill is None else torch.full_like(v, fill)) for v in out]


def table_of(tensors):
    return np.array([t.data_ptr() for t in tensors], dtype=np.uint64)


def policy_set(call, w):
    call(obs_dim=OBS, hidden=int(w["w1"].shape[0]), act_dim=ACT, **w)


def critic_set(call, table):
    call(obs_dim=OBS, act_dim=ACT, hidden=CRITIC_HID, ptrs=table, n_ptrs=12)


def start_rows(s0, n, seed):
    return dev((s0[None, :] + 0.02 * np.random.default_rng(seed).standard_normal((n, OBS))).astype(np.float32))


# ---- actor, model and value --------------------------------------------------------------------------------------------------
def build_actor_model_value(own):
    c = SimpleNamespace(own=own)
    f = lambda *shape: torch.empty(*shape, device=DEV)  # noqa: E731
    c.obs = start_rows(own.s0, B, 1)
    c.W1, c.W_nan = actor_weights(11), actor_weights(11, fill=NAN)
    c.actions, c.act_mean = f(B, ACT), f(B, ACT)
    c.next_obs, c.rewards, c.dones = f(B, OBS), f(B), torch.empty(B, dtype=torch.uint8, device=DEV)
    c.critic = critic_weights(12)
    c.critic_nan_tensors = critic_weights(12, fill=NAN)  # (kept: the table holds their addresses)
    c.critic_nan = table_of(c.critic_nan_tensors)
    # the critic of the chain: the output biases of Q1 and Q2 are the first two rewards of the step before it
    table = table_of(c.critic)
    table[5], table[11] = c.rewards.data_ptr(), c.rewards.data_ptr() + 4
    c.critic_table = table
    c.q = f(3, B)                      # q1, q2, qmin: 360 floats, read by the ensemble as 72 observations
    c.n_ens = 3 * B // OBS             # 72
    c.ens_mean, c.stats = f(5, c.n_ens, OBS + 1), f(c.n_ens, 4)
    c.pen_rewards0 = dev(np.random.default_rng(2).standard_normal(c.n_ens).astype(np.float32))
    c.pen_rewards, c.pen_dones = f(c.n_ens), torch.empty(c.n_ens, dtype=torch.uint8, device=DEV)
    c.halt = NAN                       # fixed below from the first serial pass: the median of the statistic, so that rows halt and rows do not
    c.dret, c.drow, c.dfirst = f(4), f(12), torch.empty(12, dtype=torch.int32, device=DEV)
    c.W2 = dict(actor_weights(13))     # its action bias is the returns of the step before it
    c.W2["action_bias"] = f(ACT)
    c.trow, c.tfirst = f(4), torch.empty(4, dtype=torch.int32, device=DEV)
    c.pr_actions, c.pr_states = f(POP, 4, ACT), f(5, POP, OBS)
    c.step_opts = _lib.RolloutOpts(mode=_lib.MODE_FAST, seed=5, stream_id=2)
    c.bufs = dict(actions=c.actions, act_mean=c.act_mean, next_obs=c.next_obs, rewards=c.rewards, dones=c.dones, q=c.q, ens_mean=c.ens_mean,
                  stats=c.stats, pen_rewards=c.pen_rewards, pen_dones=c.pen_dones, dret=c.dret, drow=c.drow, dfirst=c.dfirst,
                  returns_bias=c.W2["action_bias"], trow=c.trow, tfirst=c.tfirst, pr_actions=c.pr_actions, pr_states=c.pr_states)

    def reset(chain):
        e = own.eng
        policy_set(functools.partial(e._call, "hipets_policy_set"), c.W_nan)
        critic_set(functools.partial(e._call, "hipets_critic_set"), c.critic_nan)
        poison(*c.bufs.values())
        c.pen_rewards.copy_(c.pen_rewards0)
        c.pen_dones.zero_()
        torch.cuda.synchronize()

    c.reset = reset
    # the halt threshold is a constant of the case, taken once from the chain's own serial statistics
    reset("actor_model_value")
    run_chain(own.eng, c, "actor_model_value", None)
    c.halt = float(c.stats[:, 1].median())
    return c


@step("hipets_policy_set")
def _(c, call):
    policy_set(call, c.W1)


@step("hipets_policy_act", "actions", "act_mean")
def _(c, call):
    call(obs=c.obs, batch=B, sample=1, seed=3, stream_id=1, eps=None, actions=c.actions, mean_out=c.act_mean, log_std_out=None)


@step("hipets_step", "next_obs", "rewards", "dones")
def _(c, call):
    call(obs=c.obs, actions=c.actions, batch=B, opts=c.step_opts, next_obs=c.next_obs, rewards=c.rewards, dones=c.dones)


@step("hipets_critic_set")
def _(c, call):
    critic_set(call, c.critic_table)


@step("hipets_critic_q", "q")
def _(c, call):
    call(obs=c.next_obs, actions=c.actions, batch=B, q1=c.q[0], q2=c.q[1], qmin=c.q[2])


@step("hipets_ensemble_predict", "ens_mean", "stats")
def _(c, call):
    call(obs=c.q.view(c.n_ens, OBS), actions=c.actions[:c.n_ens], model_in=None, batch=c.n_ens, only_elite=0, mean=c.ens_mean, logvar=None,
         stats=c.stats)


@step("hipets_uncertainty_penalty", "pen_rewards", "pen_dones")
def _(c, call):
    call(stats=c.stats, stat=1, coef=0.5, halt_threshold=c.halt, halt_reward=-1.0, use_halt_reward=1, batch=c.n_ens, rewards=c.pen_rewards,
         dones=c.pen_dones)


@step("hipets_discounted_returns", "dret", "drow", "dfirst")
def _(c, call):  # the 72 penalised rewards as 6 steps of 4 candidates x 3 particles, bootstrapped with the first 12 qmin
    call(rewards=c.pen_rewards, dones=c.pen_dones, terminal_values=c.q[2], gamma=0.97, pop=4, horizon=6, num_particles=3, returns=c.dret,
         row_totals=c.drow, first_done=c.dfirst)


@step("hipets_trajectory_returns", "returns_bias", "trow", "tfirst")
def _(c, call):  # the 12 row totals as 3 steps of 2 candidates x 2 particles
    call(rewards=c.drow, dones=c.pen_dones, pop=2, horizon=3, num_particles=2, returns=c.W2["action_bias"], row_totals=c.trow, first_done=c.tfirst)


@step("hipets_policy_set#returns")
def _(c, call):
    policy_set(call, c.W2)


@step("hipets_policy_rollout#actor", "pr_actions", "pr_states")
def _(c, call):
    call(s0=c.obs, n=POP, horizon=4, mean_rows=1, only_elite=0, seed=7, stream_id=9, eps=None, actions=c.pr_actions, states=c.pr_states)


# ---- rollouts and plans ------------------------------------------------------------------------------------------------------
ICEM_ITERS, ICEM_K, ICEM_KEEP = 3, 4, 2


def icem_params(horizon):
    return _lib.IcemParams(population_size=POP, horizon=horizon, act_dim=ACT, num_iterations=ICEM_ITERS, elite_num=ICEM_K, keep_elite_size=ICEM_KEEP,
                           population_size_module=0, return_mean_elites=0, alpha=0.1, population_decay_factor=1.25, colored_noise_exponent=2.0)


def keep_indices(n_env, seed):
    return dev(np.random.default_rng(seed).integers(0, ICEM_K, (ICEM_ITERS, n_env, ICEM_KEEP)).astype(np.int32))


PLAN_MODE = {"policy_rollout_cem_fast": "fast", "mppi_icem_device": "device", "batched_plans_fast": "fast", "batched_icem_device": "device"}


def build_plans(own):
    c = SimpleNamespace(own=own)
    f = lambda *shape: torch.empty(*shape, device=DEV)  # noqa: E731
    g = torch.Generator().manual_seed(21)
    c.obs = start_rows(own.s0, POP, 3)
    c.W0 = actor_weights(14)
    c.s0 = np.ascontiguousarray(own.s0)
    c.s0_2 = np.ascontiguousarray(np.stack([own.s0, own.s0 + np.float32(0.01)]))
    c.lower, c.upper = dev(-torch.ones(H, ACT)), dev(torch.ones(H, ACT))
    c.fixed_actions = dev(torch.rand(POP, H, ACT, generator=g) * 2 - 1)
    c.fixed24 = dev(torch.rand(POP, generator=g) - 0.5)
    c.fixed_x = dev(torch.rand(2, H, ACT, generator=g) - 0.5)
    c.cem = hipets.Engine.cem_params(POP, H, ACT, 2, 3, 0.1, return_mean_elites=True)
    c.icem = icem_params(H)
    c.keep1, c.keep2 = keep_indices(1, 5), keep_indices(2, 6)
    c.pr_actions = f(POP, H, ACT)      # the policy rollout's actions: what the rollout of 24 candidates evaluates
    c.ret24 = f(POP)                   # that rollout's returns; its first 12 are the plan variable of the plan behind it
    c.plan_out = f(H, ACT)             # hipets_plan_cem's plan
    c.x_next = f(H, ACT)               # element 0: the return of a plan's rollout; the start of the plan behind it
    c.xb = f(2, H, ACT)                # [0]: hipets_plan_icem's plan; the start of the batched plan behind it
    c.elite, c.elite_b = f(ICEM_K, H, ACT), f(2, ICEM_K, H, ACT)
    c.outb, c.outc = f(2, H, ACT), f(2, H, ACT)
    c.ret1 = c.x_next.view(-1)[:1]
    c.bufs = dict(pr_actions=c.pr_actions, ret24=c.ret24, plan_out=c.plan_out, x_next=c.x_next, xb=c.xb, elite=c.elite, elite_b=c.elite_b,
                  outb=c.outb, outc=c.outc)

    def reset(chain):
        e = own.eng
        e.set_plan_mode(PLAN_MODE[chain])
        c.mode = _lib.MODES[PLAN_MODE[chain]]
        policy_set(functools.partial(e._call, "hipets_policy_set"), c.W0)
        poison(*c.bufs.values())
        # what a chain's first step reads, and the elements of a plan variable no call of the chain writes
        c.x_next.copy_(c.fixed_x[0])
        c.xb.copy_(c.fixed_x)
        if chain == "policy_rollout_cem_fast":
            c.x_next.view(-1)[0] = NAN
            c.plan_result = c.plan_out
        elif chain == "mppi_icem_device":
            c.pr_actions.copy_(c.fixed_actions)
            c.x_next.view(-1)[0] = NAN
            c.plan_result = c.ret24[:H * ACT]
        else:  # (the rollout of two candidates writes two of the 24 returns)
            c.ret24.copy_(c.fixed24)
            c.ret24[:2] = NAN
            if chain == "batched_plans_fast":
                c.xb[0] = NAN
                c.batched_result = c.outb
            else:
                c.outb.copy_(c.fixed_x)
                c.batched_result = c.outc
        torch.cuda.synchronize()

    c.reset = reset
    return c


def rollout_opts(c, stream_id, n_env=0):
    return _lib.RolloutOpts(mode=c.mode, seed=11, stream_id=stream_id, n_env=n_env)


@step("hipets_policy_rollout", "pr_actions")
def _(c, call):
    call(s0=c.obs, n=POP, horizon=H, mean_rows=1, only_elite=0, seed=7, stream_id=1, eps=None, actions=c.pr_actions, states=None)


@step("hipets_rollout", "ret24")
def _(c, call):
    call(actions=c.pr_actions, s0=c.s0, pop=POP, horizon=H, num_particles=P, opts=rollout_opts(c, 1), returns=c.ret24)


@step("hipets_plan_cem", "plan_out")
def _(c, call):
    call(p=c.cem, x0=c.ret24, lower=c.lower, upper=c.upper, s0=c.s0, num_particles=P, seed=13, plan_id=1, out=c.plan_out)


@step("hipets_rollout#plan", "x_next")
def _(c, call):  # one candidate: the plan of the step before
    call(actions=c.plan_result, s0=c.s0, pop=1, horizon=H, num_particles=P, opts=rollout_opts(c, 2), returns=c.ret1)


@step("hipets_plan_mppi", "ret24")
def _(c, call):  # the mean, refined in place, is the first 12 returns of the step before
    call(population_size=POP, horizon=H, act_dim=ACT, num_iterations=2, gamma=1.0, beta=0.6, mean=c.ret24, lower=c.lower, upper=c.upper, s0=c.s0,
         num_particles=P, seed=13, plan_id=2)


@step("hipets_plan_icem", "xb", "elite")
def _(c, call):
    call(p=c.icem, x0=c.x_next, lower=c.lower, upper=c.upper, elite=c.elite, has_elite=0, keep_idx=c.keep1, s0=c.s0, num_particles=P, seed=13,
         plan_id=3, out=c.xb[0])


@step("hipets_plan_cem_batched", "outb")
def _(c, call):
    call(p=c.cem, n_env=2, x0=c.xb, lower=c.lower, upper=c.upper, s0=c.s0_2, num_particles=P, seed=13, plan_id=4, out=c.outb)


@step("hipets_plan_mppi_batched", "outb")
def _(c, call):
    call(population_size=POP, horizon=H, act_dim=ACT, num_iterations=2, gamma=1.0, beta=0.6, n_env=2, mean=c.outb, lower=c.lower, upper=c.upper,
         s0=c.s0_2, num_particles=P, seed=13, plan_id=5)


@step("hipets_plan_icem_batched", "outc", "elite_b")
def _(c, call):
    call(p=c.icem, n_env=2, x0=c.outb, lower=c.lower, upper=c.upper, elite=c.elite_b, has_elite=0, keep_idx=c.keep2, s0=c.s0_2, num_particles=P,
         seed=13, plan_id=6, out=c.outc)


@step("hipets_rollout#batched", "ret24")
def _(c, call):  # one candidate per environment: the batched plans of the step before
    call(actions=c.batched_result, s0=c.s0_2, pop=2, horizon=H, num_particles=P, opts=rollout_opts(c, 3, n_env=2), returns=c.ret24)


# ---- MBPO --------------------------------------------------------------------------------------------------------------------
RING_CAP, STAGE_CAP = 256, 32
MBPO_MIN_KEPT = SAC_B  # the gathered indices stay below the rows the ring holds (asserted on the serial run)


def build_mbpo(own):
    c = SimpleNamespace(own=own)
    f = lambda *shape: torch.empty(*shape, device=DEV)  # noqa: E731
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=DEV)  # noqa: E731
    W = row_width(OBS, ACT)
    rng = np.random.default_rng(31)
    c.obs = start_rows(own.s0, B, 4)
    c.obs[:, 0] = dev((0.55 + 0.3 * rng.random(B)).astype(np.float32))  # heights on both sides of hopper's 0.7: rows end, rows stay
    c.actions = dev(rng.uniform(-1, 1, (B, ACT)).astype(np.float32))
    c.next_obs, c.rewards, c.dones, c.accum = f(B, OBS), f(B), u8(B), u8(B)
    c.ring, c.cursor, c.count = f(RING_CAP * W), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    c.idx = dev(rng.integers(0, MBPO_MIN_KEPT, SAC_B).astype(np.int64))
    c.batch, c.result, c.taps = f(SAC_B, W), f(8), f(5, SAC_B)
    c.eps_next, c.eps_cur = dev(rng.standard_normal((SAC_B, ACT)).astype(np.float32)), dev(rng.standard_normal((SAC_B, ACT)).astype(np.float32))
    c.next16 = dev(rng.standard_normal((SAC_B, OBS)).astype(np.float32))
    c.dones16 = dev((np.arange(SAC_B) % 5 == 3).astype(np.uint8))
    c.accum16 = u8(SAC_B)
    c.staging, c.offset, c.count2 = f(STAGE_CAP * W), torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    c.idx2 = dev(rng.integers(0, SAC_B, 8).astype(np.int64))
    c.out2 = f(8, W)
    c.step_opts = _lib.RolloutOpts(mode=_lib.MODE_FAST, seed=5, stream_id=4)
    torch.manual_seed(5)
    c.sac = TinySAC(OBS, ACT, SAC_HID, device=DEV)
    c.up = hipets.SACUpdater(c.sac, engine=own.eng)
    c.up._bind()
    c.sac_state = [t for t in c.up._tensors()[0] if t is not None]  # parameters, moments, targets, log_alpha, alpha: updated in place
    c.sac_start = [t.detach().clone() for t in c.sac_state]
    with torch.no_grad():  # (the coefficient the kernels read: what the updater copies in before an update)
        c.sac_start[next(i for i, t in enumerate(c.sac_state) if t is c.up._alpha)].fill_(float(c.sac.alpha))
    c.bufs = dict(next_obs=c.next_obs, rewards=c.rewards, dones=c.dones, accum=c.accum, ring=c.ring, cursor=c.cursor, count=c.count, batch=c.batch,
                  sac_state=c.sac_state, result=c.result, taps=c.taps, accum16=c.accum16, staging=c.staging, offset=c.offset, count2=c.count2,
                  out2=c.out2)
    c.partial = {"ring", "staging"}  # rows no call writes keep their poison

    def reset(chain):
        c.up._bind()  # (another updater may hold the engine's SAC slot by now)
        with torch.no_grad():
            for t, t0 in zip(c.sac_state, c.sac_start):
                t.copy_(t0)
        poison(c.next_obs, c.rewards, c.dones, c.ring, c.batch, c.result, c.taps, c.staging, c.out2)
        for t in (c.accum, c.accum16, c.cursor, c.count, c.offset, c.count2):  # read before they are written: set before the gate
            t.zero_()
        torch.cuda.synchronize()

    c.reset = reset
    return c


@step("hipets_ring_compact_transitions", "accum", "ring", "cursor", "count")
def _(c, call):
    call(obs=c.obs, action=c.actions, next_obs=c.next_obs, rewards=c.rewards, dones=c.dones, accum_dones=c.accum, n=B, obs_dim=OBS, act_dim=ACT,
         ring=c.ring, capacity=RING_CAP, cursor=c.cursor, count_out=c.count)


@step("hipets_replay_gather", "batch")
def _(c, call):
    call(ring=c.ring, capacity=RING_CAP, obs_dim=OBS, act_dim=ACT, indices=c.idx, n_rows=SAC_B, reverse_mask=1, out=c.batch)


@step("hipets_sac_update", "sac_state", "result")
def _(c, call):
    call(batch=c.batch, batch_size=SAC_B, eps_next=c.eps_next, eps_cur=c.eps_cur, update_index=0, step_critic=0, step_policy=0, step_alpha=0,
         lr_critic=3e-4, lr_policy=3e-4, lr_alpha=3e-4, result=c.result)


@step("hipets_sac_forward_taps", "taps")
def _(c, call):
    call(batch_size=SAC_B, q1=c.taps[0], q2=c.taps[1], y=c.taps[2], log_pi_next=c.taps[3], log_pi=c.taps[4])


@step("hipets_compact_transitions", "accum16", "staging", "offset", "count2")
def _(c, call):  # 16 transitions whose rewards are the update's q1 taps
    call(obs=c.obs, action=c.actions, next_obs=c.next16, rewards=c.taps[0], dones=c.dones16, accum_dones=c.accum16, n=SAC_B, obs_dim=OBS,
         act_dim=ACT, staging=c.staging, cap=STAGE_CAP, offset=c.offset, count_out=c.count2)


@step("hipets_replay_gather#staging", "out2")
def _(c, call):  # (a staging area has the ring's layout)
    call(ring=c.staging, capacity=STAGE_CAP, obs_dim=OBS, act_dim=ACT, indices=c.idx2, n_rows=8, reverse_mask=0, out=c.out2)


# ---- trainer -----------------------------------------------------------------------------------------------------------------
T_E, T_B, T_IN, T_HID, T_OUT, T_L, T_N, T_N2 = 3, 17, 5, 37, 4, 3, 64, 48  # tests/test_gpu_trainer.py "odd_hid37_in5_b17"


def build_trainer(own):
    c = SimpleNamespace(own=own)
    f = lambda *shape: torch.empty(*shape, device=DEV)  # noqa: E731
    g = torch.Generator().manual_seed(41)
    ws, bs = tr.random_model(T_E, T_IN, T_HID, T_OUT, T_L, 0)
    c.w0, c.b0 = [dev(w.float()) for w in ws], [dev(b.float()) for b in bs]
    c.w, c.b = [t.clone() for t in c.w0], [t.clone() for t in c.b0]
    c.m, c.v = ([torch.zeros_like(t) for t in c.w], [torch.zeros_like(t) for t in c.b]), ([torch.zeros_like(t) for t in c.w], [torch.zeros_like(t) for t in c.b])
    c.x, c.y = dev(torch.randn(T_N, T_IN, generator=g)), dev(torch.randn(T_N, T_OUT, generator=g) * 0.3)
    c.lo, c.hi = dev(-10 * torch.ones(T_OUT)), dev(0.5 * torch.ones(T_OUT))
    # every schedule indexes rows below 48: the calls whose targets are the 192 row scores of an evaluation have 48 rows
    c.idx = dev(torch.stack([torch.stack([torch.randperm(T_N2, generator=g)[:T_B] for _ in range(T_E)]) for _ in range(2)]).to(torch.int32))
    c.rows = dev(torch.full((2,), T_B, dtype=torch.int32))
    c.order = dev(torch.randperm(T_N, generator=g).to(torch.int32))
    c.loss, c.gsq = f(3, 2, T_E), f(3, 2, T_E)
    c.score, c.row_score = f(2, T_E), f(2, T_E, T_N)
    c.d_train, c.keep_train = pack_train_desc(torch.device(DEV), c.w, c.b, "silu", 0.01, T_OUT, T_B,
                                              adam=(c.m[0], c.m[1], c.v[0], c.v[1], c.lo, c.hi, 1e-3, 0.9, 0.999, 1e-8, 1e-5, 0))
    c.d_eval, c.keep_eval = pack_train_desc(torch.device(DEV), c.w, c.b, "silu", 0.01, T_OUT, 1)
    c.bufs = dict(params=c.w + c.b, moments=c.m[0] + c.m[1] + c.v[0] + c.v[1], loss=c.loss, gsq=c.gsq, score=c.score, row_score=c.row_score)

    def reset(chain):
        for t, t0 in zip(c.w + c.b, c.w0 + c.b0):
            t.copy_(t0)
        for t in c.bufs["moments"]:
            t.zero_()
        poison(c.loss, c.gsq, c.score, c.row_score)
        torch.cuda.synchronize()

    c.reset = reset
    return c


def scores_as_targets(c, k):
    """the first 192 row scores of evaluation k as the targets [48, 4] of the steps behind it"""
    return c.row_score[k].view(-1)[:T_N2 * T_OUT]


@step("hipets_train_steps", "params", "moments", "loss", "gsq")
def _(c, call):
    call(d=c.d_train, x=c.x, y=c.y, n_rows=T_N, idx=c.idx, rows=c.rows, n_steps=2, step0=0, loss=c.loss[0], grad_sq=c.gsq[0])


@step("hipets_train_eval", "score", "row_score")
def _(c, call):
    call(d=c.d_eval, x=c.x, y=c.y, n_rows=T_N, order=None, score=c.score[0], row_score=c.row_score[0])


@step("hipets_train_steps_loss", "params", "moments", "loss", "gsq")
def _(c, call):
    call(d=c.d_train, x=c.x, y=scores_as_targets(c, 0), n_rows=T_N2, idx=c.idx, rows=c.rows, n_steps=2, step0=2, loss=c.loss[1], grad_sq=c.gsq[1],
         loss_kind=_lib.TRAIN_LOSS["nll"], bounds_per_member=0, grad_scale=0.5)


@step("hipets_train_eval_loss", "score", "row_score")
def _(c, call):
    call(d=c.d_eval, x=c.x, y=c.y, n_rows=T_N, order=c.order, score=c.score[1], row_score=c.row_score[1], loss_kind=_lib.TRAIN_LOSS["nll"])


@step("hipets_train_steps#scores", "params", "moments", "loss", "gsq")
def _(c, call):
    call(d=c.d_train, x=c.x, y=scores_as_targets(c, 1), n_rows=T_N2, idx=c.idx, rows=c.rows, n_steps=2, step0=4, loss=c.loss[2], grad_sq=c.gsq[2])


# ---- PlaNet ------------------------------------------------------------------------------------------------------------------
PL_LATENT, PL_BELIEF, PL_HID, PL_H, PL_P = 7, 22, 19, 5, 2  # tests/test_gpu_planet.py: nothing a multiple of 4


def build_planet(own):
    c = SimpleNamespace(own=own)
    f = lambda *shape: torch.empty(*shape, device=DEV)  # noqa: E731
    g = torch.Generator().manual_seed(51)
    c.latent, c.belief = dev(torch.randn(2, PL_LATENT, generator=g) * 0.3), dev(torch.randn(2, PL_BELIEF, generator=g) * 0.3)
    c.lower, c.upper = dev(-torch.ones(PL_H, ACT)), dev(torch.ones(PL_H, ACT))
    c.fixed_x = dev(torch.rand(2, PL_H, ACT, generator=g) - 0.5)
    c.cem = hipets.Engine.cem_params(POP, PL_H, ACT, 2, 3, 0.1, return_mean_elites=True)
    c.icem = icem_params(PL_H)
    c.keep = keep_indices(2, 7)
    c.x0 = dev(c.fixed_x[0].clone())
    c.out1, c.xb, c.outb, c.outc, c.x_last, c.out3 = f(PL_H, ACT), f(2, PL_H, ACT), f(2, PL_H, ACT), f(2, PL_H, ACT), f(PL_H, ACT), f(PL_H, ACT)
    c.elite = f(2, ICEM_K, PL_H, ACT)
    c.bufs = dict(out1=c.out1, xb=c.xb, outb=c.outb, outc=c.outc, elite=c.elite, x_last=c.x_last, out3=c.out3)

    def reset(chain):
        poison(*c.bufs.values())
        c.xb.copy_(c.fixed_x)      # all but element 0, the return of the first plan's rollout
        c.xb.view(-1)[0] = NAN
        c.x_last.copy_(c.fixed_x[1])
        c.x_last.view(-1)[:2] = NAN  # the returns of the batched plans' rollout
        torch.cuda.synchronize()

    c.reset = reset
    return c


@step("hipets_plan_planet_cem", "out1")
def _(c, call):
    call(p=c.cem, x0=c.x0, lower=c.lower, upper=c.upper, latent0=c.latent, belief0=c.belief, num_particles=PL_P, seed=17, plan_id=1, out=c.out1)


@step("hipets_planet_rollout", "xb")
def _(c, call):
    call(actions=c.out1, latent0=c.latent, belief0=c.belief, pop=1, horizon=PL_H, num_particles=PL_P, opts=_lib.PlanetOpts(seed=19, stream_id=1),
         returns=c.xb)


@step("hipets_plan_planet_cem_batched", "outb")
def _(c, call):
    call(p=c.cem, n_env=2, x0=c.xb, lower=c.lower, upper=c.upper, latent0=c.latent, belief0=c.belief, num_particles=PL_P, seed=17, plan_id=2,
         out=c.outb)


@step("hipets_plan_planet_mppi_batched", "outb")
def _(c, call):
    call(population_size=POP, horizon=PL_H, act_dim=ACT, num_iterations=2, gamma=1.0, beta=0.6, n_env=2, mean=c.outb, lower=c.lower, upper=c.upper,
         latent0=c.latent, belief0=c.belief, num_particles=PL_P, seed=17, plan_id=3)


@step("hipets_plan_planet_icem_batched", "outc", "elite")
def _(c, call):
    call(p=c.icem, n_env=2, x0=c.outb, lower=c.lower, upper=c.upper, elite=c.elite, has_elite=0, keep_idx=c.keep, latent0=c.latent, belief0=c.belief,
         num_particles=PL_P, seed=17, plan_id=4, out=c.outc)


@step("hipets_planet_rollout#batched", "x_last")
def _(c, call):
    call(actions=c.outc, latent0=c.latent, belief0=c.belief, pop=2, horizon=PL_H, num_particles=PL_P,
         opts=_lib.PlanetOpts(seed=19, stream_id=2, n_env=2), returns=c.x_last)


@step("hipets_plan_planet_cem#returns", "out3")
def _(c, call):
    call(p=c.cem, x0=c.x_last, lower=c.lower, upper=c.upper, latent0=c.latent, belief0=c.belief, num_particles=PL_P, seed=17, plan_id=5, out=c.out3)


FAMILY = {"actor_model_value": build_actor_model_value, "policy_rollout_cem_fast": build_plans, "mppi_icem_device": build_plans,
          "batched_plans_fast": build_plans, "batched_icem_device": build_plans, "mbpo": build_mbpo, "trainer": build_trainer, "planet": build_planet}


# ---------------------------------------------------------------------------------------------------------------------------------
# running a chain
# ---------------------------------------------------------------------------------------------------------------------------------
def run_chain(eng, c, chain, streams):
    """enqueue the chain's calls: on the default stream with a synchronisation behind each (``streams`` None), or step k on
    ``streams[k % 2]`` with nothing between the calls; returns the host time the enqueueing took"""
    t0 = time.perf_counter()
    for k, key in enumerate(CHAINS[chain]):
        fn = STEPS[key][0]
        call = functools.partial(eng._call, sc.symbol_of(key))
        if streams is None:
            fn(c, call)
            torch.cuda.synchronize()
        else:
            with torch.cuda.stream(streams[k % 2]):
                fn(c, call)
    return time.perf_counter() - t0


def outputs_of(chain):
    names = []
    for key in CHAINS[chain]:
        names += [n for n in STEPS[key][1] if n not in names]
    return names


def first_difference(chain, got, ref):
    """None, or the first call of the chain one of whose outputs differs from the serial run's"""
    steps = CHAINS[chain]
    for k, key in enumerate(steps):
        bad = [n for n in STEPS[key][1] if not same_bits(got[n], ref[n])]
        if bad:
            before = f" (it reads what step {k - 1}, {steps[k - 1]}, wrote)" if k else ""
            return f"chain {chain}: step {k}, {key}, is the first call whose output differs from the serial run: {', '.join(bad)}{before}"
    return None


class Own:
    """the module's own engine, its models, and per chain the buffers and the serial run's bits"""

    def __init__(self):
        self.eng = hipets.Engine(DEV)
        self.eng.set_persistent(False)  # two persistent kernels side by side would wait for each other: never in this module
        om, self.s0 = cc.make_case(OBS, ACT, dict(ensemble_size=5, hid=40, termination="hopper", learned_rewards=True, reward=None))
        self.spec = to_spec(om, OBS, ACT)
        self.eng.set_model(self.spec)
        self.eng.ensemble_set(self.spec)
        pm = pl.make_synthetic_planet(PL_LATENT, ACT, PL_BELIEF, PL_HID, seed=9)
        self.planet_spec = hipets.PlaNetSpec(**{k: getattr(pm, k) for k in pl.PLANET_TENSORS}, min_std=pm.min_std)
        self.eng.planet_set_model(self.planet_spec)
        self._families, self._refs = {}, {}

    def family(self, chain):
        build = FAMILY[chain]
        if build not in self._families:
            self._families[build] = build(self)
        return self._families[build]

    def reference(self, chain):
        """the chain on the default stream, a synchronisation behind every call: computed once, never changed"""
        if chain not in self._refs:
            c = self.family(chain)
            c.reset(chain)
            run_chain(self.eng, c, chain, None)
            self._refs[chain] = take(c, outputs_of(chain))
        return self._refs[chain]


@pytest.fixture(scope="module")
def own():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t0 = time.perf_counter()
    o = Own()
    yield o
    torch.cuda.synchronize()
    o.eng.close()
    print(f"\n[streams] module wall time {time.perf_counter() - t0:.1f} s")


@pytest.fixture(scope="module")
def lanes(own):
    """the stream pairs of the two pairings, each shown to run concurrently (stream_gate.calibrate), and a third stream"""
    fresh = [torch.cuda.Stream(DEV) for _ in range(sg.MAX_CANDIDATES + 1)]
    default = torch.cuda.default_stream(torch.device(DEV))
    i, second = sg.calibrate(fresh[0], fresh[1:])
    j, side = sg.calibrate(default, fresh)
    third = next(s for s in fresh if s is not fresh[0] and s is not second)
    print(f"[streams] pairing side_side: gated stream = fresh stream 0, second = candidate {i}; pairing default_side: gated stream = "
          f"the default stream, second = candidate {j}")
    return {"side_side": (fresh[0], second), "default_side": (default, side), "third": third, "chosen": {"side_side": i, "default_side": j}}


def gated_run(lanes, pairing, what, enqueue):
    """``enqueue(streams)`` three times: it resets and enqueues the case; un-gated for the host's time, then behind a gate sized from
    it.  Returns after the gated run has executed; fails if the gate had ended before the last call was enqueued."""
    streams = lanes[pairing]
    took = enqueue(streams, None)
    torch.cuda.synchronize()
    if sg.MIN_FACTOR * took > sg.MAX_GATE_S:  # a host hiccup in the warm-up is no property of the case: time it once more
        took = min(took, enqueue(streams, None))
        torch.cuda.synchronize()
    length = sg.gate_length(took)
    done = enqueue(streams, length)
    closed = sg.still_closed(done)
    torch.cuda.synchronize()
    print(f"[streams] {what} / {pairing}: un-gated enqueue {took * 1e3:.2f} ms, gate {length * 1e3:.1f} ms ({length / took:.0f} x), "
          f"second stream = candidate {lanes['chosen'][pairing]}, gate still closed after the last enqueue: {closed}")
    assert closed, f"{what} / {pairing}: the gate ({length * 1e3:.1f} ms) had ended before the last call was enqueued: the run proves nothing"


# ---------------------------------------------------------------------------------------------------------------------------------
# gated dependency chains
# ---------------------------------------------------------------------------------------------------------------------------------
PAIRING_IDS = [p[0] for p in sc.PAIRINGS]


def test_calibration_an_unordered_reader_sees_the_old_value(lanes):
    """(stream_gate.calibrate has asserted it for both pairings when the fixture was built: without it no gated case has power)"""
    assert set(PAIRING_IDS) <= set(lanes)


@pytest.mark.parametrize("pairing", PAIRING_IDS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_gated_chain_gives_the_serial_bits(own, lanes, chain, pairing):
    c, ref = own.family(chain), own.reference(chain)
    names = outputs_of(chain)
    for n in names:  # the serial run itself: no poison left, so a NaN in a gated run is a missed wait and nothing else
        if n not in getattr(c, "partial", ()):
            assert all(bool(torch.isfinite(t).all()) for t in ref[n] if t.dtype.is_floating_point), f"{chain}: serial {n} is not finite"
    if chain == "mbpo":  # every row was alive before the step (all are stored); the step's own ends reach the ring's done column and the flags
        ended = int((ref["dones"][0] != 0).sum())
        assert int(ref["count"][0][0]) == B >= MBPO_MIN_KEPT and 0 < ended < B, f"{ended} of {B} rows ended in the step"
        assert torch.equal(ref["accum"][0], ref["dones"][0])
    if chain == "actor_model_value":
        halted = int(ref["pen_dones"][0].sum())
        assert 0 < halted < c.n_ens, f"{halted} of {c.n_ens} rows halted"
    results = {}

    def enqueue(streams, length):
        c.reset(chain)
        done = sg.gate(streams[0], length) if length is not None else None
        took = run_chain(own.eng, c, chain, streams)
        if length is None:
            torch.cuda.synchronize()
            results["ungated"] = take(c, names)
            return took
        return done

    gated_run(lanes, pairing, chain, enqueue)
    results["gated"] = take(c, names)
    for how in ("gated", "ungated"):
        diff = first_difference(chain, results[how], ref)
        assert diff is None, f"{how}, {pairing}: {diff}"


# ---------------------------------------------------------------------------------------------------------------------------------
# snapshot slots under a gate; calls that take no part
# ---------------------------------------------------------------------------------------------------------------------------------
class Slots:
    """an actor and a critic, two snapshots each, and their serial outputs"""

    def __init__(self, own):
        e = self.eng = own.eng
        self.obs = start_rows(own.s0, B, 8)
        self.act = dev(np.random.default_rng(9).uniform(-1, 1, (B, ACT)).astype(np.float32))
        self.W = [actor_weights(61, hid=72), actor_weights(62, hid=72)]
        self.C = [critic_weights(63), critic_weights(64)]
        self.tables = [table_of(t) for t in self.C]
        self.out_a, self.out_q = torch.empty(B, ACT, device=DEV), torch.empty(3, B, device=DEV)
        self.serial = {}
        for k in (0, 1):
            self.set("policy", k)
            self.read("policy")
            self.set("critic", k)
            self.read("critic")
            torch.cuda.synchronize()
            self.serial["policy", k], self.serial["critic", k] = self.out_a.clone(), self.out_q.clone()

    def set(self, slot, k):
        if slot == "policy":
            policy_set(functools.partial(self.eng._call, "hipets_policy_set"), self.W[k])
        else:
            critic_set(functools.partial(self.eng._call, "hipets_critic_set"), self.tables[k])

    def read(self, slot):
        if slot == "policy":
            self.eng._call("hipets_policy_act", obs=self.obs, batch=B, sample=0, seed=0, stream_id=0, eps=None, actions=self.out_a, mean_out=None,
                           log_std_out=None)
        else:
            self.eng._call("hipets_critic_q", obs=self.obs, actions=self.act, batch=B, q1=self.out_q[0], q2=self.out_q[1], qmin=self.out_q[2])

    def out(self, slot):
        return self.out_a if slot == "policy" else self.out_q


@pytest.fixture(scope="module")
def slots(own):
    return Slots(own)


@pytest.mark.parametrize("pairing", PAIRING_IDS)
@pytest.mark.parametrize("slot", ["policy", "critic"])
def test_a_snapshot_set_behind_a_gate_is_the_one_the_next_call_reads(slots, lanes, slot, pairing):
    """W0 is set and used; then W1 is set on the gated stream and read on the other: the result carries W1's bits, not W0's"""
    w0, w1 = slots.serial[slot, 0], slots.serial[slot, 1]
    assert torch.isfinite(w0).all() and torch.isfinite(w1).all() and not torch.equal(w0, w1)

    def enqueue(streams, length):
        slots.set(slot, 0)
        slots.read(slot)
        torch.cuda.synchronize()
        assert torch.equal(slots.out(slot), w0)
        poison(slots.out(slot))
        torch.cuda.synchronize()
        done = sg.gate(streams[0], length) if length is not None else None
        t0 = time.perf_counter()
        with torch.cuda.stream(streams[0]):
            slots.set(slot, 1)
        with torch.cuda.stream(streams[1]):
            slots.read(slot)
        return time.perf_counter() - t0 if length is None else done

    gated_run(lanes, pairing, f"snapshot {slot}", enqueue)
    got = slots.out(slot)
    assert not torch.equal(got, w0), f"{slot}: the reader saw the snapshot from before"
    assert same_bits([got], [w1]), f"{slot}: the reader did not see the snapshot set on the other stream"


def _cem_sample(s, call, out):
    call(p=s.cem, mu=s.mu, dispersion=s.disp, lower=s.lower, upper=s.upper, z=None, seed=3, stream_id=4, population=out)


def _particle_reduce(s, call, out):
    call(totals=s.totals, pop=POP, num_particles=P, returns=out)


def _policy_normals(s, call, out):
    call(batch=B, act_dim=ACT, seed=3, stream_id=5, out=out)


LAUNCH_ONLY_BETWEEN = {"hipets_cem_sample": (_cem_sample, (POP, H, ACT)), "hipets_particle_reduce": (_particle_reduce, (POP,)),
                       "hipets_policy_normals": (_policy_normals, (B, ACT))}
REFUSED_BETWEEN = {"hipets_policy_act": dict(obs="obs", batch=0, sample=0, seed=0, stream_id=0, eps=None, actions="out", mean_out=None, log_std_out=None),
                   "hipets_rollout": dict(actions="actions3", s0="s0", pop=0, horizon=H, num_particles=P, opts="opts", returns="out")}


@pytest.mark.parametrize("between", sorted(LAUNCH_ONLY_BETWEEN) + ["refused " + s for s in sorted(REFUSED_BETWEEN)])
def test_a_call_that_takes_no_part_leaves_the_order_intact(own, slots, lanes, between):
    """policy_set(W1) behind a gate, then a launch-only helper on a third stream or a refused call, then policy_act on the second stream:
    the actions carry W1's bits; the helper's own output is what it is alone"""
    eng, third = own.eng, lanes["third"]
    w0, w1 = slots.serial["policy", 0], slots.serial["policy", 1]
    s = SimpleNamespace(cem=hipets.Engine.cem_params(POP, H, ACT, 2, 3, 0.1), mu=torch.zeros(H, ACT, device=DEV), disp=torch.full((H, ACT), 0.25, device=DEV),
                        lower=-torch.ones(H, ACT, device=DEV), upper=torch.ones(H, ACT, device=DEV),
                        totals=dev(np.random.default_rng(3).standard_normal(B).astype(np.float32)), obs=slots.obs, actions3=torch.zeros(POP, H, ACT, device=DEV),
                        s0=np.ascontiguousarray(own.s0), opts=_lib.RolloutOpts(mode=_lib.MODE_FAST, seed=1, stream_id=1))
    refused = between.startswith("refused ")
    symbol = between.split()[-1]
    if refused:
        s.out = torch.zeros(B, ACT, device=DEV)
        kw = {k: (getattr(s, v) if isinstance(v, str) else v) for k, v in REFUSED_BETWEEN[symbol].items()}
        alone = None
    else:
        fn, shape = LAUNCH_ONLY_BETWEEN[symbol]
        out = torch.empty(*shape, device=DEV)
        fn(s, functools.partial(eng._call, symbol), out)
        torch.cuda.synchronize()
        alone = out.clone()

    def enqueue(streams, length):
        slots.set("policy", 0)
        slots.read("policy")
        poison(slots.out_a)
        if not refused:
            poison(out)
        torch.cuda.synchronize()
        done = sg.gate(streams[0], length) if length is not None else None
        t0 = time.perf_counter()
        with torch.cuda.stream(streams[0]):
            slots.set("policy", 1)
        if refused:  # the rollout is refused behind its stream entry, the actor call before it
            with torch.cuda.stream(third if symbol == "hipets_rollout" else streams[1]), pytest.raises(hipets.HipetsError) as err:
                eng._call(symbol, **kw)
            assert err.value.kind == hipets.ERR_INVALID_ARGUMENT
        else:
            with torch.cuda.stream(third):
                fn(s, functools.partial(eng._call, symbol), out)
        with torch.cuda.stream(streams[1]):
            slots.read("policy")
        return time.perf_counter() - t0 if length is None else done

    gated_run(lanes, "side_side", f"between: {between}", enqueue)
    assert not torch.equal(slots.out_a, w0) and same_bits([slots.out_a], [w1])
    if not refused:
        assert torch.isfinite(alone).all() and same_bits([out], [alone])


# ---------------------------------------------------------------------------------------------------------------------------------
# un-gated: the staging ring, workspace growth, the public wrappers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_nine_host_observations_through_the_staging_ring_across_streams(own, lanes):
    """nine rollouts and CEM plans back to back, nine different host observations, alternating streams, no synchronisation: the ring of
    four pinned slots blocks the host on a slot's fifth use (by design) and every call still computes with its own observation"""
    eng = own.eng
    eng.set_plan_mode("fast")
    g = torch.Generator().manual_seed(71)
    actions = dev(torch.rand(POP, H, ACT, generator=g) * 2 - 1)
    x0, lower, upper = torch.zeros(H, ACT, device=DEV), -torch.ones(H, ACT, device=DEV), torch.ones(H, ACT, device=DEV)
    cem = hipets.Engine.cem_params(POP, H, ACT, 2, 3, 0.1, return_mean_elites=True)
    obs = [np.ascontiguousarray(own.s0 + np.float32(0.01 * k)) for k in range(9)]

    def one(k, out):
        if k % 2 == 0:
            eng._call("hipets_rollout", actions=actions, s0=obs[k], pop=POP, horizon=H, num_particles=P,
                      opts=_lib.RolloutOpts(mode=_lib.MODE_FAST, seed=11, stream_id=7), returns=out)
        else:
            eng._call("hipets_plan_cem", p=cem, x0=x0, lower=lower, upper=upper, s0=obs[k], num_particles=P, seed=13, plan_id=7, out=out)

    outs = [torch.empty(POP if k % 2 == 0 else H * ACT, device=DEV) for k in range(9)]
    serial = []
    for k in range(9):
        one(k, outs[k])
        torch.cuda.synchronize()
        serial.append(outs[k].clone())
    assert all(torch.isfinite(t).all() for t in serial)
    assert not torch.equal(serial[0], serial[2]) and not torch.equal(serial[1], serial[3])  # the observation matters
    for pairing in PAIRING_IDS:
        poison(*outs)
        torch.cuda.synchronize()
        for k in range(9):
            with torch.cuda.stream(lanes[pairing][k % 2]):
                one(k, outs[k])
        torch.cuda.synchronize()
        for k in range(9):
            assert same_bits([outs[k]], [serial[k]]), f"{pairing}: call {k} ({'rollout' if k % 2 == 0 else 'plan_cem'}) differs from its serial result"


def test_workspace_growth_on_the_other_stream(own, lanes):
    """a small DEVICE rollout on one stream, at once a larger one on the other: the second call frees and reallocates the workspace
    (state, totals, termination flags) the first one's kernels use.  On a fresh engine, so that the buffers do grow."""
    eng = hipets.Engine(DEV)
    try:
        eng.set_persistent(False)
        eng.set_model(own.spec)
        g = torch.Generator().manual_seed(81)
        small, large = dev(torch.rand(10, 4, ACT, generator=g) * 2 - 1), dev(torch.rand(600, H, ACT, generator=g) * 2 - 1)
        out_s, out_l = torch.empty(10, device=DEV), torch.empty(600, device=DEV)
        s0 = np.ascontiguousarray(own.s0)
        opts = _lib.RolloutOpts(mode=_lib.MODE_DEVICE, seed=11, stream_id=3)

        def run(actions, out):
            pop, horizon, _ = actions.shape
            eng._call("hipets_rollout", actions=actions, s0=s0, pop=pop, horizon=horizon, num_particles=P, opts=opts, returns=out)

        poison(out_s, out_l)
        torch.cuda.synchronize()
        a, b = lanes["side_side"]
        with torch.cuda.stream(a):
            run(small, out_s)
        with torch.cuda.stream(b):
            run(large, out_l)
        torch.cuda.synchronize()
        got = out_s.clone(), out_l.clone()
        run(small, out_s)
        torch.cuda.synchronize()
        run(large, out_l)
        torch.cuda.synchronize()
        assert torch.isfinite(out_s).all() and torch.isfinite(out_l).all()
        assert same_bits([got[0]], [out_s]), "the small rollout differs from its serial result"
        assert same_bits([got[1]], [out_l]), "the large rollout differs from its serial result"
    finally:
        torch.cuda.synchronize()
        eng.close()


def _agent_act(own):
    fn = hipets.HipTrajectoryEvalFn(own.spec, P, engine=own.eng, seed=2, mode="fast")
    cfg = dict(_target_="hipets.CEMOptimizer", num_iterations=2, elite_ratio=0.1, population_size=POP, alpha=0.1, device=DEV, lower_bound="???",
               upper_bound="???", return_mean_elites=True, seed=3)
    agent = hipets.TrajectoryOptimizerAgent(cfg, [-1.0] * ACT, [1.0] * ACT, planning_horizon=H)
    agent.optimizer.optimizer.engine = own.eng  # the optimizer plans on the objective's engine: one fused hipets_plan_cem on this module's own
    agent.set_trajectory_eval_fn(fn)
    return [torch.from_numpy(np.asarray(agent.act(own.s0), dtype=np.float32))]


def _sac_update(own):
    torch.manual_seed(91)
    sac = TinySAC(OBS, ACT, SAC_HID, device=DEV)
    rng = np.random.default_rng(92)
    t = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    memory = FixedMemory([dict(state=t(SAC_B, OBS), action=t(SAC_B, ACT).tanh(), next_state=t(SAC_B, OBS), reward=t(SAC_B),
                               terminated=torch.from_numpy((np.arange(SAC_B) % 4 == 1).astype(np.float32)))])
    up = hipets.SACUpdater(sac, engine=own.eng)
    res = up.update_many([memory], SAC_B, 0, reverse_mask=True, eps=[(dev(t(SAC_B, ACT)), dev(t(SAC_B, ACT)))])
    return [torch.tensor(res[0], dtype=torch.float64)] + [p.detach().clone() for p in sac.params().values()]


def _trainer_steps(own):
    mlp = tr.TinyGaussianMLP(T_E, OBS + ACT, T_HID, OBS, T_L, act="silu")
    ws, bs = tr.random_model(T_E, OBS + ACT, T_HID, OBS, T_L, 11, dtype=torch.float32)
    tr.load_params(mlp, ws, bs)
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((3 * T_B, OBS)).astype(np.float32)
    data = tr.Batch(obs=obs, act=rng.uniform(-1, 1, (3 * T_B, ACT)).astype(np.float32), next_obs=obs + 0.1 * rng.standard_normal(obs.shape).astype(np.float32))
    trainer = hipets.ModelTrainer(tr.TinyDynamicsModel(mlp), optim_lr=1e-2, engine=own.eng)
    losses, _ = trainer.train(tr.TransitionIterator(data, T_B), num_epochs=1, evaluate=False)
    assert trainer._step == 3
    return [torch.tensor(losses, dtype=torch.float64)] + [l.weight.detach().clone() for l in mlp.layers()] + [l.bias.detach().clone() for l in mlp.layers()]


def _policy_sequences(own):
    torch.manual_seed(93)
    ro = hipets.PolicyRollout(own.spec, TinyGaussianPolicy(OBS, ACT, ACTOR_HID).to(DEV), engine=own.eng, only_elite=False, seed=3)
    return list(ro.sequences(start_rows(own.s0, POP, 5), horizon=4, mean_rows=1, stream_id=2, return_states=True))


def _ensemble_predict(own):
    predictor = hipets.EnsemblePredictor(own.spec, engine=own.eng)
    return list(predictor.predict(start_rows(own.s0, B, 6), dev(np.random.default_rng(7).uniform(-1, 1, (B, ACT)).astype(np.float32))))


WRAPPERS = {"TrajectoryOptimizerAgent.act": _agent_act, "SACUpdater.update_many": _sac_update, "ModelTrainer.train": _trainer_steps,
            "PolicyRollout.sequences": _policy_sequences, "EnsemblePredictor.predict": _ensemble_predict}


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_a_public_wrapper_on_a_side_stream_gives_the_default_streams_bits(own, lanes, wrapper):
    default, side = lanes["default_side"]
    want = [t.cpu() for t in WRAPPERS[wrapper](own)]
    torch.cuda.synchronize()
    side.wait_stream(default)
    with torch.cuda.stream(side):
        got = WRAPPERS[wrapper](own)
    default.wait_stream(side)
    got = [t.cpu() for t in got]
    assert len(got) == len(want) and all(bool(torch.isfinite(t).all()) for t in want)
    assert same_bits(got, want), f"{wrapper}: under torch.cuda.stream(side) the result differs from the default stream's"
