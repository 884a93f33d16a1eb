"""The stream contract of include/hipets.h as a table: every symbol of ``hipets._lib.SYMBOLS`` that takes a ``stream`` belongs to exactly
one class below (tests/test_stream_contract_host.py checks the partition without a GPU), and ``CHAINS`` are the dependency chains
tests/test_gpu_streams.py runs across two streams -- generated from here, there is no second list.

A chain is a tuple of steps; a step is a symbol, or ``symbol#tag`` where a chain calls one symbol twice.  Step k runs on stream
k % 2 of the pairing, so every step but the last is a PRODUCER before a stream switch and every step but the first a CONSUMER after
one: step k + 1 reads device memory step k writes (the wiring is in test_gpu_streams.py, one function per step)."""

# they take part in the ordering and synchronise `stream` before they return (they read HOST staging and caller tensors that may go away)
SYNCHRONISING = ("hipets_set_model", "hipets_set_model_columns", "hipets_planet_set_model", "hipets_ensemble_set")

# one kernel on the caller's buffers, no workspace: they neither wait for another call nor are waited for (bodies read in
# csrc/plan.hip, csrc/rollout.hip, csrc/policy.hip: of the engine they use host fields only -- the model's sizes, the particle
# reduction, the LDS limit)
LAUNCH_ONLY = ("hipets_cem_sample", "hipets_cem_refit", "hipets_cem_refit_elites", "hipets_gather_rows", "hipets_mppi_sample",
               "hipets_mppi_update", "hipets_icem_sample", "hipets_icem_shift", "hipets_particle_reduce", "hipets_fast_schedule",
               "hipets_fast_normals", "hipets_device_perms", "hipets_policy_normals")

# the sharded plans: tests/test_gpu_dist.py and tests/test_gpu_sharded_world.py
NEEDS_COMMUNICATOR = ("hipets_plan_cem_sharded", "hipets_plan_mppi_sharded", "hipets_plan_icem_sharded")

CHAINS = {
    # actor, model and value: W -> actions -> (next_obs, rewards) -> a critic whose output biases ARE two of those rewards -> q -> the
    # ensemble's statistics of rows made of q -> penalised rewards and halts -> discounted returns -> returns of their row totals
    # -> an actor whose action bias IS those returns -> that actor rolled through the ensemble
    "actor_model_value": ("hipets_policy_set", "hipets_policy_act", "hipets_step", "hipets_critic_set", "hipets_critic_q",
                          "hipets_ensemble_predict", "hipets_uncertainty_penalty", "hipets_discounted_returns", "hipets_trajectory_returns",
                          "hipets_policy_set#returns", "hipets_policy_rollout#actor"),
    # rollouts and plans; a chain stages at most four host observations (the pinned ring has four slots: a fifth blocks the host)
    "policy_rollout_cem_fast": ("hipets_policy_rollout", "hipets_rollout", "hipets_plan_cem", "hipets_rollout#plan"),
    "mppi_icem_device": ("hipets_rollout", "hipets_plan_mppi", "hipets_rollout#plan", "hipets_plan_icem"),
    "batched_plans_fast": ("hipets_plan_icem", "hipets_plan_cem_batched", "hipets_plan_mppi_batched", "hipets_rollout#batched"),
    "batched_icem_device": ("hipets_plan_mppi_batched", "hipets_plan_icem_batched", "hipets_rollout#batched", "hipets_plan_mppi"),
    # MBPO: model step -> ring -> gathered batch -> SAC update -> its taps -> staging area -> gathered again
    "mbpo": ("hipets_step", "hipets_ring_compact_transitions", "hipets_replay_gather", "hipets_sac_update", "hipets_sac_forward_taps",
             "hipets_compact_transitions", "hipets_replay_gather#staging"),
    # trainer: the weights updated in place, and targets that are the previous evaluation's row scores
    "trainer": ("hipets_train_steps", "hipets_train_eval", "hipets_train_steps_loss", "hipets_train_eval_loss", "hipets_train_steps#scores"),
    # PlaNet: plan -> rollout of the plan -> batched plans from it -> rollout -> plan
    "planet": ("hipets_plan_planet_cem", "hipets_planet_rollout", "hipets_plan_planet_cem_batched", "hipets_plan_planet_mppi_batched",
               "hipets_plan_planet_icem_batched", "hipets_planet_rollout#batched", "hipets_plan_planet_cem#returns"),
}

# (name, first stream, second stream): both fresh side streams, and the default stream with a side stream
PAIRINGS = (("side_side", "side", "side"), ("default_side", "default", "side"))


def symbol_of(step: str) -> str:
    return step.split("#")[0]


def roles():
    """{symbol: {"producer": [chains], "consumer": [chains]}} of the symbols in CHAINS"""
    out = {}
    for name, steps in CHAINS.items():
        for k, step in enumerate(steps):
            r = out.setdefault(symbol_of(step), {"producer": [], "consumer": []})
            if k < len(steps) - 1 and name not in r["producer"]:
                r["producer"].append(name)
            if k > 0 and name not in r["consumer"]:
                r["consumer"].append(name)
    return out


# every other stream-taking symbol takes part in the contract: where it produces before a stream switch, where it consumes after one
ORDERED = roles()


def stream_symbols(symbols) -> list:
    """the names in ``hipets._lib.SYMBOLS`` whose parameters include ``stream``"""
    return [name for name, (_, params) in symbols.items() if any(p == "stream" for p, _ in params)]
