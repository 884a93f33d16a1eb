"""TEST INFRASTRUCTURE: restatements of what hipets/policy_rollout.py replaces -- the SAC actor rolled through the dynamics ensemble's
expected next observation -- built from tests/policy_restatement.py (the actor) and tests/ensemble_restatement.py (the model).

  step_f64 / rollout_f64   one step / H steps in float64: GaussianPolicy (the mean action for rows below `mean_rows`, a sample with
                           `eps` for the others), the model input, the mean over the requested members of their mean heads, the delta
                           rule (one_dim_tr_model.py:281-286).  The GPU tests' reference.
  step_f32 / rollout_f32   the same in float32 in torch CPU's op order: actor_f32, model_input, ensemble_f32_torch, torch's mean(dim=0)
                           over the members (gaussian_mlp.py:213-215, basic_ensemble.py:131-136), `pred + obs` and the no-delta
                           columns.  Pinned to the reference's own classes by tests/golden/policy_rollout_cases.npz
                           (tests/make_policy_rollout_golden.py).
  compose_np               the device's stated float32 composition of a next state from the members' means: sequential adds in
                           requested order, one division, the delta rule -- one rounded numpy float32 operation per line.
`rule` everywhere: what says how a prediction becomes an observation -- a hipets.ModelSpec or anything with obs_dim, target_is_delta and
no_delta_list (delta_rule builds one from plain values).
"""
import types

import numpy as np

import ensemble_restatement as er
import policy_restatement as pr


def delta_rule(obs_dim, target_is_delta=True, no_delta_list=()):
    return types.SimpleNamespace(obs_dim=int(obs_dim), target_is_delta=bool(target_is_delta), no_delta_list=list(no_delta_list))


def _next_state(state, pred, rule):
    """one_dim_tr_model.py:281-286 in the dtype of its arguments: the learned-reward column (the last) is dropped"""
    nxt = pred[:, :rule.obs_dim]
    if rule.target_is_delta:
        tmp = nxt + state
        for d in rule.no_delta_list:
            tmp[:, d] = nxt[:, d]
        nxt = tmp
    return nxt


def _actions(actor, w, state, eps_t, mean_rows):
    """rows below `mean_rows`: the mean action; the others: the sample with their row of `eps_t`"""
    act = actor(w, state, sample=False)[0]
    if mean_rows < len(state):
        act = act.copy()
        act[mean_rows:] = actor(w, state[mean_rows:], sample=True, eps=eps_t[mean_rows:])[0]
    return act


def step_f64(case, w, state, eps_t, mean_rows, only_elite, rule):
    """(actions [n, A], next state [n, obs]) in float64 from `state` [n, obs]"""
    state = np.asarray(state, np.float64)
    act = _actions(pr.actor_f64, w, state, eps_t, mean_rows)
    x = er.model_input(case, state, act, f64=True)
    raw = er.raw_heads_f64(case, x, er.member_list(case, only_elite))
    return act, _next_state(state, raw[..., :case["out_dim"]].mean(axis=0), rule)


def step_f32(case, w, state, eps_t, mean_rows, only_elite, rule, member_means=False):
    """the same in float32, torch CPU's op order; `member_means`: also the members' means [n_members, n, out] the step averaged"""
    import torch

    state = np.asarray(state, np.float32)
    act = _actions(pr.actor_f32, w, state, eps_t, mean_rows).astype(np.float32)
    x = er.model_input(case, state, act)
    means = er.ensemble_f32_torch(case, x, only_elite)[0]
    pred = torch.from_numpy(np.ascontiguousarray(means)).mean(dim=0).numpy()
    nxt = _next_state(state, pred, rule)
    return (act, nxt, means) if member_means else (act, nxt)


def _rollout(step, case, w, s0, H, eps, mean_rows, only_elite, rule):
    states, actions = [np.asarray(s0)], []
    for t in range(H):
        a, s = step(case, w, states[-1], None if eps is None else eps[t], mean_rows, only_elite, rule)
        actions.append(a)
        states.append(s)
    return np.stack(actions, axis=1), np.stack(states)


def rollout_f64(case, w, s0, H, eps, mean_rows, only_elite, rule):
    """(actions [n, H, A], states [H + 1, n, obs]) in float64; `eps` [H, n, A] (None with mean_rows == n)"""
    return _rollout(step_f64, case, w, np.asarray(s0, np.float64), H, eps, mean_rows, only_elite, rule)


def rollout_f32(case, w, s0, H, eps, mean_rows, only_elite, rule):
    return _rollout(step_f32, case, w, np.asarray(s0, np.float32), H, eps, mean_rows, only_elite, rule)


def compose_np(state, member_means, rule):
    """the next state [n, obs] as hipets_policy_rollout composes it from `state` [n, obs] and the requested members' means
    [n_members, n, out_dim], float32 throughout"""
    state, means = np.asarray(state, np.float32), np.asarray(member_means, np.float32)
    acc = means[0]
    for m in means[1:]:
        acc = acc + m
    pred = acc / np.float32(len(means))
    pred = pred[:, :rule.obs_dim]
    if not rule.target_is_delta:
        return pred
    nxt = state + pred
    for d in rule.no_delta_list:
        nxt[:, d] = pred[:, d]
    return nxt


def make_actor(name, case, hidden, rows):
    """(weights, eps [rows, A]) of an actor of `hidden` width over `case`'s (obs_dim, act_dim): policy_restatement.make_case, keyed by
    `name` (its per-dimension action scale and bias included: actions reach about -3 .. 3)"""
    w, _, eps = pr.make_case(name, case["obs_dim"], hidden, case["act_dim"], rows=rows)
    return w, eps
