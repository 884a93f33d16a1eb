"""Reward tables with grouped terms (hipets.RewardTerms with level / op / 'group' / 'const'), shared by
tests/test_reward_groups_host.py and tests/test_gpu_reward_groups.py: the three shipped closed-form rewards restated in the op
order of the enum forms in csrc/closed_forms.hpp reward_eval (so that the kernel's table machine repeats the enum's fp32 ops one
for one), and a custom form that uses every construct.  Not a test module."""
import torch

from hipets import RewardTerm as T
from hipets import RewardTerms


def cartpole_pets_terms():
    """HIPETS_REW_CARTPOLE_PETS: e0 = (s0 - 0.6 sin s1) - 0, e1 = (-0.6 cos s1) - 0.6, exp(-(e0^2 + e1^2) / 0.36) + (-0.01 * a0^2).
    a - b == a + (-b) and -(x) / c == x / (-c) bit for bit, 0 + x == x (up to the sign of a zero)."""
    return RewardTerms([
        T("linear", 0, level=2), T("sin", 1, w=-0.6, level=2), T("square", 0, source="group", level=1),  # e0^2
        T("cos", 1, w=-0.6, level=2), T("square", 0, c=0.6, source="group", level=1),                    # + e1^2
        T("linear", 0, w=-1.0, c=0.6 * 0.6, source="const", level=1, op="div"), T("exp", 0, source="group"),
        T("square", 0, source="act", level=1), T("linear", 0, w=-0.01, source="group")])


def halfcheetah_terms(act_dim=6):
    """HIPETS_REW_HALFCHEETAH: run = s0 - 0.0 * (s2 * s2); sq = sum a^2 from 0 in dim order; run + (-0.1 * sq).  The -0.0 weight
    keeps the enum's 0 * s2^2 term, NaN for a non-finite s2."""
    return RewardTerms([T("linear", 0), T("square", 2, w=-0.0)] + [T("square", i, source="act", level=1) for i in range(act_dim)]
                       + [T("linear", 0, w=-0.1, source="group")])


PUSHER_GOAL = (0.45, -0.05, -0.323)


def pusher_terms(act_dim=7):
    """HIPETS_REW_PUSHER: -((0.5 * tip_obj + 1.25 * obj_goal) + 0.1 * sq): three sums at level 2, their weighted sum at level 1,
    the sign at level 0 -- 17 entries.  |g - s| == |s - g| bit for bit."""
    return RewardTerms([T("abs", 14 + k, j=17 + k, level=2) for k in range(3)] + [T("linear", 0, w=0.5, source="group", level=1)]
                       + [T("abs", 17 + k, c=PUSHER_GOAL[k], level=2) for k in range(3)] + [T("linear", 0, w=1.25, source="group", level=1)]
                       + [T("square", i, source="act", level=2) for i in range(act_dim)] + [T("linear", 0, w=0.1, source="group", level=1)]
                       + [T("linear", 0, w=-1.0, source="group")])


# ---- a custom form with every construct (obs >= 8, act 3) -------------------------------------------------------------------------
#   0.25 + exp(-((s0 - 0.4 sin(s1 - s2) - 1)^2 + (0.4 cos(s1 - 0.3) - 0.2)^2) / 0.5)     three levels, div by a const, exp; sin with j, cos with c
#        - 0.3 sqrt((s3 - s4)^2 + s5^2 + 0.01)                                           sqrt of a sum of squares plus a constant
#        + 0.5 s6 cos(s7)                                                                mul
#        - 0.05 sum a^2
CUSTOM_ACT = 3
CUSTOM_ENTRIES = [
    T("linear", 0, level=2), T("sin", 1, w=-0.4, j=2, level=2), T("square", 0, c=1.0, source="group", level=1),
    T("cos", 1, w=0.4, c=0.3, level=2), T("square", 0, c=0.2, source="group", level=1),
    T("linear", 0, w=-1.0, c=0.5, source="const", level=1, op="div"), T("exp", 0, source="group"),
    T("square", 3, j=4, level=1), T("square", 5, level=1), T("linear", 0, c=0.01, source="const", level=1), T("sqrt", 0, w=-0.3, source="group"),
    T("linear", 6, level=1), T("cos", 7, level=1, op="mul"), T("linear", 0, w=0.5, source="group"),
] + [T("square", i, source="act", level=1) for i in range(CUSTOM_ACT)] + [T("linear", 0, w=-0.05, source="group")]
CUSTOM_BIAS = 0.25


def custom_terms(alive_bonus=0.0, termination_fn=None):
    return RewardTerms(CUSTOM_ENTRIES, bias=CUSTOM_BIAS, alive_bonus=alive_bonus, termination_fn=termination_fn)


def custom_formula_f64(act, nobs):
    """the custom form written out by hand in float64 -> (value [B], sum of the magnitudes of what is added up [B])"""
    s, a = nobs.double(), act.double()
    d2 = (s[:, 0] - 0.4 * torch.sin(s[:, 1] - s[:, 2]) - 1.0) ** 2 + (0.4 * torch.cos(s[:, 1] - 0.3) - 0.2) ** 2
    parts = [torch.full_like(d2, CUSTOM_BIAS), torch.exp(-d2 / 0.5), -0.3 * torch.sqrt((s[:, 3] - s[:, 4]) ** 2 + s[:, 5] ** 2 + 0.01),
             0.5 * s[:, 6] * torch.cos(s[:, 7]), -0.05 * (a ** 2).sum(dim=1)]
    return sum(parts), sum(p.abs() for p in parts)
