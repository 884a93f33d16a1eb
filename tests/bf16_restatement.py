"""The arithmetic of precision='bf16' (include/hipets.h HIPETS_PREC_BF16), restated on the oracle: for every linear layer both
operands are rounded to bf16 (round-to-nearest-even), products are exact, accumulation is fp32; bias, activation and everything
outside the linear layers stay fp32.  Shared by tests/test_bf16_host.py and tests/test_gpu_bf16.py."""
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pets_oracle as po
from test_gpu_rollout import _random_case


def bf16_rne_bits(x):
    """numpy restatement of csrc/gemm_bf16.hpp bf16_rne_bits: the bf16 nearest-even rounding of finite fp32 values, as fp32."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def members_forward_bf16(m, x):
    """pets_oracle._members_forward with both operands of every matmul rounded to bf16."""
    el = m.active_members
    act = po._ACT[m.activation]
    h = x
    nl = len(m.weights)
    for li in range(nl):
        w = m.weights[li][el, ...]
        b = m.biases[li][el, ...]
        h = h.to(torch.bfloat16).float().matmul(w.to(torch.bfloat16).float()) + b
        if li < nl - 1:
            h = act(h)
    if m.deterministic:
        return h, None
    out = m.out_size
    mean = h[..., :out]
    logvar = h[..., out:]
    logvar = m.max_logvar - F.softplus(m.max_logvar - logvar)
    logvar = m.min_logvar + F.softplus(logvar - m.min_logvar)
    return mean, logvar


def scaled_case(obs, act, pop, P, H, seed=0, gain=2.0, **mkw):
    """test_gpu_rollout._random_case with every weight tensor multiplied by `gain`: the stock synthetic initialiser
    (std 1 / (2 sqrt(in))) has too little gain to tell bf16 from fp32 in one step."""
    om, actions, s0, perms, eps = _random_case(obs, act, pop, P, H, seed=seed, **mkw)
    om = dataclasses.replace(om, weights=[w * gain for w in om.weights])
    return om, actions, s0, perms, eps


def emulated_rollout(monkeypatch, om, actions, s0, P, **kw):
    """po.rollout with the bf16 restatement installed (called directly: the oracle memo never sees it)."""
    with monkeypatch.context() as mp:
        mp.setattr(po, "_members_forward", members_forward_bf16)
        return po.rollout(om, actions, s0, P, **kw)


CFG2 = (17, 6, 500, 20, dict(ensemble_size=5, hid=200))
T1_ATOL = 2e-6   # the fp32 mode's one-step tolerance
T2_REL = 1e-4    # ... and its whole-rollout tolerance: |err| <= 1e-4 max(1, |v|)
