"""The reference of the posterior-update tests: a stand-in with PlaNetModel's attribute names (mbrl/models/planet.py:196-272, no mbrl
import) and a plain torch restatement of ``update_posterior`` (planet.py:592-641 -> :309-347) in any dtype -- float64 is the reference,
float32 what tests/test_planet_posterior_host.py holds against it."""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from planet_f64 import CONF, T1, t1_excess  # noqa: F401

CONF_IMAGE = (3, 64, 64)
CONF_CONVS = ((32, 4, 2), (64, 4, 2), (128, 4, 2), (256, 4, 2))  # conf/dynamics_model/planet.yaml: (C_out, kernel, stride); encoding 1024
SMALL_HEAD = (3, 2, 5, 7)

# (image, [(C_out, kernel, stride), ...], encoding size or None for nn.Identity): K = C_in k k of every residue mod 4 (9, 18, 27, 48), 17 = one
# past a 16 chunk; C_out 1, 5, 16, 17, 33; kernels 1..5, one of them the whole remaining image; strides 1, 2, 3, one dropping trailing
# pixels; 1, 9, 16 and 17 output positions per image; 1, 2 and 4 layers; K = 297 and 425 take the K-split path (>= 16 k-blocks)
ENCODER_EDGES = [
    ((1, 8, 8), [(5, 3, 1)], 7),
    ((2, 9, 11), [(16, 3, 2), (17, 2, 1)], None),
    ((3, 11, 11), [(33, 3, 3), (1, 3, 1)], 6),
    ((3, 10, 10), [(16, 4, 2)], None),
    ((2, 3, 19), [(5, 3, 1)], 16),
    ((3, 13, 12), [(17, 1, 1), (8, 5, 2), (16, 2, 1), (5, 3, 1)], None),
    ((1, 8, 9), [(17, 1, 1), (4, 1, 1)], 5),
]
ENCODER_CASES = [(image, tuple(convs), enc, SMALL_HEAD) for image, convs, enc in ENCODER_EDGES] + [(CONF_IMAGE, CONF_CONVS, None, CONF)]
STEP_CASES = [((3, 8, 8), ((8, 4, 2),), None, dims) for dims in ((1, 1, 1, 1), (17, 15, 33, 65), (7, 2, 22, 19))] + [(CONF_IMAGE, CONF_CONVS, None, CONF)]


def case_id(case):
    image, convs, enc, dims = case
    return "x".join(map(str, image)) + "_" + "-".join("c%dk%ds%d" % c for c in convs) + f"_fc{enc}_" + "x".join(map(str, dims))


class StandIn(nn.Module):
    """Xavier-uniform weights (gain 1), biases U(-0.1, 0.1), from a seeded generator."""

    def __init__(self, image, convs, enc, dims, seed=0):
        super().__init__()
        L, A, Hb, Fh = dims
        self.obs_shape, self.latent_state_size, self.action_size, self.belief_size, self.min_std = image, L, A, Hb, 0.1
        self.encoder = nn.Module()
        layers, (C, H, W) = [], image
        for c_out, k, s in convs:
            layers.append(nn.Sequential(nn.Conv2d(C, c_out, k, stride=s), nn.ReLU()))
            C, H, W = c_out, (H - k) // s + 1, (W - k) // s + 1
        self.encoder.convs = nn.ModuleList(layers)
        self.encoder.fc = nn.Identity() if enc is None else nn.Linear(C * H * W, enc)
        enc = C * H * W if enc is None else enc
        self.belief_model = nn.Module()
        self.belief_model.embedding_layer = nn.Sequential(nn.Linear(L + A, Hb), nn.ReLU())
        self.belief_model.rnn = nn.GRUCell(Hb, Hb)
        self.prior_transition_model = nn.Sequential(nn.Linear(Hb, Fh), nn.ReLU(), nn.Linear(Fh, 2 * L))
        self.posterior_transition_model = nn.Sequential(nn.Linear(enc + Hb, Fh), nn.ReLU(), nn.Linear(Fh, 2 * L))
        self.reward_model = nn.Sequential(nn.Linear(Hb + L, Fh), nn.ReLU(), nn.Linear(Fh, Fh), nn.ReLU(), nn.Linear(Fh, 1))
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                if p.ndim >= 2:
                    nn.init.xavier_uniform_(p, gain=1.0, generator=g)
                else:
                    p.uniform_(-0.1, 0.1, generator=g)
        self.rng = torch.Generator().manual_seed(seed + 1)
        self._current_posterior_sample = self._current_belief = None

    def reset_posterior(self):
        self._current_posterior_sample = self._current_belief = None


@functools.lru_cache(maxsize=None)
def make_case(case, n_env):
    """(model, uint8 images [n_env, C, H, W], actions [2, n_env, A], eps [3, n_env, L]) of a case, made once and shared"""
    image, convs, enc, dims = case
    model = StandIn(image, convs, enc, dims, seed=sum(dims) + len(convs))
    g = torch.Generator().manual_seed(n_env)
    obs = torch.randint(0, 256, (3, n_env) + tuple(image), generator=g, dtype=torch.uint8)
    actions = torch.rand(2, n_env, dims[1], generator=g) * 2 - 1
    eps = torch.randn(3, n_env, dims[0], generator=g)
    return model, obs, actions, eps


def encode(model, obs, dtype=torch.float64):
    """Conv2dEncoder.forward on the normalised pixels (planet.py:274-275, util.py:152-157)"""
    x = obs.to(dtype) / 256.0 - 0.5
    for layer in model.encoder.convs:
        x = F.relu(F.conv2d(x, layer[0].weight.to(dtype), layer[0].bias.to(dtype), stride=layer[0].stride))
    h = x.reshape(x.shape[0], -1)
    fc = model.encoder.fc
    return h if isinstance(fc, nn.Identity) else F.linear(h, fc.weight.to(dtype), fc.bias.to(dtype))


def step(model, obs, action, latent, belief, eps, dtype=torch.float64):
    """_forward_transition_models(only_posterior=True) (planet.py:309-347): (next latent, next belief); eps None = the posterior mean"""
    lin = lambda m, x: F.linear(x, m.weight.to(dtype), m.bias.to(dtype))  # noqa: E731
    bm, post, L, Hb = model.belief_model, model.posterior_transition_model, model.latent_state_size, model.belief_size
    emb = F.relu(lin(bm.embedding_layer[0], torch.cat([latent.to(dtype), action.to(dtype)], dim=1)))
    gi = F.linear(emb, bm.rnn.weight_ih.to(dtype), bm.rnn.bias_ih.to(dtype))
    gh = F.linear(belief.to(dtype), bm.rnn.weight_hh.to(dtype), bm.rnn.bias_hh.to(dtype))
    r = torch.sigmoid(gi[:, :Hb] + gh[:, :Hb])
    z = torch.sigmoid(gi[:, Hb:2 * Hb] + gh[:, Hb:2 * Hb])
    n = torch.tanh(gi[:, 2 * Hb:] + r * gh[:, 2 * Hb:])
    nb = (1 - z) * n + z * belief.to(dtype)
    params = lin(post[2], F.relu(lin(post[0], torch.cat([nb, encode(model, obs, dtype)], dim=1))))
    mean, std = params[:, :L], F.softplus(params[:, L:]) + model.min_std
    return (mean if eps is None else mean + std * eps.to(dtype)), nb


def episode(case, n_env, sample, dtype=torch.float64, states=None):
    """reset, update(action=None), two update(action): [(latent, belief)] per step.  ``states``: the (latent, belief) each step starts
    from (the device's own previous outputs, so that errors do not compound); None: the evaluation's own."""
    model, obs, actions, eps = make_case(case, n_env)
    L, A, Hb, _ = case[3]
    out, latent, belief = [], torch.zeros(n_env, L), torch.zeros(n_env, Hb)
    for t in range(3):
        if states is not None and t > 0:
            latent, belief = states[t - 1]
        action = torch.zeros(n_env, A) if t == 0 else actions[t - 1]
        latent, belief = step(model, obs[t], action, latent, belief, eps[t] if sample else None, dtype)
        out.append((latent, belief))
    return out
