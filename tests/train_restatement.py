"""TEST HELPER (not collected): our own restatement of one GaussianMLP ensemble training step and of the evaluation score,
written out by hand in torch (no autograd, no torch.optim), in float64 or float32:

  loss    GaussianMLP._nll_loss over _default_forward (mbrl/models/gaussian_mlp.py:140-153, 291-305; util/math.py:41-64)
  update  its gradient, then torch.optim.Adam with coupled weight decay (model_trainer.py:63-68), torch's non-fused order
  score   GaussianMLP.eval_score averaged over rows and dims (gaussian_mlp.py:337-361)

plus small stand-ins for the live objects the trainer reads (a GaussianMLP-shaped module in a OneDTransitionRewardModel-shaped
wrapper, and the replay buffer's two iterators), so the GPU tests run where mbrl is not installed.  The stand-in iterators
make their random draws in the same calls as mbrl.util.replay_buffer's; tests/test_trainer_host.py checks that against the
reference where it is available.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

ACTS = ("silu", "relu", "leaky_relu", "tanh", "sigmoid")
_MODULES = {"silu": torch.nn.SiLU, "relu": torch.nn.ReLU, "leaky_relu": torch.nn.LeakyReLU, "tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid}


def act_fwd(name, z, slope=0.01):
    if name == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    if name == "silu":
        return z / (1 + torch.exp(-z))
    if name == "leaky_relu":
        return torch.where(z > 0, z, z * slope)
    if name == "tanh":
        return torch.tanh(z)
    return 1 / (1 + torch.exp(-z))


def act_grad(name, z, slope=0.01):
    if name == "relu":
        return (z > 0).to(z.dtype)
    if name == "silu":
        s = 1 / (1 + torch.exp(-z))
        return s * (1 + z * (1 - s))
    if name == "leaky_relu":
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if name == "tanh":
        return 1 - torch.tanh(z) ** 2
    s = 1 / (1 + torch.exp(-z))
    return s * (1 - s)


def softplus(x):
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20))))


def softplus_grad(x):
    return torch.where(x > 20, torch.ones_like(x), 1 / (1 + torch.exp(-torch.clamp(x, max=20))))


def forward(ws, bs, x, act, slope=0.01):
    """x [E, B, in] -> (list of layer inputs, list of hidden pre-activations, raw output [E, B, 2 out])."""
    inputs, zs = [x], []
    h = x
    for li in range(len(ws)):
        z = h @ ws[li] + bs[li]
        if li < len(ws) - 1:
            zs.append(z)
            h = act_fwd(act, z, slope)
            inputs.append(h)
        else:
            return inputs, zs, z


def nll_step(ws, bs, x, y, min_lv, max_lv, act, slope=0.01):
    """Per-member loss [E], raw gradients (dws, dbs) of the summed loss, for x [E, B, in], y [E, B, out]."""
    inputs, zs, o = forward(ws, bs, x, act, slope)
    out = y.shape[-1]
    mean, raw = o[..., :out], o[..., out:]
    u = max_lv - raw
    lv1 = max_lv - softplus(u)
    w = lv1 - min_lv
    lv = min_lv + softplus(w)
    d = mean - y
    iv = torch.exp(-lv)
    l2iv = d * d * iv
    n = y.shape[1] * out
    loss = (l2iv + lv).sum((1, 2)) / n
    dmean = 2 * d * iv / n
    dlv = (1 - l2iv) / n
    draw = dlv * softplus_grad(w) * softplus_grad(u)
    dz = torch.cat([dmean, draw], dim=-1)
    dws, dbs = [None] * len(ws), [None] * len(ws)
    for li in range(len(ws) - 1, -1, -1):
        dws[li] = inputs[li].transpose(1, 2) @ dz
        dbs[li] = dz.sum(1, keepdim=True)
        if li > 0:
            dz = (dz @ ws[li].transpose(1, 2)) * act_grad(act, zs[li - 1], slope)
    return loss, dws, dbs


def adam_(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """torch.optim.Adam (_single_tensor_adam, no amsgrad / maximize), in place on p, m, v; step = the step count after it."""
    b1, b2 = betas
    g = g.add(p, alpha=weight_decay) if weight_decay != 0 else g
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))


def train_step(ws, bs, ms, vs, x, y, min_lv, max_lv, act, step, lr, weight_decay, eps=1e-8, slope=0.01):
    """One Model.update in place on ws / bs (lists of [E, ., .]) and the Adam moments ms / vs = ([per-layer w], [per-layer b]).
    Returns (per-member loss [E], per-member sum of squared raw gradients [E])."""
    loss, dws, dbs = nll_step(ws, bs, x, y, min_lv, max_lv, act, slope)
    gsq = sum((g * g).sum((1, 2)) for g in dws + dbs)
    for li in range(len(ws)):
        adam_(ws[li], dws[li], ms[0][li], vs[0][li], step, lr, eps=eps, weight_decay=weight_decay)
        adam_(bs[li], dbs[li], ms[1][li], vs[1][li], step, lr, eps=eps, weight_decay=weight_decay)
    return loss, gsq


def eval_score(ws, bs, x, y, act, slope=0.01):
    """Per-member mean over rows and dims of (mean - y)^2, x [N, in], y [N, out]."""
    _, _, o = forward(ws, bs, x.unsqueeze(0).expand(ws[0].shape[0], -1, -1), act, slope)
    out = y.shape[-1]
    return ((o[..., :out] - y) ** 2).mean((1, 2))


def random_model(E, in_dim, hid, out, n_layers, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    dims = [in_dim] + [hid] * (n_layers - 1) + [2 * out]
    ws = [torch.randn(E, dims[i], dims[i + 1], generator=g, dtype=dtype) / (2 * dims[i] ** 0.5) for i in range(n_layers)]
    bs = [torch.randn(E, 1, dims[i + 1], generator=g, dtype=dtype) * 0.1 for i in range(n_layers)]
    return ws, bs


# ---- stand-ins for the live objects ------------------------------------------------------------------------------------
class EnsembleLinear(torch.nn.Module):
    def __init__(self, E, n_in, n_out):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(E, n_in, n_out))
        self.bias = torch.nn.Parameter(torch.zeros(E, 1, n_out))
        self.use_bias = True

    def forward(self, x):
        return x.matmul(self.weight) + self.bias


class TinyGaussianMLP(torch.nn.Module):
    """The attributes hipets.ModelTrainer reads from a GaussianMLP (same parameter registration order)."""

    def __init__(self, E, in_dim, hid, out, n_layers, act="silu", deterministic=False, learn_logvar_bounds=False):
        super().__init__()
        self.num_members = E
        self.deterministic = deterministic
        self.hidden_layers = torch.nn.Sequential(*[torch.nn.Sequential(EnsembleLinear(E, in_dim if i == 0 else hid, hid), _MODULES[act]())
                                                   for i in range(n_layers - 1)])
        self.mean_and_logvar = EnsembleLinear(E, hid, out if deterministic else 2 * out)
        if not deterministic:
            self.min_logvar = torch.nn.Parameter(-10 * torch.ones(1, out), requires_grad=learn_logvar_bounds)
            self.max_logvar = torch.nn.Parameter(0.5 * torch.ones(1, out), requires_grad=learn_logvar_bounds)
        self.elite_models = None

    def layers(self):
        return [l[0] for l in self.hidden_layers] + [self.mean_and_logvar]

    def set_elite(self, elite):
        self.elite_models = list(elite)


class TinyDynamicsModel(torch.nn.Module):
    """A OneDTransitionRewardModel-shaped wrapper: delta targets, no normaliser, no learned rewards."""

    def __init__(self, mlp, num_elites=None):
        super().__init__()
        self.model = mlp
        self.num_elites = num_elites or mlp.num_members
        self.device = torch.device("cpu")

    def _process_batch(self, batch):
        obs = torch.as_tensor(batch.obs)
        act = torch.as_tensor(batch.act)
        nobs = torch.as_tensor(batch.next_obs)
        return torch.cat([obs, act], dim=obs.ndim - 1).float(), (nobs - obs).float()

    def set_elite(self, elite):
        self.model.set_elite(elite)


class Batch(SimpleNamespace):
    def __len__(self):
        return len(self.obs)

    def __getitem__(self, item):
        return Batch(obs=self.obs[item], act=self.act[item], next_obs=self.next_obs[item])


class TransitionIterator:
    """The replay buffer's iterator protocol: ``__iter__`` redraws ``_order`` with ``rng.permutation`` when shuffling."""

    def __init__(self, transitions, batch_size, shuffle_each_epoch=False, rng=None):
        self.transitions = transitions
        self.num_stored = len(transitions)
        self._order = np.arange(self.num_stored)
        self.batch_size = batch_size
        self._current_batch = 0
        self._shuffle_each_epoch = shuffle_each_epoch
        self._rng = rng if rng is not None else np.random.default_rng()

    def __iter__(self):
        self._current_batch = 0
        if self._shuffle_each_epoch:
            self._order = self._rng.permutation(self.num_stored)
        return self

    def __next__(self):
        start = self._current_batch * self.batch_size
        if start >= self.num_stored:
            raise StopIteration
        self._current_batch += 1
        return self.transitions[self._order[start:min(start + self.batch_size, self.num_stored)]]

    def __len__(self):
        return (self.num_stored - 1) // self.batch_size + 1


class BootstrapIterator(TransitionIterator):
    def __init__(self, transitions, batch_size, ensemble_size, shuffle_each_epoch=False, permute_indices=True, rng=None, member_indices=None):
        super().__init__(transitions, batch_size, shuffle_each_epoch, rng)
        self._ensemble_size = ensemble_size
        self._bootstrap_iter = ensemble_size > 1
        if member_indices is not None:
            self.member_indices = np.asarray(member_indices)
        elif permute_indices:
            self.member_indices = np.stack([self._rng.permutation(self.num_stored) for _ in range(ensemble_size)])
        else:
            self.member_indices = self._rng.choice(self.num_stored, size=(ensemble_size, self.num_stored), replace=True)

    def __next__(self):
        if not self._bootstrap_iter:
            return super().__next__()
        start = self._current_batch * self.batch_size
        if start >= self.num_stored:
            raise StopIteration
        self._current_batch += 1
        sel = self._order[start:min(start + self.batch_size, self.num_stored)]
        parts = [self.transitions[m[sel]] for m in self.member_indices]
        return Batch(obs=np.stack([p.obs for p in parts]), act=np.stack([p.act for p in parts]),
                     next_obs=np.stack([p.next_obs for p in parts]))

    def toggle_bootstrap(self):
        if self._ensemble_size > 1:
            self._bootstrap_iter = not self._bootstrap_iter

    @property
    def ensemble_size(self):
        return self._ensemble_size


def load_params(mlp, ws, bs):
    with torch.no_grad():
        for lin, w, b in zip(mlp.layers(), ws, bs):
            lin.weight.copy_(torch.as_tensor(w))
            lin.bias.copy_(torch.as_tensor(b))
