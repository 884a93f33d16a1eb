"""TEST HELPER (not collected): our own restatement of one GaussianMLP ensemble training step and of the evaluation score,
written out by hand in torch (no autograd, no torch.optim), in float64 or float32:

  loss    GaussianMLP._nll_loss over _default_forward (mbrl/models/gaussian_mlp.py:140-153, 291-305; util/math.py:41-64)
  update  its gradient, then torch.optim.Adam with coupled weight decay (model_trainer.py:63-68), torch's non-fused order
  score   GaussianMLP.eval_score averaged over rows and dims (gaussian_mlp.py:337-361)

plus small stand-ins for the live objects the trainer reads (a GaussianMLP-shaped module in a OneDTransitionRewardModel-shaped
wrapper, and the replay buffer's two iterators), so the GPU tests run where mbrl is not installed.  The stand-in iterators
make their random draws in the same calls as mbrl.util.replay_buffer's; tests/test_trainer_host.py checks that against the
reference where it is available.  At the end: what the GPU trainer tests share (run_steps: the same steps on the GPU and in
both restatements; check: the self-calibrated rule).
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


# ---- shared by the GPU trainer tests (tests/test_gpu_trainer.py, tests/test_gpu_trainer_edges.py) ------------------------
LR, WD = 1e-3, 1e-5


def dist(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def check(hip, f32, f64, what, f32_others=()):
    """The suite's self-calibrated rule: the HIP result may lie at most 4x as far from the float64 restatement as the float32
    restatement does, plus a 1e-7 floor.  Prints the distances.  f32_others = further float32 restatements in other summation
    orders: where the float32 orders are themselves further apart than the rule allows (one's distance from float64 is more than
    4x another's + 1e-7), float32 rounding decides the quantity and the yardstick is the largest of their distances."""
    d_hip, d_32 = dist(hip, f64), dist(f32, f64)
    d_all = [d_32] + [dist(t, f64) for t in f32_others]
    print(f"{what}: |hip - f64| = {d_hip:.3e}, |f32 - f64| = {d_32:.3e}" + "".join(f", other order {d:.3e}" for d in d_all[1:]))
    if max(d_all) > 4 * min(d_all) + 1e-7:
        d_32 = max(d_all)
    assert d_hip <= 4 * d_32 + 1e-7, f"{what}: |hip - f64| = {d_hip:.3e} > 4 |f32 - f64| = {4 * d_32:.3e} + 1e-7"


def mirrored(ws, bs):
    """The same network with its input features and hidden units in reverse order (apply twice to get the original back): with
    mirrored inputs, every contraction of a step sums the same terms in the other order."""
    L = len(ws)
    ws = [w.flip(1, 2) if l < L - 1 else w.flip(1) for l, w in enumerate(ws)]
    bs = [b.flip(2) if l < L - 1 else b for l, b in enumerate(bs)]
    return ws, bs


def fresh_state(ws, bs, dtype, device):
    """(weights, biases, exp_avg, exp_avg_sq) copies of a model in ``dtype`` on ``device``, the moments zero."""
    w = [t.to(device, dtype).clone() for t in ws]
    b = [t.to(device, dtype).clone() for t in bs]
    return w, b, ([torch.zeros_like(t) for t in w], [torch.zeros_like(t) for t in b]), ([torch.zeros_like(t) for t in w], [torch.zeros_like(t) for t in b])


def run_steps(engine, E, B, in_dim, hid, out, n_layers, act, n_steps, N=None, seed=0, steps_per_launch=0, ragged_last=False, *,
              bounds=None, edit_params=None, rows=None, edit_idx=None, step0=0, calls=None, restate=True, f32_orders=False, device="cuda:0"):
    """n_steps steps on the GPU and in the float32 / float64 restatements; returns the three final states and per-step losses
    ({"hip" | "f32" | "f64": (w, b, m, v, loss [S, E], grad_sq [S, E])}) and, under "inputs", what the run was fed.

    bounds(lo, hi) edits the logvar bounds [1, out] in place; edit_params(ws, bs) the float64 initial parameters; rows is an
    explicit per-step row count (n_steps = len(rows)); edit_idx(idx) edits the int32 schedule [S, E, B] in place (an index
    outside [0, N) stands for a row of zeros, in the restatement too); step0 = Adam steps taken before; calls = step counts
    of consecutive train_steps calls the run is split into; restate=False skips the CPU restatements; f32_orders adds two float32
    restatements of the same sums in other orders: "f32r" with every minibatch's rows reversed (the contractions over the batch),
    "f32m" with the rows reversed and the network mirrored (every contraction)."""
    g = torch.Generator().manual_seed(seed + 1)
    N = N or max(3 * B, 64)
    x = torch.randn(N, in_dim, generator=g, dtype=torch.float64)
    y = torch.randn(N, out, generator=g, dtype=torch.float64) * 0.3
    ws, bs = random_model(E, in_dim, hid, out, n_layers, seed)
    if edit_params is not None:
        edit_params(ws, bs)
    lo, hi = -10 * torch.ones(1, out, dtype=torch.float64), 0.5 * torch.ones(1, out, dtype=torch.float64)
    lo[0, 0], hi[0, 0] = -2.0, -1.0  # one column whose bounds are active
    if bounds is not None:
        bounds(lo, hi)
    if rows is not None:
        n_steps = len(rows)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:B] for _ in range(E)]) for _ in range(n_steps)]).to(torch.int32)
    if edit_idx is not None:
        edit_idx(idx)
    if rows is None:
        rows = torch.full((n_steps,), B, dtype=torch.int32)
        if ragged_last:
            rows[-1] = max(1, B // 3)
    rows = torch.as_tensor(rows, dtype=torch.int32)
    res = {"inputs": dict(x=x, y=y, ws=ws, bs=bs, lo=lo, hi=hi, idx=idx, rows=rows)}
    # dataset row N of the restatement is the row of zeros an outside index reads
    sel_all = torch.where((idx >= 0) & (idx < N), idx.long(), torch.full_like(idx, N, dtype=torch.int64))
    x0, y0 = torch.cat([x, torch.zeros(1, in_dim, dtype=x.dtype)]), torch.cat([y, torch.zeros(1, out, dtype=y.dtype)])
    kinds = (("f64", torch.float64), ("f32", torch.float32)) + ((("f32r", torch.float32), ("f32m", torch.float32)) if f32_orders else ())
    for name, dtype in kinds if restate else ():
        w, b, m, v = fresh_state(*(mirrored(ws, bs) if name == "f32m" else (ws, bs)), dtype, "cpu")
        xd, yd = (x0.flip(1) if name == "f32m" else x0).to(dtype), y0.to(dtype)
        losses, gsqs = [], []
        for s in range(n_steps):
            sel = sel_all[s, :, :rows[s]]
            if name in ("f32r", "f32m"):
                sel = sel.flip(-1)
            l, gq = train_step(w, b, m, v, xd[sel], yd[sel], lo.to(dtype), hi.to(dtype), act, step0 + s + 1, LR, WD)
            losses.append(l)
            gsqs.append(gq)
        if name == "f32m":
            (w, b), m, v = mirrored(w, b), mirrored(*m), mirrored(*v)
        res[name] = (w, b, m, v, torch.stack(losses), torch.stack(gsqs))
    w, b, m, v = fresh_state(ws, bs, torch.float32, device)
    lo_d, hi_d = lo.float().reshape(-1).to(device), hi.float().reshape(-1).to(device)
    x_d, y_d, idx_d, rows_d = x.float().to(device), y.float().to(device), idx.to(device), rows.to(device)
    loss, gsq, done = [], [], 0
    for n in calls or [n_steps]:
        l, gq = engine.train_steps(w, b, m, v, lo_d, hi_d, x_d, y_d, idx_d[done:done + n].contiguous(), rows_d[done:done + n].contiguous(),
                                   step0 + done, lr=LR, weight_decay=WD, activation=act, steps_per_launch=steps_per_launch)
        loss.append(l)
        gsq.append(gq)
        done += n
    assert done == n_steps
    if device != "cpu":
        torch.cuda.synchronize()
    res["hip"] = (w, b, m, v, torch.cat(loss), torch.cat(gsq))
    return res
