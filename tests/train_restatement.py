"""TEST HELPER (not collected): our own restatement of one GaussianMLP ensemble training step and of the evaluation score,
written out by hand in torch (no autograd, no torch.optim), in float64 or float32:

  loss    GaussianMLP._nll_loss over _default_forward (mbrl/models/gaussian_mlp.py:140-153, 291-305; util/math.py:41-64), with
          shared or per-member logvar bounds, or GaussianMLP._mse_loss of a deterministic model (gaussian_mlp.py:283-289)
  update  its gradient (times grad_scale, the 1 / E of BasicEnsemble.loss), then torch.optim.Adam with coupled weight decay
          (model_trainer.py:63-68), torch's non-fused order
  score   GaussianMLP.eval_score averaged over rows and dims (gaussian_mlp.py:337-361)

The defaults (kind "nll", shared bounds, grad_scale 1, torch's matmul) are the update hipets.ModelTrainer trained first; the others
are what it trains with ``extended=True``.  Plus small stand-ins for the live objects the trainer reads (a GaussianMLP-shaped
module in a OneDTransitionRewardModel-shaped wrapper, the replay buffer's two iterators, and a CPU engine), so the GPU tests run
where mbrl is not installed; tests/train_loss_restatement.py adds the BasicEnsemble-shaped one.  The stand-in iterators
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


def seq_matmul(a, b):
    """a @ b ([E, M, K] by [E, K, N]) with the K products of every element added one after the other in the operands' dtype: the
    summation order of a plain loop (the MFMA kernels accumulate along K in order too; torch's matmul blocks and vectorises)."""
    acc = torch.zeros(a.shape[0], a.shape[1], b.shape[2], dtype=a.dtype)
    for k in range(a.shape[2]):
        acc += a[:, :, k:k + 1] * b[:, k:k + 1, :]
    return acc


def forward(ws, bs, x, act, slope=0.01, sequential=False):
    """x [E, B, in] -> (list of layer inputs, list of hidden pre-activations, raw output [E, B, output columns]).
    ``sequential``: every contraction through seq_matmul."""
    mm = seq_matmul if sequential else torch.matmul
    inputs, zs = [x], []
    h = x
    for li in range(len(ws)):
        z = mm(h, ws[li]) + bs[li]
        if li < len(ws) - 1:
            zs.append(z)
            h = act_fwd(act, z, slope)
            inputs.append(h)
        else:
            return inputs, zs, z


def backward(ws, inputs, zs, dz, act, slope=0.01, sequential=False):
    """The raw gradients (dws, dbs) behind dz = d loss / d (raw output), last layer first (weights as the forward pass saw them)."""
    mm = seq_matmul if sequential else torch.matmul
    dws, dbs = [None] * len(ws), [None] * len(ws)
    for li in range(len(ws) - 1, -1, -1):
        dws[li] = mm(inputs[li].transpose(1, 2), dz)
        dbs[li] = mm(torch.ones_like(dz[:, :, :1]).transpose(1, 2), dz) if sequential else dz.sum(1, keepdim=True)
        if li > 0:
            dz = mm(dz, ws[li].transpose(1, 2)) * act_grad(act, zs[li - 1], slope)
    return dws, dbs


def nll_step(ws, bs, x, y, min_lv, max_lv, act, slope=0.01, grad_scale=1.0, sequential=False):
    """GaussianMLP._nll_loss: per-member mean NLL [E] (without grad_scale) and the raw gradients (dws, dbs) of grad_scale * their
    sum, for x [E, B, in], y [E, B, out]; min_lv / max_lv broadcast against [E, B, out] ([1, out] shared, [E, 1, out] per member)."""
    inputs, zs, o = forward(ws, bs, x, act, slope, sequential)
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
    if grad_scale == 1.0:  # the plain mean's division by n; any other scale is folded into one factor, as the kernel folds it
        dmean, dlv = 2 * d * iv / n, (1 - l2iv) / n
    else:
        dmean, dlv = 2 * d * iv * (grad_scale / n), (1 - l2iv) * (grad_scale / n)
    draw = dlv * softplus_grad(w) * softplus_grad(u)
    return loss, *backward(ws, inputs, zs, torch.cat([dmean, draw], dim=-1), act, slope, sequential)


def mse_step(ws, bs, x, y, act, slope=0.01, grad_scale=1.0, sequential=False):
    """GaussianMLP._mse_loss (mbrl/models/gaussian_mlp.py:283-289) of a deterministic model, whose output layer is out wide:
    per-member loss [E] (the SUM over rows and dims of the squared error, without grad_scale) and the raw gradients (dws, dbs) of
    grad_scale * loss."""
    inputs, zs, o = forward(ws, bs, x, act, slope, sequential)
    d = o - y
    loss = (d * d).sum((1, 2))
    return loss, *backward(ws, inputs, zs, 2 * d * grad_scale, act, slope, sequential)


def bounds_3d(t, E):
    """logvar bounds [out] / [1, out] (shared) or [E, out] (per member) as a tensor that broadcasts against [E, B, out]"""
    t = t.reshape(-1, t.shape[-1])
    return t.reshape(1, 1, -1) if t.shape[0] == 1 else t.reshape(E, 1, -1)


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


def train_step(ws, bs, ms, vs, x, y, min_lv, max_lv, act, step, lr, weight_decay, eps=1e-8, slope=0.01, grad_scale=1.0, sequential=False,
               kind="nll"):
    """One Model.update of loss ``kind`` ("nll" / "mse": min_lv / max_lv are not read) in place on ws / bs (lists of [E, ., .]) and
    the Adam moments ms / vs = ([per-layer w], [per-layer b]).  grad_scale is the 1 / E of BasicEnsemble.loss
    (basic_ensemble.py:196-221), which reaches every member's gradient (and so grad_norm, model.py:156-167) but not its reported
    loss.  Returns (per-member loss [E], per-member sum of squared raw gradients [E], grad_scale included)."""
    if kind == "mse":
        loss, dws, dbs = mse_step(ws, bs, x, y, act, slope, grad_scale, sequential)
    else:
        E = ws[0].shape[0]
        loss, dws, dbs = nll_step(ws, bs, x, y, bounds_3d(min_lv, E), bounds_3d(max_lv, E), act, slope, grad_scale, sequential)
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


def random_model(E, in_dim, hid, out, n_layers, seed, dtype=torch.float64, kind="nll"):
    """(ws, bs) with the output layer of the kind: 2 out wide under "nll" (mean | raw logvar), out wide under "mse" """
    g = torch.Generator().manual_seed(seed)
    dims = [in_dim] + [hid] * (n_layers - 1) + [out if kind == "mse" else 2 * out]
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
    """ws / bs [E, ., .] into a stand-in model: whole into a TinyGaussianMLP's layers, row e into member e where layers() gives a
    list of the members' one-member layers (train_loss_restatement.TinyBasicEnsemble)"""
    with torch.no_grad():
        for lin, w, b in zip(mlp.layers(), ws, bs):
            w, b = torch.as_tensor(w), torch.as_tensor(b)
            if isinstance(lin, list):
                for e, member in enumerate(lin):
                    member.weight.copy_(w[e:e + 1])
                    member.bias.copy_(b[e:e + 1])
            else:
                lin.weight.copy_(w)
                lin.bias.copy_(b)


class CpuEngine:
    """Engine.train_steps / train_eval in float32 on the CPU through the restatement (host-logic tests, and the measured final-weight
    bound of the GPU golden tests).  ``kinds=False``: the engine as it was before the loss kinds -- it refuses the keywords ``loss``,
    ``grad_scale`` and ``bounds_per_member``.  ``mirrored``: every contraction of a step sums the same terms in the other order
    (mirrored network and inputs, minibatch rows reversed).  ``calls`` records the keywords of every call."""

    device = torch.device("cpu")

    def __init__(self, kinds=True, mirrored=False):
        self.kinds, self.mirrored, self.calls = kinds, mirrored, []

    def _kind_keywords(self, fn, given, **defaults):
        if given and not self.kinds or set(given) - set(defaults):
            raise TypeError(f"{fn}() got an unexpected keyword argument {sorted(given)[0]!r}")
        return dict(defaults, **given)

    def train_steps(self, weights, biases, exp_avg, exp_avg_sq, lo, hi, x, y, idx, rows, step0, *, lr, betas=(0.9, 0.999), eps=1e-8,
                    weight_decay=0.0, activation="silu", leaky_slope=0.01, steps_per_launch=0, **kind):
        kind = self._kind_keywords("train_steps", kind, loss="nll", grad_scale=1.0, bounds_per_member=False)
        loss, grad_scale = kind["loss"], kind["grad_scale"]
        self.calls.append(dict(fn="train_steps", idx=idx.clone(), rows=rows.clone(), lo=lo, hi=hi, **kind))
        E, out = weights[0].shape[0], y.shape[1]
        if loss == "nll":
            assert lo.numel() == hi.numel() == (E * out if kind["bounds_per_member"] else out)
            lo, hi = lo.reshape(-1, out), hi.reshape(-1, out)
        else:
            assert lo is None and hi is None and weights[-1].shape[2] == out
        state = (weights, biases, exp_avg[0], exp_avg[1], exp_avg_sq[0], exp_avg_sq[1])
        if self.mirrored:
            w, b, mw, mb, vw, vb = (list(p) for pair in (mirrored(weights, biases), mirrored(*exp_avg), mirrored(*exp_avg_sq)) for p in pair)
            w, b, mw, mb, vw, vb = ([t.clone() for t in ts] for ts in (w, b, mw, mb, vw, vb))
            x = x.flip(1)
        else:
            w, b, mw, mb, vw, vb = state
        losses, gsqs = [], []
        for s in range(idx.shape[0]):
            sel = idx[s, :, :int(rows[s])].long()
            if self.mirrored:
                sel = sel.flip(-1)
            l, g = train_step(w, b, (mw, mb), (vw, vb), x[sel], y[sel], lo, hi, activation, step0 + s + 1, lr, weight_decay, eps, leaky_slope,
                              grad_scale, kind=loss)
            losses.append(l)
            gsqs.append(g)
        if self.mirrored:
            back = [p for pair in (mirrored(w, b), mirrored(mw, mb), mirrored(vw, vb)) for p in pair]
            for dst, src in zip(state, back):
                for d, s_ in zip(dst, src):
                    d.copy_(s_)
        self.calls[-1].update(loss_out=torch.stack(losses), gsq_out=torch.stack(gsqs))
        return torch.stack(losses), torch.stack(gsqs)

    def train_eval(self, weights, biases, x, y, order=None, *, activation="silu", leaky_slope=0.01, row_scores=False, **kind):
        kind = self._kind_keywords("train_eval", kind, loss="nll")
        self.calls.append(dict(fn="train_eval", **kind))
        assert weights[-1].shape[2] == (y.shape[1] if kind["loss"] == "mse" else 2 * y.shape[1])
        score = eval_score(weights, biases, x, y, activation, leaky_slope)
        if not row_scores:
            return score
        xo, yo = (x[order.long()], y[order.long()]) if order is not None else (x, y)
        _, _, o = forward(weights, biases, xo.unsqueeze(0).expand(weights[0].shape[0], -1, -1), activation, leaky_slope)
        return score, ((o[..., :y.shape[1]] - yo) ** 2).sum(-1)


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


def member_bounds(E, out, dtype=torch.float64):
    """Per-member bounds [E, out]: the defaults (-10, 0.5), but member 1 clamps column 0 to (-2, -1): a kernel that reads member 0's
    bounds for everyone computes another loss for member 1."""
    lo, hi = -10 * torch.ones(E, out, dtype=dtype), 0.5 * torch.ones(E, out, dtype=dtype)
    lo[1, 0], hi[1, 0] = -2.0, -1.0
    return lo, hi


def run_steps(engine, E, B, in_dim, hid, out, n_layers, act, n_steps, N=None, seed=0, steps_per_launch=0, ragged_last=False, *,
              kind="nll", per_member_bounds=False, grad_scale=1.0, bounds=None, edit_params=None, rows=None, edit_idx=None, step0=0,
              calls=None, restate=True, f32_orders=False, sequential_order=False, device="cuda:0"):
    """n_steps steps of loss ``kind`` on the GPU and in the float32 / float64 restatements; returns the three final states and
    per-step losses ({"hip" | "f32" | "f64": (w, b, m, v, loss [S, E], grad_sq [S, E])}) and, under "inputs", what the run was fed.

    "nll" runs with shared logvar bounds [1, out] (one column's are active), or with per_member_bounds (member_bounds); "mse" with
    none.  The engine is handed ``loss`` / ``grad_scale`` / ``bounds_per_member`` only where one of them is off its default.
    bounds(lo, hi) edits the bounds in place; edit_params(ws, bs) the float64 initial parameters; rows is an
    explicit per-step row count (n_steps = len(rows)); edit_idx(idx) edits the int32 schedule [S, E, B] in place (an index
    outside [0, N) stands for a row of zeros, in the restatement too); step0 = Adam steps taken before; calls = step counts
    of consecutive train_steps calls the run is split into; restate=False skips the CPU restatements; f32_orders adds two float32
    restatements of the same sums in other orders: "f32r" with every minibatch's rows reversed (the contractions over the batch),
    "f32m" with the rows reversed and the network mirrored (every contraction); sequential_order a third, "f32s", with every
    contraction summed one product after the other (seq_matmul), the order closest to the kernel's."""
    g = torch.Generator().manual_seed(seed + 1)
    N = N or max(3 * B, 64)
    x = torch.randn(N, in_dim, generator=g, dtype=torch.float64)
    y = torch.randn(N, out, generator=g, dtype=torch.float64) * 0.3
    ws, bs = random_model(E, in_dim, hid, out, n_layers, seed, kind=kind)
    if edit_params is not None:
        edit_params(ws, bs)
    if kind != "nll":
        lo = hi = None
    elif per_member_bounds:
        lo, hi = member_bounds(E, out)
    else:
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
    kinds = ((("f64", torch.float64), ("f32", torch.float32)) + ((("f32r", torch.float32), ("f32m", torch.float32)) if f32_orders else ())
             + ((("f32s", torch.float32),) if sequential_order else ()))
    scale = float(np.float32(grad_scale))  # the float32 value the library is handed
    for name, dtype in kinds if restate else ():
        w, b, m, v = fresh_state(*(mirrored(ws, bs) if name == "f32m" else (ws, bs)), dtype, "cpu")
        xd, yd = (x0.flip(1) if name == "f32m" else x0).to(dtype), y0.to(dtype)
        lod, hid_ = (lo.to(dtype), hi.to(dtype)) if kind == "nll" else (None, None)
        losses, gsqs = [], []
        for s in range(n_steps):
            sel = sel_all[s, :, :rows[s]]
            if name in ("f32r", "f32m"):
                sel = sel.flip(-1)
            l, gq = train_step(w, b, m, v, xd[sel], yd[sel], lod, hid_, act, step0 + s + 1, LR, WD, grad_scale=scale,
                               sequential=name == "f32s", kind=kind)
            losses.append(l)
            gsqs.append(gq)
        if name == "f32m":
            (w, b), m, v = mirrored(w, b), mirrored(*m), mirrored(*v)
        res[name] = (w, b, m, v, torch.stack(losses), torch.stack(gsqs))
    w, b, m, v = fresh_state(ws, bs, torch.float32, device)
    lo_d, hi_d = (lo.float().reshape(-1).to(device), hi.float().reshape(-1).to(device)) if kind == "nll" else (None, None)
    kw = {} if (kind, per_member_bounds, grad_scale) == ("nll", False, 1.0) else dict(loss=kind, grad_scale=grad_scale,
                                                                                      bounds_per_member=per_member_bounds)
    x_d, y_d, idx_d, rows_d = x.float().to(device), y.float().to(device), idx.to(device), rows.to(device)
    loss, gsq, done = [], [], 0
    for n in calls or [n_steps]:
        l, gq = engine.train_steps(w, b, m, v, lo_d, hi_d, x_d, y_d, idx_d[done:done + n].contiguous(), rows_d[done:done + n].contiguous(),
                                   step0 + done, lr=LR, weight_decay=WD, activation=act, steps_per_launch=steps_per_launch, **kw)
        loss.append(l)
        gsq.append(gq)
        done += n
    assert done == n_steps
    if device != "cpu":
        torch.cuda.synchronize()
    res["hip"] = (w, b, m, v, torch.cat(loss), torch.cat(gsq))
    return res
