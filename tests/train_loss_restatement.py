"""TEST HELPER (not collected): tests/train_restatement.py extended to the loss kinds hipets.ModelTrainer trains with
``extended=True``, written out by hand in torch (no autograd, no torch.optim), in float64 or float32:

  mse_step         GaussianMLP._mse_loss (mbrl/models/gaussian_mlp.py:283-289): the SUM over rows and dims of the squared error of a
                   deterministic model, whose output layer is out wide, and its gradient
  nll_step_kind    train_restatement.nll_step with per-member logvar bounds and a gradient scale
  train_step_kind  one Model.update of either kind: grad_scale is the 1 / E of BasicEnsemble.loss (basic_ensemble.py:196-221), which
                   reaches every member's gradient (and so grad_norm, model.py:156-167) but not its reported loss

plus the stand-ins the tests need where mbrl is not installed: TinyBasicEnsemble (a ``members`` ModuleList of one-member
TinyGaussianMLPs in the reference's parameter order), a CPU engine that accepts the new keywords (and can run every contraction
in the other summation order), and run_steps_kind: the same steps on the GPU and in both restatements."""
from __future__ import annotations

import json
import warnings

import numpy as np
import torch

import train_restatement as tr


def seq_matmul(a, b):
    """a @ b ([E, M, K] by [E, K, N]) with the K products of every element added one after the other in the operands' dtype: the
    summation order of a plain loop (the MFMA kernels accumulate along K in order too; torch's matmul blocks and vectorises)."""
    acc = torch.zeros(a.shape[0], a.shape[1], b.shape[2], dtype=a.dtype)
    for k in range(a.shape[2]):
        acc += a[:, :, k:k + 1] * b[:, k:k + 1, :]
    return acc


def _forward(ws, bs, x, act, slope, sequential):
    if not sequential:
        return tr.forward(ws, bs, x, act, slope)
    inputs, zs, h = [x], [], x
    for li in range(len(ws)):
        z = seq_matmul(h, ws[li]) + bs[li]
        if li == len(ws) - 1:
            return inputs, zs, z
        zs.append(z)
        h = tr.act_fwd(act, z, slope)
        inputs.append(h)


def mse_step(ws, bs, x, y, act, slope=0.01, grad_scale=1.0, sequential=False):
    """Per-member loss [E] (sum of squared errors, without grad_scale) and the raw gradients (dws, dbs) of grad_scale * loss.
    ``sequential``: every contraction through seq_matmul."""
    inputs, zs, o = _forward(ws, bs, x, act, slope, sequential)
    d = o - y
    loss = (d * d).sum((1, 2))
    return loss, *_backward(ws, inputs, zs, 2 * d * grad_scale, act, slope, sequential)


def nll_step_kind(ws, bs, x, y, min_lv, max_lv, act, slope=0.01, grad_scale=1.0, sequential=False):
    """Per-member mean NLL [E] (without grad_scale) and the raw gradients of grad_scale * sum of them; min_lv / max_lv are
    [1, out] (shared) or [E, 1, out] (member e's own bounds).  ``sequential``: every contraction through seq_matmul."""
    inputs, zs, o = _forward(ws, bs, x, act, slope, sequential)
    out = y.shape[-1]
    mean, raw = o[..., :out], o[..., out:]
    u = max_lv - raw
    lv1 = max_lv - tr.softplus(u)
    w = lv1 - min_lv
    lv = min_lv + tr.softplus(w)
    d = mean - y
    iv = torch.exp(-lv)
    l2iv = d * d * iv
    n = y.shape[1] * out
    loss = (l2iv + lv).sum((1, 2)) / n
    scale = grad_scale / n
    dmean = 2 * d * iv * scale
    draw = (1 - l2iv) * scale * tr.softplus_grad(w) * tr.softplus_grad(u)
    return loss, *_backward(ws, inputs, zs, torch.cat([dmean, draw], dim=-1), act, slope, sequential)


def _backward(ws, inputs, zs, dz, act, slope, sequential=False):
    mm = seq_matmul if sequential else torch.matmul
    dws, dbs = [None] * len(ws), [None] * len(ws)
    for li in range(len(ws) - 1, -1, -1):
        dws[li] = mm(inputs[li].transpose(1, 2), dz)
        dbs[li] = mm(torch.ones_like(dz[:, :, :1]).transpose(1, 2), dz) if sequential else dz.sum(1, keepdim=True)
        if li > 0:
            dz = mm(dz, ws[li].transpose(1, 2)) * tr.act_grad(act, zs[li - 1], slope)
    return dws, dbs


def bounds_3d(t, E):
    """logvar bounds [out] / [1, out] (shared) or [E, out] (per member) as a tensor that broadcasts against [E, B, out]"""
    t = t.reshape(-1, t.shape[-1])
    return t.reshape(1, 1, -1) if t.shape[0] == 1 else t.reshape(E, 1, -1)


def train_step_kind(kind, ws, bs, ms, vs, x, y, min_lv, max_lv, act, step, lr, weight_decay, eps=1e-8, slope=0.01, grad_scale=1.0,
                    sequential=False):
    """One Model.update of loss ``kind`` ("nll" / "mse") in place on ws / bs and the Adam moments; returns (per-member loss [E],
    per-member sum of squared raw gradients [E], grad_scale included).  ``sequential``: every contraction through seq_matmul."""
    E = ws[0].shape[0]
    if kind == "mse":
        loss, dws, dbs = mse_step(ws, bs, x, y, act, slope, grad_scale, sequential)
    else:
        loss, dws, dbs = nll_step_kind(ws, bs, x, y, bounds_3d(min_lv, E), bounds_3d(max_lv, E), act, slope, grad_scale, sequential)
    gsq = sum((g * g).sum((1, 2)) for g in dws + dbs)
    for li in range(len(ws)):
        tr.adam_(ws[li], dws[li], ms[0][li], vs[0][li], step, lr, eps=eps, weight_decay=weight_decay)
        tr.adam_(bs[li], dbs[li], ms[1][li], vs[1][li], step, lr, eps=eps, weight_decay=weight_decay)
    return loss, gsq


def random_model_kind(kind, E, in_dim, hid, out, n_layers, seed, dtype=torch.float64):
    """train_restatement.random_model with the output layer of the kind: out wide under "mse", 2 out under "nll" """
    g = torch.Generator().manual_seed(seed)
    dims = [in_dim] + [hid] * (n_layers - 1) + [out if kind == "mse" else 2 * out]
    ws = [torch.randn(E, dims[i], dims[i + 1], generator=g, dtype=dtype) / (2 * dims[i] ** 0.5) for i in range(n_layers)]
    bs = [torch.randn(E, 1, dims[i + 1], generator=g, dtype=dtype) * 0.1 for i in range(n_layers)]
    return ws, bs


# ---- stand-ins for the live objects ------------------------------------------------------------------------------------
class TinyBasicEnsemble(torch.nn.Module):
    """The attributes hipets.ModelTrainer reads from a BasicEnsemble of one-member GaussianMLPs: ``members``, ``deterministic``,
    ``__len__``, a set_elite that warns and keeps every member (basic_ensemble.py:262-267).  parameters() runs member by member
    (min_logvar, max_logvar, then the layers' weight / bias), the reference's order."""

    def __init__(self, E, in_dim, hid, out, n_layers, act="silu", deterministic=False, learn_logvar_bounds=False):
        super().__init__()
        self.members = torch.nn.ModuleList([tr.TinyGaussianMLP(1, in_dim, hid, out, n_layers, act=act, deterministic=deterministic,
                                                               learn_logvar_bounds=learn_logvar_bounds) for _ in range(E)])
        self.num_members = E
        self.deterministic = deterministic
        self.elite_models = None

    def __len__(self):
        return len(self.members)

    def layers(self):
        """per linear layer, a stand-in whose weight / bias are the members' [1, ., .] parameters in member order"""
        per_member = [m.layers() for m in self.members]
        return [[pm[i] for pm in per_member] for i in range(len(per_member[0]))]

    def set_elite(self, elite):
        warnings.warn("BasicEnsemble does not support elite models yet. All models will be used.")


def load_params_kind(mlp, ws, bs):
    """tr.load_params for either stand-in: ws / bs [E, ., .] go whole into a TinyGaussianMLP, row e into member e of a
    TinyBasicEnsemble"""
    if not isinstance(mlp, TinyBasicEnsemble):
        return tr.load_params(mlp, ws, bs)
    with torch.no_grad():
        for layer, w, b in zip(mlp.layers(), ws, bs):
            for e, lin in enumerate(layer):
                lin.weight.copy_(torch.as_tensor(w)[e:e + 1])
                lin.bias.copy_(torch.as_tensor(b)[e:e + 1])


def stacked_params(mlp):
    """(ws, bs) [E, ., .] of the live parameters of either stand-in"""
    if not isinstance(mlp, TinyBasicEnsemble):
        return [l.weight.detach().clone() for l in mlp.layers()], [l.bias.detach().clone() for l in mlp.layers()]
    return ([torch.cat([l.weight.detach() for l in layer]) for layer in mlp.layers()],
            [torch.cat([l.bias.detach() for l in layer]) for layer in mlp.layers()])


class CpuEngineKinds:
    """Engine.train_steps / train_eval with the loss keywords, in float32 on the CPU through the restatement (host-logic tests, and the
    measured final-weight bound of the GPU golden tests).  ``mirrored``: every contraction of a step sums the same terms in the other
    order (train_restatement.mirrored network and inputs, minibatch rows reversed).  ``calls`` records the keywords of every call."""

    device = torch.device("cpu")

    def __init__(self, mirrored=False):
        self.mirrored = mirrored
        self.calls = []

    def train_steps(self, weights, biases, exp_avg, exp_avg_sq, lo, hi, x, y, idx, rows, step0, *, lr, betas=(0.9, 0.999), eps=1e-8,
                    weight_decay=0.0, activation="silu", leaky_slope=0.01, steps_per_launch=0, loss="nll", grad_scale=1.0,
                    bounds_per_member=False):
        self.calls.append(dict(fn="train_steps", loss=loss, grad_scale=grad_scale, bounds_per_member=bounds_per_member,
                               idx=idx.clone(), rows=rows.clone(), lo=lo, hi=hi))
        E, out = weights[0].shape[0], y.shape[1]
        if loss == "nll":
            assert lo.numel() == hi.numel() == (E * out if bounds_per_member else out)
            lo, hi = lo.reshape(-1, out), hi.reshape(-1, out)
        else:
            assert lo is None and hi is None and weights[-1].shape[2] == out
        state = (weights, biases, exp_avg[0], exp_avg[1], exp_avg_sq[0], exp_avg_sq[1])
        if self.mirrored:
            w, b, mw, mb, vw, vb = (list(p) for pair in (tr.mirrored(weights, biases), tr.mirrored(*exp_avg), tr.mirrored(*exp_avg_sq)) for p in pair)
            w, b, mw, mb, vw, vb = ([t.clone() for t in ts] for ts in (w, b, mw, mb, vw, vb))
            x = x.flip(1)
        else:
            w, b, mw, mb, vw, vb = state
        losses, gsqs = [], []
        for s in range(idx.shape[0]):
            sel = idx[s, :, :int(rows[s])].long()
            if self.mirrored:
                sel = sel.flip(-1)
            l, g = train_step_kind(loss, w, b, (mw, mb), (vw, vb), x[sel], y[sel], lo, hi, activation, step0 + s + 1, lr, weight_decay, eps,
                                   leaky_slope, grad_scale)
            losses.append(l)
            gsqs.append(g)
        if self.mirrored:
            back = [p for pair in (tr.mirrored(w, b), tr.mirrored(mw, mb), tr.mirrored(vw, vb)) for p in pair]
            for dst, src in zip(state, back):
                for d, s_ in zip(dst, src):
                    d.copy_(s_)
        self.calls[-1].update(loss_out=torch.stack(losses), gsq_out=torch.stack(gsqs))
        return torch.stack(losses), torch.stack(gsqs)

    def train_eval(self, weights, biases, x, y, order=None, *, activation="silu", leaky_slope=0.01, row_scores=False, loss="nll"):
        self.calls.append(dict(fn="train_eval", loss=loss))
        assert weights[-1].shape[2] == (y.shape[1] if loss == "mse" else 2 * y.shape[1])
        score = tr.eval_score(weights, biases, x, y, activation, leaky_slope)
        if not row_scores:
            return score
        xo, yo = (x[order.long()], y[order.long()]) if order is not None else (x, y)
        _, _, o = tr.forward(weights, biases, xo.unsqueeze(0).expand(weights[0].shape[0], -1, -1), activation, leaky_slope)
        return score, ((o[..., :y.shape[1]] - yo) ** 2).sum(-1)


def golden_setup(meta, arr):
    """The model of a tests/golden/trainerx_*.npz recording at its initial weights (and bounds) with the reference's split, member
    indices and RNG state: (mlp, dynamics model, train iterator, validation iterator or None, rng)."""
    E, L = meta["E"], meta["n_layers"]
    cls = TinyBasicEnsemble if meta["basic"] else tr.TinyGaussianMLP
    mlp = cls(E, meta["in_dim"], meta["hid"], meta["out"], L, act=meta["act"], deterministic=meta["deterministic"])
    load_params_kind(mlp, [arr[f"w0_{i}"] for i in range(L)], [arr[f"b0_{i}"] for i in range(L)])
    if not meta["deterministic"]:
        with torch.no_grad():
            for e, m in enumerate(mlp.members if meta["basic"] else [mlp]):
                m.min_logvar.copy_(torch.from_numpy(arr["min_logvar"][e:e + 1]))
                m.max_logvar.copy_(torch.from_numpy(arr["max_logvar"][e:e + 1]))
    model = tr.TinyDynamicsModel(mlp, num_elites=meta["num_elites"])
    data = tr.Batch(obs=arr["obs"], act=arr["act"], next_obs=arr["next_obs"])
    rng = np.random.default_rng()
    rng.bit_generator.state = json.loads(meta["rng_state_after_split"])
    train = tr.BootstrapIterator(data[arr["train_rows"]], meta["batch_size"], E, shuffle_each_epoch=True, rng=rng,
                                 member_indices=arr["member_indices"])
    val = None
    if len(arr["val_rows"]):
        val = tr.TransitionIterator(data[arr["val_rows"]], meta["batch_size"], shuffle_each_epoch=False, rng=rng)
    return mlp, model, train, val, rng


# ---- shared by the GPU tests (tests/test_gpu_trainer_kinds.py) --------------------------------------------------------------
def member_bounds(E, out, dtype=torch.float64):
    """Per-member bounds [E, out]: the defaults (-10, 0.5), but member 1 clamps column 0 to (-2, -1): a kernel that reads member 0's
    bounds for everyone computes another loss for member 1."""
    lo, hi = -10 * torch.ones(E, out, dtype=dtype), 0.5 * torch.ones(E, out, dtype=dtype)
    lo[1, 0], hi[1, 0] = -2.0, -1.0
    return lo, hi


def run_steps_kind(engine, kind, E, B, in_dim, hid, out, n_layers, act, n_steps, N=None, seed=0, steps_per_launch=0, ragged_last=False, *,
                   grad_scale=1.0, restate=True, f32_orders=False, device="cuda:0"):
    """n_steps steps of loss ``kind`` on the GPU and in the float32 / float64 restatements, as train_restatement.run_steps: returns
    {"hip" | "f32" | "f64": (w, b, m, v, loss [S, E], grad_sq [S, E])} and, under "inputs", what the run was fed.  "nll" runs with
    per-member bounds (member_bounds).  f32_orders adds the two further float32 restatements of train_restatement.run_steps: "f32r" with
    every minibatch's rows reversed (the contractions over the batch sum in the other order), "f32m" with the rows reversed and the
    network mirrored (every contraction does); and a third, "f32s", with every contraction summed one product after the other
    (seq_matmul), the order closest to the kernel's."""
    g = torch.Generator().manual_seed(seed + 1)
    N = N or max(3 * B, 64)
    x = torch.randn(N, in_dim, generator=g, dtype=torch.float64)
    y = torch.randn(N, out, generator=g, dtype=torch.float64) * 0.3
    ws, bs = random_model_kind(kind, E, in_dim, hid, out, n_layers, seed)
    lo, hi = member_bounds(E, out) if kind == "nll" else (None, None)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:B] for _ in range(E)]) for _ in range(n_steps)]).to(torch.int32)
    rows = torch.full((n_steps,), B, dtype=torch.int32)
    if ragged_last:
        rows[-1] = max(1, B // 3)
    res = {"inputs": dict(x=x, y=y, ws=ws, bs=bs, lo=lo, hi=hi, idx=idx, rows=rows)}
    kinds = (("f64", torch.float64), ("f32", torch.float32)) + ((("f32r", torch.float32), ("f32m", torch.float32), ("f32s", torch.float32)) if f32_orders else ())
    for name, dtype in kinds if restate else ():
        w, b, m, v = tr.fresh_state(*(tr.mirrored(ws, bs) if name == "f32m" else (ws, bs)), dtype, "cpu")
        xd, yd = (x.flip(1) if name == "f32m" else x).to(dtype), y.to(dtype)
        lod, hid_ = (lo.to(dtype), hi.to(dtype)) if kind == "nll" else (None, None)
        losses, gsqs = [], []
        for s in range(n_steps):
            sel = idx[s, :, :rows[s]].long()
            if name in ("f32r", "f32m"):
                sel = sel.flip(-1)
            l, gq = train_step_kind(kind, w, b, m, v, xd[sel], yd[sel], lod, hid_, act, s + 1, tr.LR, tr.WD,
                                    grad_scale=float(np.float32(grad_scale)),  # the float32 value the library is handed
                                    sequential=name == "f32s")
            losses.append(l)
            gsqs.append(gq)
        if name == "f32m":
            (w, b), m, v = tr.mirrored(w, b), tr.mirrored(*m), tr.mirrored(*v)
        res[name] = (w, b, m, v, torch.stack(losses), torch.stack(gsqs))
    w, b, m, v = tr.fresh_state(ws, bs, torch.float32, device)
    lo_d, hi_d = (lo.float().to(device).contiguous(), hi.float().to(device).contiguous()) if kind == "nll" else (None, None)
    loss, gsq = engine.train_steps(w, b, m, v, lo_d, hi_d, x.float().to(device), y.float().to(device), idx.to(device), rows.to(device), 0,
                                   lr=tr.LR, weight_decay=tr.WD, activation=act, steps_per_launch=steps_per_launch, loss=kind,
                                   grad_scale=grad_scale, bounds_per_member=kind == "nll")
    if device != "cpu":
        torch.cuda.synchronize()
    res["hip"] = (w, b, m, v, loss, gsq)
    return res
