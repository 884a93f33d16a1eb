"""PlaNet's posterior update on the device: what every environment step of ``mbrl/algorithms/planet.py:162-170`` runs before it plans.

    posterior = hipets.PlaNetPosterior(planet_model)            # or (planet_model, n_env=16) for the batched agents
    posterior.reset()
    state = posterior.update(obs, action=action, rng=rng)       # the stock loop's planet.update_posterior(obs, action, rng)

``PlaNetModel.update_posterior`` (mbrl/models/planet.py:592-641 -> :309-347) -- pixel normalisation, ``Conv2dEncoder``
(mbrl/models/util.py:101-157), ``BeliefModel``, ``posterior_transition_model`` and one sample -- as one HIP launch per conv layer, one
for the encoding half of the posterior's first Linear and one for the head, for ``n_env`` environments at once.  With a live model
and ``n_env == 1`` the results are also stored where the reference keeps them, so ``PlaNetModel.reset``, ``render`` and
``PlaNetTrajectoryEvalFn.prepare()`` work unchanged; the batched results are what ``Batched*Agent.plan`` takes as ``latent=`` /
``belief=``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ._lib import ENCODER_MAX, POSTERIOR_MAX
from .engine import Engine, get_engine
from .model import UnsupportedModelError, is_planet_model
from .reference_draws import planet_posterior_draws

_LDS_LIMIT = 160 * 1024  # the engine's LDS opt-in limit (hipets_create)
_STOCK = "; keep the stock route (PlaNetModel.update_posterior)"


def _pad16(x: int) -> int:
    return (x + 15) & ~15


@dataclass
class PlaNetPosteriorSpec:
    """The tensors ``PlaNetModel.update_posterior`` reads, torch layouts ([out, in] Linear weights, [C_out, C_in, k, k] conv weights);
    the belief tensors carry ``PlaNetSpec``'s names."""

    conv_weights: List[torch.Tensor]  # encoder.convs[i][0]
    conv_biases: List[torch.Tensor]
    strides: List[int]
    w_embed: torch.Tensor  # belief_model.embedding_layer[0]
    b_embed: torch.Tensor
    w_ih: torch.Tensor  # belief_model.rnn (GRUCell), gates r | z | n
    b_ih: torch.Tensor
    w_hh: torch.Tensor
    b_hh: torch.Tensor
    w_post1: torch.Tensor  # posterior_transition_model[0]: [F, Hb + enc] over [belief | encoding]
    b_post1: torch.Tensor
    w_post2: torch.Tensor  # posterior_transition_model[2]: [2 L, F]
    b_post2: torch.Tensor
    image_shape: Tuple[int, int, int] = (3, 64, 64)
    w_fc: Optional[torch.Tensor] = None  # encoder.fc, None for nn.Identity
    b_fc: Optional[torch.Tensor] = None
    min_std: float = 0.1
    layer_shapes: List[Tuple[int, int, int]] = field(default_factory=list, repr=False)  # (C, H, W) behind every conv layer, by validate()

    @property
    def latent_size(self) -> int:
        return int(self.w_post2.shape[0]) // 2

    @property
    def belief_size(self) -> int:
        return int(self.w_hh.shape[1])

    @property
    def action_size(self) -> int:
        return int(self.w_embed.shape[1]) - self.latent_size

    @property
    def hidden_size(self) -> int:
        return int(self.w_post1.shape[0])

    @property
    def encoding_size(self) -> int:
        return int(self.w_post1.shape[1]) - self.belief_size

    def tensors(self) -> list:
        """The pointer table of hipets_planet_posterior_set_model, in its order."""
        convs = [t for pair in zip(self.conv_weights, self.conv_biases) for t in pair]
        return convs + [self.w_fc, self.b_fc, self.w_embed, self.b_embed, self.w_ih, self.b_ih, self.w_hh, self.b_hh, self.w_post1, self.b_post1,
                        self.w_post2, self.b_post2]

    def validate(self):
        n = len(self.conv_weights)
        if not (len(self.conv_biases) == len(self.strides) == n):
            raise UnsupportedModelError("encoder needs one bias and one stride per conv weight")

        def within(limits):
            for v, lo, hi, what in limits:
                if not lo <= v <= hi:
                    raise UnsupportedModelError(f"{what} {v} outside [{lo}, {hi}]" + _STOCK)

        within([(n, 1, ENCODER_MAX["convs"], "conv layers"), (self.image_shape[0], 1, ENCODER_MAX["channels"], "image channels"),
                (self.image_shape[1], 1, ENCODER_MAX["image"], "image height"), (self.image_shape[2], 1, ENCODER_MAX["image"], "image width")])
        C, H, W = (int(v) for v in self.image_shape)
        shapes = []
        for i, (w, b, s) in enumerate(zip(self.conv_weights, self.conv_biases, self.strides)):
            if w.ndim != 4 or w.shape[2] != w.shape[3]:
                raise UnsupportedModelError(f"conv layer {i} has a non-square kernel {tuple(w.shape)}" + _STOCK)
            c_out, c_in, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
            if c_in != C or tuple(b.shape) != (c_out,):
                raise UnsupportedModelError(f"conv layer {i} ({tuple(w.shape)}, bias {tuple(b.shape)}) does not chain onto {C} channels")
            within([(c_out, 1, ENCODER_MAX["channels"], f"conv layer {i} channels"), (k, 1, min(ENCODER_MAX["kernel"], H, W), f"conv layer {i} kernel"),
                    (int(s), 1, ENCODER_MAX["stride"], f"conv layer {i} stride")])
            C, H, W = c_out, (H - k) // int(s) + 1, (W - k) // int(s) + 1
            if C * H * W > ENCODER_MAX["layer_floats"]:
                raise UnsupportedModelError(f"conv layer {i} has {C * H * W} outputs per image, more than {ENCODER_MAX['layer_floats']}" + _STOCK)
            shapes.append((C, H, W))
        self.layer_shapes = shapes
        flat = C * H * W
        L, A, Hb, F, enc = self.latent_size, self.action_size, self.belief_size, self.hidden_size, self.encoding_size
        if (self.w_fc is None) != (self.b_fc is None):
            raise UnsupportedModelError("the encoder's Linear needs weight and bias, or neither")
        if self.w_fc is None and flat != enc:
            raise UnsupportedModelError(f"no encoder Linear, and the flattened conv output {flat} is not the encoding size {enc}")
        for v, hi, what in ((flat, ENCODER_MAX["flat"], "flattened conv output"), (enc, ENCODER_MAX["flat"], "encoding size"), (L, POSTERIOR_MAX["latent"], "latent size"),
                            (A, POSTERIOR_MAX["action"], "action size"), (Hb, POSTERIOR_MAX["belief"], "belief size"), (F, POSTERIOR_MAX["hidden"], "hidden size")):
            if not 1 <= v <= hi:
                raise UnsupportedModelError(f"{what} {v} outside [1, {hi}]" + _STOCK)
        want = {"w_embed": (Hb, L + A), "b_embed": (Hb,), "w_ih": (3 * Hb, Hb), "b_ih": (3 * Hb,), "w_hh": (3 * Hb, Hb), "b_hh": (3 * Hb,),
                "w_post1": (F, Hb + enc), "b_post1": (F,), "w_post2": (2 * L, F), "b_post2": (2 * L,)}
        if self.w_fc is not None:
            want.update(w_fc=(enc, flat), b_fc=(enc,))
        for name, shp in want.items():
            if tuple(getattr(self, name).shape) != shp:
                raise UnsupportedModelError(f"posterior tensor {name} has shape {tuple(getattr(self, name).shape)}, expected {shp}")
        lds = 64 * (max(_pad16(L + A), _pad16(F)) + max(_pad16(Hb), _pad16(2 * L)) + _pad16(Hb) + 2 * _pad16(3 * Hb) + 20)
        if lds > _LDS_LIMIT:
            raise UnsupportedModelError(f"posterior head needs {lds} bytes of LDS, the limit is {_LDS_LIMIT}" + _STOCK)
        if not self.min_std >= 0.0:
            raise UnsupportedModelError("min_std must be non-negative")


def _pair(v) -> tuple:
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def spec_from_planet_posterior(model, image_shape: Optional[Sequence[int]] = None) -> PlaNetPosteriorSpec:
    """Read a live ``mbrl.models.PlaNetModel`` (duck-typed; tensors are references to the live parameters).  ``image_shape``: (C, H, W),
    by default the model's ``obs_shape``."""
    if not (is_planet_model(model) and all(hasattr(model, a) for a in ("encoder", "posterior_transition_model"))
            and all(hasattr(model.encoder, a) for a in ("convs", "fc"))):
        raise UnsupportedModelError("not a PlaNetModel with an encoder (encoder.convs, encoder.fc) and a posterior_transition_model")
    bm, post, enc = model.belief_model, model.posterior_transition_model, model.encoder
    if type(bm.embedding_layer[1]).__name__ != "ReLU" or type(post[1]).__name__ != "ReLU":
        raise UnsupportedModelError("PlaNet heads with a non-ReLU activation have no fused implementation" + _STOCK)
    ws, bs, strides = [], [], []
    for i, layer in enumerate(enc.convs):
        conv, act = layer[0], layer[1]
        if type(act).__name__ != "ReLU":
            raise UnsupportedModelError(f"encoder activation {type(act).__name__} has no fused implementation (ReLU only)" + _STOCK)
        if _pair(conv.padding) != (0, 0) or _pair(conv.dilation) != (1, 1) or conv.groups != 1 or conv.bias is None:
            raise UnsupportedModelError(f"conv layer {i} uses padding, dilation, groups or no bias: the conv kernel has none of them" + _STOCK)
        if len(set(_pair(conv.stride))) != 1 or len(set(_pair(conv.kernel_size))) != 1:
            raise UnsupportedModelError(f"conv layer {i} has a non-square kernel or stride" + _STOCK)
        ws.append(conv.weight.detach())
        bs.append(conv.bias.detach())
        strides.append(int(_pair(conv.stride)[0]))
    fc = None if type(enc.fc).__name__ == "Identity" else enc.fc
    shape = tuple(int(v) for v in (image_shape if image_shape is not None else model.obs_shape))
    d = lambda t: t.detach()  # noqa: E731
    spec = PlaNetPosteriorSpec(
        conv_weights=ws, conv_biases=bs, strides=strides, image_shape=shape, w_fc=None if fc is None else d(fc.weight), b_fc=None if fc is None else d(fc.bias),
        w_embed=d(bm.embedding_layer[0].weight), b_embed=d(bm.embedding_layer[0].bias), w_ih=d(bm.rnn.weight_ih), b_ih=d(bm.rnn.bias_ih),
        w_hh=d(bm.rnn.weight_hh), b_hh=d(bm.rnn.bias_hh), w_post1=d(post[0].weight), b_post1=d(post[0].bias), w_post2=d(post[2].weight),
        b_post2=d(post[2].bias), min_std=float(model.min_std))
    spec.validate()
    return spec


def planet_posterior_version(spec: PlaNetPosteriorSpec) -> tuple:
    """Freshness token, ``planet_version``'s rule over the encoder, belief and posterior tensors (``PlaNetModel.update`` trains them in
    place between episodes; a detached view shares its parameter's version counter)."""
    return tuple(int(t._version) for t in spec.tensors() if t is not None)


class PlaNetPosterior:
    """``PlaNetModel.update_posterior`` for ``n_env`` environments on the device.  ``model``: a live PlaNetModel or a
    :class:`PlaNetPosteriorSpec`.  Anything the kernels cannot express raises UnsupportedModelError here, at construction."""

    def __init__(self, model, n_env: int = 1, engine: Optional[Engine] = None, image_shape: Optional[Sequence[int]] = None):
        if isinstance(model, PlaNetPosteriorSpec):
            self._live, self.spec = None, model
            model.validate()
        else:
            self._live, self.spec = model, spec_from_planet_posterior(model, image_shape)
        if not 1 <= int(n_env) <= ENCODER_MAX["env"]:
            raise ValueError(f"n_env {n_env} outside [1, {ENCODER_MAX['env']}]")
        self.n_env = int(n_env)
        dev = self.spec.w_embed.device
        self.engine = engine if engine is not None else get_engine(dev if dev.type == "cuda" else "cuda")
        dev = self.engine.device
        self.latent = torch.zeros(self.n_env, self.spec.latent_size, dtype=torch.float32, device=dev)
        self.belief = torch.zeros(self.n_env, self.spec.belief_size, dtype=torch.float32, device=dev)
        self._first = torch.ones(self.n_env, dtype=torch.uint8, device=dev)
        self._n_first = -1  # environments that start their next step from zeros; -1: reset() has not been called
        self._version = None

    def _bind(self):
        """Re-pack when a tensor changed in place or another owner sits in the engine's slot."""
        version = planet_posterior_version(self.spec)
        if version != self._version or self.engine.posterior_spec is not self.spec:
            self.engine.planet_posterior_set_model(self.spec)
            self._version = version

    def reset(self, env_ids: Optional[Sequence[int]] = None):
        """Start all environments, or only ``env_ids``, from zero latent, belief and action at their next :meth:`update`; the others
        keep their state."""
        if env_ids is None or self._n_first < 0:
            self._first.fill_(1)
        else:
            self._first[torch.as_tensor(list(env_ids), dtype=torch.long, device=self._first.device)] = 1
        self._n_first = int(self._first.sum().item()) if env_ids is not None else self.n_env
        if self._live is not None and self.n_env == 1:
            self._live.reset_posterior()

    def encode(self, obs) -> torch.Tensor:
        """The encoder's output for ``obs``, f32 [n_env, encoding_size] on the device."""
        self._bind()
        return self.engine.planet_encode(obs, self.n_env)

    def update(self, obs, action=None, rng: Optional[torch.Generator] = None, *, sample: bool = True,
               eps: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """One posterior step: ``obs`` [n_env, C, H, W] ([C, H, W] for one environment; uint8 or float32 raw pixels, numpy or torch, host or
        device), ``action`` [n_env, A] ([A] for one environment), or None straight after :meth:`reset`.  Returns {"latent": [n_env, L],
        "belief": [n_env, Hb]}, device float32.  The normals are the reference's -- one ``randn([n_env, L])`` from ``rng`` (default: the
        live model's ``rng``) -- unless ``eps`` [n_env, L] is given; ``sample=False`` returns the posterior mean and draws nothing."""
        dev = self.engine.device
        if action is None:
            if self._n_first != self.n_env:
                raise ValueError("action=None is allowed only straight after reset() (planet.py:619-624)")
        else:
            action = torch.as_tensor(action).to(device=dev, dtype=torch.float32)
            if action.ndim == 1 and self.n_env == 1:
                action = action.unsqueeze(0)
            if tuple(action.shape) != (self.n_env, self.spec.action_size):
                raise ValueError(f"action has shape {tuple(action.shape)}, expected {(self.n_env, self.spec.action_size)}")
            action = action.contiguous()
        if sample and eps is None:
            rng = rng if rng is not None else getattr(self._live, "rng", None)
            if rng is None:
                raise ValueError("update() needs rng= (a PlaNetPosteriorSpec has no generator of its own), eps= or sample=False")
            eps = planet_posterior_draws(self.spec.latent_size, self.n_env, rng)
        if eps is not None:
            eps = torch.as_tensor(eps).to(device=dev, dtype=torch.float32).reshape(self.n_env, self.spec.latent_size).contiguous()
        self._bind()
        self.engine.planet_posterior_update(obs, self.latent, self.belief, action=action, eps=eps if sample else None,
                                            first_mask=self._first if self._n_first != 0 else None)
        if self._n_first != 0:
            self._first.zero_()
            self._n_first = 0
        out = {"latent": self.latent.clone(), "belief": self.belief.clone()}
        if self._live is not None and self.n_env == 1:  # planet.py:631-637
            self._live._current_posterior_sample, self._live._current_belief = out["latent"], out["belief"]
        return out
