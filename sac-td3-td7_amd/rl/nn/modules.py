"""Host-side (torch) modules with the reference nets' interface, for ``make_nn`` callables.

A reference user builds custom nets through the agents' ``make_nn`` hook (td7.py:46,56-61,
td3.py:45,53-56, sac.py:39,47-50), typically returning ``SALEActor`` / ``SALECritic`` /
``SALEEncoder`` (rl/nn/sale.py:16-121) or ``MLPActor`` / ``MLPCritic`` (rl/nn/mlp.py:38-104)
with chosen widths.  These classes have the same constructor arguments, state_dict names and
default initialisation (rl/nn/layout.py), and the forward methods the reference's agents call.
The engine agents read the widths and the initial weights off them; training runs on the device.
"""

from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from rl.nn.layout import SALE_ACTOR, SALE_CRITIC, SALE_ENCODER, _dim


def avg_l1_norm(x: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """sale.py:11-13: x / clamp(mean |x| over the last dim, eps)."""
    return x / x.abs().mean(-1, keepdim=True).clamp(min=eps)


class _Linears(nn.Module):
    """nn.Linear layers named after a layout table (nn.Linear default initialisation)."""

    def __init__(self, table, env):
        super().__init__()
        for name, fin, fout in table:
            self.add_module(name, nn.Linear(_dim(fin, env), _dim(fout, env)))


# hidden activations the engine runs (rle_config act_*, include/rle.h RLE_ACT_*), by name
def _act_name(fn) -> str:
    """A SALE `activ` callable (sale.py:25,67,97) or a make_mlp action_fn module (mlp.py:23) -> "relu" /
    "elu" / "identity" / "leaky_relu" / "silu" / "gelu"; NotImplementedError for anything the engine does not
    run (hidden Tanh, other slopes / alphas, GELU's tanh approximation, functools.partial objects, the rest)."""
    if fn in (F.relu, torch.relu) or isinstance(fn, nn.ReLU):
        return "relu"
    if fn is F.elu or (isinstance(fn, nn.ELU) and fn.alpha == 1.0):
        return "elu"
    if isinstance(fn, nn.Identity):
        return "identity"
    if fn is F.leaky_relu or (isinstance(fn, nn.LeakyReLU) and fn.negative_slope == 0.01):
        return "leaky_relu"
    if fn is F.silu or isinstance(fn, nn.SiLU):
        return "silu"
    if fn is F.gelu or (isinstance(fn, nn.GELU) and fn.approximate == "none"):
        return "gelu"
    raise NotImplementedError(f"activation {getattr(fn, '__name__', fn)!r}: the engine runs ReLU, ELU (alpha 1), "
                              "Identity, LeakyReLU (slope 0.01), SiLU and GELU (exact)")


_LN_ONLY = ("LayerNorm runs in the critics of TD3 / SAC only, as MLPCritic(layer_norm=True): "
            "nn.LayerNorm(width, elementwise_affine=False), eps 1e-5, after every hidden Linear")


def _no_layer_norm(kind: str, layer_norm) -> None:
    if layer_norm:
        raise NotImplementedError(f"{kind}(layer_norm=...): {_LN_ONLY}")


def _check_layer_norm(layer_norm) -> bool:
    """MLPCritic's layer_norm argument -> on / off.  True, or a description of the one form the engine runs (an
    nn.LayerNorm instance or a dict of its keyword arguments): no affine parameters, eps 1e-5.  Anything else
    is NotImplementedError."""
    if layer_norm is None or layer_norm is False:
        return False
    if layer_norm is True:
        return True
    if isinstance(layer_norm, nn.LayerNorm):
        affine, eps = layer_norm.elementwise_affine, layer_norm.eps
    elif isinstance(layer_norm, dict):
        extra = set(layer_norm) - {"elementwise_affine", "eps", "bias"}
        if extra:
            raise NotImplementedError(f"layer_norm arguments {sorted(extra)}: {_LN_ONLY}")
        affine, eps = layer_norm.get("elementwise_affine", True), layer_norm.get("eps", 1e-5)
    else:
        raise NotImplementedError(f"layer_norm={layer_norm!r}: {_LN_ONLY}")
    if affine:
        raise NotImplementedError(f"an affine LayerNorm (elementwise_affine=True): {_LN_ONLY}")
    if eps != 1e-5:
        raise NotImplementedError(f"LayerNorm eps {eps}: {_LN_ONLY}")
    return True


_DROP_ONLY = ("dropout runs in the critics of TD3 / SAC only, inside their LayerNorm blocks, as "
              "MLPCritic(layer_norm=True, dropout=p) with 0 <= p < 1: Linear -> Dropout(p) -> LayerNorm -> activation "
              "in every hidden layer (dropout without LayerNorm is not run)")


def _no_dropout(kind: str, dropout) -> None:
    if dropout:
        raise NotImplementedError(f"{kind}(dropout=...): {_DROP_ONLY}")


def _check_dropout(dropout, layer_norm: bool) -> float:
    """MLPCritic's dropout argument -> p (0.0: off).  A probability in [0, 1), or None / False; p > 0 needs
    layer_norm.  Anything else is NotImplementedError (a probability outside [0, 1): ValueError)."""
    if dropout is None or dropout is False:
        return 0.0
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)):
        raise NotImplementedError(f"dropout={dropout!r}: {_DROP_ONLY}")
    p = float(dropout)
    if not 0.0 <= p < 1.0:  # (NaN fails too)
        raise ValueError(f"dropout={dropout!r}: a probability in [0, 1)")
    if p > 0.0 and not layer_norm:
        raise NotImplementedError(f"dropout={p} without layer_norm: {_DROP_ONLY}")
    return p


class NormAct(nn.Module):
    """One hidden block's LayerNorm and activation as a single Sequential slot, so the Linear layers of a
    LayerNorm critic stay at indices 0, 2, 4, ... and its state_dict names are those of a plain one (the norm has
    no parameter and no buffer).  forward: act(layer_norm(z)) -- per row mu = mean(z), var = mean((z - mu)^2),
    u = (z - mu) / sqrt(var + 1e-5), h = act(u).  dropout = p > 0 (the DroQ block): F.dropout(z, p, self.training)
    ahead of the norm -- inverted dropout in train(), nothing in eval()."""

    def __init__(self, width: int, act: nn.Module, dropout: float = 0.0):
        super().__init__()
        self.norm = nn.LayerNorm(width, elementwise_affine=False)
        self.act = act
        self.p = float(dropout)

    def forward(self, z):
        if self.p > 0.0:
            z = F.dropout(z, self.p, self.training)
        return self.act(self.norm(z))


class SALEEncoder(_Linears):
    """sale.py:16-55: zs = AvgL1Norm(zs3(elu(zs2(elu(zs1(s)))))), zsa = zsa3(elu(zsa2(elu(zsa1([zs, a])))))."""

    def __init__(self, state_dim: int, action_dim: int, zs_dim: int = 256, hdim: int = 256, activ=F.elu,
                 layer_norm=False, dropout=0.0):
        _no_layer_norm("SALEEncoder", layer_norm)
        _no_dropout("SALEEncoder", dropout)
        super().__init__(SALE_ENCODER, {"S": state_dim, "A": action_dim, "H": hdim, "Z": zs_dim})
        self.state_dim, self.action_dim, self.zs_dim, self.hdim, self.activ = state_dim, action_dim, zs_dim, hdim, activ

    def encode_state(self, state: torch.Tensor) -> torch.Tensor:
        h = self.activ(self.zs2(self.activ(self.zs1(state))))
        return avg_l1_norm(self.zs3(h))

    def encode_state_action(self, zs: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        h = self.activ(self.zsa1(torch.cat([zs, action], -1)))
        return self.zsa3(self.activ(self.zsa2(h)))


class SALEActor(_Linears):
    """sale.py:58-83: tanh(l3(relu(l2(relu(l1([AvgL1Norm(l0(s)), zs]))))))."""

    def __init__(self, state_dim: int, action_dim: int, zs_dim: int = 256, hdim: int = 256, activ=F.relu,
                 layer_norm=False, dropout=0.0):
        _no_layer_norm("SALEActor", layer_norm)
        _no_dropout("SALEActor", dropout)
        super().__init__(SALE_ACTOR, {"S": state_dim, "A": action_dim, "H": hdim, "Z": zs_dim})
        self.state_dim, self.action_dim, self.zs_dim, self.hdim, self.activ = state_dim, action_dim, zs_dim, hdim, activ

    def inference_mean(self, obs: torch.Tensor, zs: torch.Tensor) -> torch.Tensor:
        h = torch.cat([avg_l1_norm(self.l0(obs)), zs], -1)
        h = self.activ(self.l2(self.activ(self.l1(h))))
        return torch.tanh(self.l3(h))


class SALECritic(_Linears):
    """sale.py:86-121: q3(elu(q2(elu(q1([AvgL1Norm(q01([s, a])), zsa, zs])))))."""

    def __init__(self, state_dim: int, action_dim: int, zs_dim: int = 256, hdim: int = 256, activ=F.elu,
                 layer_norm=False, dropout=0.0):
        _no_layer_norm("SALECritic", layer_norm)  # (its q01 output already carries AvgL1Norm)
        _no_dropout("SALECritic", dropout)
        super().__init__(SALE_CRITIC, {"S": state_dim, "A": action_dim, "H": hdim, "Z": zs_dim})
        self.state_dim, self.action_dim, self.zs_dim, self.hdim, self.activ = state_dim, action_dim, zs_dim, hdim, activ

    def estimate_q_value(self, obs, action, zsa, zs) -> torch.Tensor:
        h = torch.cat([avg_l1_norm(self.q01(torch.cat([obs, action], -1))), zsa, zs], -1)
        return self.q3(self.activ(self.q2(self.activ(self.q1(h)))))


def _mlp(fin: int, fout: int, hidden_sizes, action_fn="ReLU", init_weight=None, init_bias=None, layer_norm=False,
         dropout=0.0):
    """make_mlp (mlp.py:10-35): Linear-act-...-Linear (indices 0, 2, 4, ...); weights by nn.init.<init_weight>
    (default xavier_normal_), biases by nn.init.<init_bias> (default zeros_).  Returns (Sequential, activation
    name).  action_fn=None is refused: make_mlp then pops the output Linear (mlp.py:34), not an activation.
    layer_norm: every hidden block is Linear-NormAct (LayerNorm, then the activation, in the activation's slot);
    dropout: the NormAct's own (ahead of its norm)."""
    if action_fn is None:
        raise NotImplementedError("make_mlp(action_fn=None) drops the output layer (mlp.py:34 pops the last Linear); "
                                  "use action_fn='Identity' for a net without activations")
    act = getattr(nn, action_fn)() if isinstance(action_fn, str) else action_fn
    name = _act_name(act)
    init_w = nn.init.xavier_normal_ if init_weight is None else getattr(nn.init, init_weight)
    init_b = nn.init.zeros_ if init_bias is None else getattr(nn.init, init_bias)
    dims = [fin] + list(hidden_sizes) + [fout]
    mods = []
    for i in range(len(dims) - 1):
        lin = nn.Linear(dims[i], dims[i + 1])
        init_w(lin.weight.data)
        init_b(lin.bias.data)
        mods += [lin, NormAct(dims[i + 1], act, dropout) if layer_norm else act]
    return nn.Sequential(*mods[:-1]), name


def _sizes(hidden_sizes):
    sizes = [hidden_sizes] * 2 if isinstance(hidden_sizes, int) else list(hidden_sizes)
    if not 2 <= len(sizes) <= 6:  # (make_mlp takes any depth, mlp.py:10-35; the engine builds 2..6, rle.h)
        raise NotImplementedError(f"hidden_sizes {sizes}: the engine builds MLPs of 2 to 6 hidden layers")
    return sizes


class MLPActor(nn.Module):
    """mlp.py:38-72: mean = mlp(s); SAC heads chunk it into (mean, log_std)."""

    def __init__(self, state_dim: int, action_dim: int, hidden_sizes=256, layer_norm=False, dropout=0.0,
                 **mlp_kwargs):
        _no_layer_norm("MLPActor", layer_norm)
        _no_dropout("MLPActor", dropout)
        super().__init__()
        self.state_dim, self.action_dim, self.hidden_sizes = state_dim, action_dim, _sizes(hidden_sizes)
        self.mlp, self.act = _mlp(state_dim, action_dim, self.hidden_sizes, **mlp_kwargs)

    def inference_mean(self, state):
        return self.mlp(state)

    def inference_mean_logvar(self, state):
        return self.mlp(state).chunk(2, -1)


class MLPCritic(nn.Module):
    """mlp.py:75-104: q = mlp([s, a]).  layer_norm=True: parameter-free LayerNorm (eps 1e-5) after every hidden
    Linear, before the activation (NormAct); the output layer is not normalised.  dropout=p with layer_norm=True: the
    DroQ critic, Linear -> Dropout(p) -> LayerNorm -> activation in every hidden layer (active in train(), as in the
    device step's passes; off in eval(), as in rle_eval)."""

    def __init__(self, state_dim: int, action_dim: int, hidden_sizes=256, layer_norm=False, dropout=0.0,
                 **mlp_kwargs):
        super().__init__()
        self.state_dim, self.action_dim, self.hidden_sizes = state_dim, action_dim, _sizes(hidden_sizes)
        self.layer_norm = _check_layer_norm(layer_norm)
        self.dropout = _check_dropout(dropout, self.layer_norm)
        self.mlp, self.act = _mlp(state_dim + action_dim, 1, self.hidden_sizes, layer_norm=self.layer_norm,
                                  dropout=self.dropout, **mlp_kwargs)

    def estimate_q_value(self, state, action):
        return self.mlp(torch.cat([state, action], -1))


def nets_from_make_nn(alg: str, make_nn, state_dim: int, action_dim: int, kwargs: dict):
    """The first five values of nets_and_settings_from_make_nn (hidden width, net shape, state_dicts, activations,
    LayerNorm): what callers from before the critics' dropout unpack."""
    return nets_and_settings_from_make_nn(alg, make_nn, state_dim, action_dim, kwargs)[:5]


def nets_and_settings_from_make_nn(alg: str, make_nn, state_dim: int, action_dim: int, kwargs: dict):
    """Call a reference-style make_nn hook (state_dim / action_dim passed as keywords, as
    annotate_make_nn does) and return six values for the engine, in this order: the hidden width, the net shape,
    {net name: numpy state_dict}, the activations, whether the critics carry LayerNorm, and the critics' dropout
    probability.  Only this module's classes (the reference's default net types) are accepted, with
    one shape across the agent's nets: (hdim, zs_dim) of the SALE nets, hidden_sizes of the MLPs
    (the shape is {"zs_dim": ...} or {"hidden_sizes": [...]}, as rle_config takes them).  The
    activations are make_config's act_actor / act_critic / act_encoder (the names _act_name returns):
    the SALE nets' `activ`, make_mlp's action_fn; the two critics must agree.  The fifth value is MLPCritic's
    layer_norm (both critics must agree; False for TD7), the sixth MLPCritic's dropout (both critics must agree;
    0.0: none)."""
    import numpy as np

    kw = dict(kwargs)
    kw["state_dim"], kw["action_dim"] = state_dim, action_dim
    out = make_nn(**kw)
    names = {"td7": ("policy", "q1", "q2", "encoder"), "td3": ("policy", "q1", "q2"),
             "sac": ("policy", "q1", "q2")}[alg]
    kinds = {"td7": (SALEActor, SALECritic, SALECritic, SALEEncoder),
             "td3": (MLPActor, MLPCritic, MLPCritic), "sac": (MLPActor, MLPCritic, MLPCritic)}[alg]
    if not isinstance(out, (tuple, list)) or len(out) != len(names):
        raise TypeError(f"make_nn must return {len(names)} nets {names}")
    widths = set()
    nets = {}
    acts = {}
    lns = set()
    drops = set()
    for name, kind, m in zip(names, kinds, out):
        if type(m) is not kind:
            raise NotImplementedError(f"make_nn returned {type(m).__name__} for {name}; the engine builds "
                                      f"rl.nn.{kind.__name__} nets only")
        role = "act_actor" if name == "policy" else "act_encoder" if name == "encoder" else "act_critic"
        act = _act_name(m.activ) if isinstance(m, (SALEActor, SALECritic, SALEEncoder)) else m.act
        if acts.setdefault(role, act) != act:
            raise NotImplementedError(f"one activation for both critics (got {acts[role]} and {act})")
        if isinstance(m, MLPCritic):
            lns.add(bool(getattr(m, "layer_norm", False)))
            drops.add(float(getattr(m, "dropout", 0.0)))
        if isinstance(m, (SALEActor, SALECritic, SALEEncoder)):
            widths.add((m.hdim, m.zs_dim))
        else:
            widths.add(tuple(m.hidden_sizes))
        want_out = 2 * action_dim if (alg == "sac" and name == "policy") else (action_dim if name == "policy" else None)
        if want_out is not None and getattr(m, "action_dim", want_out) != want_out:
            raise ValueError(f"{name}: output width {m.action_dim}, expected {want_out}")
        nets[name] = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in m.state_dict().items()}
    if len(widths) != 1:
        raise NotImplementedError(f"one net shape across the agent's nets (got {sorted(widths)})")
    if len(lns) > 1:
        raise NotImplementedError("layer_norm must be the same for both critics (got one with and one without)")
    if len(drops) > 1:
        raise NotImplementedError(f"dropout must be the same for both critics (got {sorted(drops)})")
    w = widths.pop()
    if alg == "td7":
        return w[0], {"zs_dim": w[1]}, nets, acts, False, 0.0
    return w[-1], {"hidden_sizes": list(w)}, nets, acts, bool(lns and lns.pop()), (drops.pop() if drops else 0.0)
