"""LayerNorm critics (TEST INFRASTRUCTURE): ``Linear -> LayerNorm -> activation`` in every hidden layer of the
TD3 / SAC critics, as a composite activation of the CPU oracle.

``oracle.agents`` resolves a golden's ``meta_acts`` through ``oracle.nets.ACTS`` and applies the callable after
every hidden ``Linear``.  Importing this module registers ``"ln_<act>"`` there for every activation the engine
runs -- ``act(F.layer_norm(x, x.shape[-1:]))``: no affine parameters, eps 1e-5, torch's defaults -- so the oracle
with critic ``"ln_relu"`` IS a LayerNorm critic; oracle/ itself does not change, and edge_cases.float64_oracle()
works on it as it stands.  tests/test_layer_norm.py pins the composite bitwise to rl.nn.MLPCritic(layer_norm=True).

``LN_CASES`` are shape edges of tests/edge_cases.py run again with such a critic: the smallest shapes at which the
row ops' masks and passes can go wrong.  ``registered(name)`` puts a case into edge_cases' tables while a test runs
(as tests/more_acts.py does); ``registered(name, engine=True)`` also swaps the sweep's engine builder
(tests/test_shape_edges_gpu.py ``_engine``) for one that strips the ``ln_`` prefix from the activation it
hands rle_create and calls ``set_layer_norm(True)``, so the sweep's own body, ``check_trains_like_the_oracle``,
runs on the case with its own criteria.
"""

from __future__ import annotations

import contextlib

import numpy as np
import torch.nn.functional as F

import edge_cases as EC
import more_acts  # noqa: F401  (registers leaky_relu / silu / gelu)
from oracle import nets as N

PREFIX = "ln_"


def _composite(act):
    return lambda x: act(F.layer_norm(x, x.shape[-1:]))


for _name in ("relu", "elu", "identity", "leaky_relu", "silu", "gelu"):
    N.ACTS[PREFIX + _name] = _composite(N.ACTS[_name])

# name -> (source case of edge_cases.CASES, critic composite, {"actor": ...} beyond the default, seed).  Seeds:
# 501 + the case's position, fixed before the engine ran any of them; every case meets the host criteria of
# tests/test_shape_edges.py (float32 oracle against float64) at that seed (tests/test_layer_norm.py).  A case that
# stops doing so takes the first of seed + 100 k that meets them.
LN_CASES = {
    "ln-td3-min": ("td3-min", "ln_relu", {}, 501),        # one lane, one valid row of 16
    "ln-td3-k49": ("td3-k49", "ln_relu", {}, 502),        # 20 of 32 columns live, 1 masked row, LAP
    "ln-td3-deep6": ("td3-deep6", "ln_elu", {}, 503),     # six unequal widths, three row blocks
    "ln-sac-h260": ("sac-h260", "ln_relu", {}, 504),      # second float4 pass with one live lane
    "ln-sac-a25": ("sac-a25", "ln_gelu", {}, 505),        # run-time activation on u, stand-alone rsample
    "ln-sac-min": ("sac-min", "ln_relu", {}, 506),        # auto temperature at the minimum
    "ln-td3-w100": ("td3-w100", "ln_identity", {}, 507),  # LN with no activation, 112 padded rows
}


def meta_acts(critic, actor="default"):
    return np.array([actor, critic, "default"])


def strip(g):
    """The golden the engine is built from: the critic's composite replaced by its plain activation."""
    g = dict(g)
    acts = [str(v) for v in g["meta_acts"]]
    assert acts[1].startswith(PREFIX), acts
    acts[1] = acts[1][len(PREFIX):]
    g["meta_acts"] = np.array(acts)
    return g


def ln_engine(g, plan=None, build=None):
    """engine_from_golden (or ``build``) on strip(g), with the critics' LayerNorm switched on: (engine, replay)."""
    from harness import engine_from_golden

    out = (build or engine_from_golden)(strip(g), plan=plan)
    eng, rep = out[0], out[1]
    eng.set_layer_norm(True)
    assert eng.layer_norm()
    return eng, rep


@contextlib.contextmanager
def registered(name, engine=False):
    """edge_cases.CASES[name] and a golden(name) carrying the composite, while the block runs; engine=True: the
    GPU sweep's ``_engine`` builds LayerNorm engines for the registered case."""
    src, critic, more, seed = LN_CASES[name]
    assert name not in EC.CASES
    plain = EC.golden

    def golden(case):
        g = plain(case)
        if case in LN_CASES:
            g["meta_acts"] = meta_acts(LN_CASES[case][1], LN_CASES[case][2].get("actor", "default"))
        return g

    EC.CASES[name] = EC.CASES[src]._replace(seed=seed)
    EC.golden = golden
    sweep = plain_engine = None
    if engine:
        import test_shape_edges_gpu as sweep

        plain_engine = sweep._engine

        def _engine(case, plan=None, g=None):
            if case not in LN_CASES:
                return plain_engine(case, plan, g)
            g = EC.reference(case)["g"] if g is None else g
            with EC.edge_env(case):
                return ln_engine(g, plan)

        sweep._engine = _engine
    try:
        yield EC.CASES[name]
    finally:
        if engine:
            sweep._engine = plain_engine
        EC.golden = plain
        del EC.CASES[name]


def reference(name):
    """edge_cases.reference of an LN_CASES entry (float32 and float64 oracle runs, computed once, shared)."""
    with registered(name):
        return EC.reference(name)
