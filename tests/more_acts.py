"""LeakyReLU / SiLU / GELU as hidden activations (TEST INFRASTRUCTURE).

Importing this module registers the three torch functions under the names rle_config's act_* strings use
("leaky_relu", "silu", "gelu": torch's defaults -- slope 0.01, the exact erf GELU) in ``oracle.nets.ACTS``,
the table the oracle resolves a golden's ``meta_acts`` through; oracle/ itself does not change.  The nine
``*_tiny_acts_*`` goldens (tests/golden/make_golden_more_acts.py) pin these callables to the reference's modules.

``ACT_CASES`` are the shape edges of tests/edge_cases.py run again with the new activations: the smallest
shapes at which one of their paths (the loss head fused into a DX at a width that pads, the stand-alone head,
one valid row, H > 256, six unequal layers) can go wrong.  A case is its source case with another seed and a
``meta_acts`` entry in its golden; ``registered(name)`` puts it into edge_cases' tables while a test runs, so
edge_cases.reference and the sweep's own test bodies take it as one of theirs, and takes it out again.
"""

from __future__ import annotations

import contextlib

import torch.nn.functional as F

import edge_cases as EC
from oracle import nets as N

N.ACTS.update({"leaky_relu": F.leaky_relu, "silu": F.silu, "gelu": F.gelu})

NAMES = ("leaky_relu", "silu", "gelu")
GOLDENS = [f"{alg}_tiny_acts_{v}" for alg in ("td7", "td3", "sac") for v in "abc"]

# name -> (source case of edge_cases.CASES, {"actor" / "critic" / "encoder": name}, seed).  Seeds: 301 + the
# case's position, fixed before the engine ran any of them; a case that misses the host criteria of
# tests/test_shape_edges.py (float32 oracle against float64) at its seed takes the first of seed + 100 k that
# meets them (DESIGN "More hidden activations" lists those).
ACT_CASES = {
    "acts-td3-k49": ("td3-k49", {"critic": "gelu", "actor": "silu"}, 301),
    "acts-td7-odd": ("td7-odd", {"critic": "silu", "encoder": "gelu", "actor": "leaky_relu"}, 302),
    "acts-td7-b1": ("td7-b1", {"critic": "gelu"}, 303),
    # (404: at 304 one of 67,600 policy mlp.2 weights ends 1.09e-5 from float64 after 4 steps, past the 1e-5)
    "acts-sac-h260": ("sac-h260", {"critic": "leaky_relu", "actor": "gelu"}, 404),
    "acts-sac-a25": ("sac-a25", {"actor": "silu"}, 305),
    "acts-td3-deep6": ("td3-deep6", {"actor": "silu", "critic": "silu"}, 306),
}


@contextlib.contextmanager
def registered(name):
    """edge_cases.CASES[name] and a golden(name) carrying the case's activations, while the block runs."""
    import numpy as np

    src, acts, seed = ACT_CASES[name]
    assert name not in EC.CASES
    plain = EC.golden

    def golden(case):
        g = plain(case)
        if case in ACT_CASES:
            g["meta_acts"] = np.array([ACT_CASES[case][1].get(k, "default") for k in ("actor", "critic", "encoder")])
        return g

    EC.CASES[name] = EC.CASES[src]._replace(seed=seed)
    EC.golden = golden
    try:
        yield EC.CASES[name]
    finally:
        EC.golden = plain
        del EC.CASES[name]


def reference(name):
    """edge_cases.reference of an ACT_CASES entry (float32 and float64 oracle runs, computed once, shared)."""
    with registered(name):
        return EC.reference(name)
