"""Generate the LeakyReLU / SiLU / GELU goldens by running the REFERENCE itself (build container only).

Usage (from the repo root, in the build container where the reference exists):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_more_acts.py [name ...]

``make_golden`` is imported unchanged; the three activations are added to its ``SALE_ACTIV`` /
``MLP_ACTION_FN`` tables at run time (the reference takes any ``activ`` callable, sale.py:25,67,97, and any
``torch.nn`` name as make_mlp's ``action_fn``, mlp.py:13,23), and ``run_config`` writes nine tiny goldens
shaped like the ``*_tiny_act`` ones: Tiny-v0, H 32, B 16, capacity 64, fill 50, 6 to 8 steps.  Each
activation is seen in every role (actor / critic / encoder) once per algorithm.

Nothing here runs on the GPU box; only the .npz files travel.
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

_names = sys.argv[1:]
sys.argv = sys.argv[:1]  # (make_golden reads its ONLY filter off sys.argv at import)
import make_golden as mg  # noqa: E402

import torch.nn.functional as F  # noqa: E402

mg.ONLY = set(_names)
mg.SALE_ACTIV.update({"leaky_relu": F.leaky_relu, "silu": F.silu, "gelu": F.gelu})
mg.MLP_ACTION_FN.update({"leaky_relu": "LeakyReLU", "silu": "SiLU", "gelu": "GELU"})


def main():
    run = mg.run_config
    # TD7: a with LAP and a hard update inside the trajectory (target_update_rate 4 of 8 steps), b without LAP
    run("td7_tiny_acts_a", "td7", "Tiny-v0", 32, 16, 64, 50, 8, True, 51, extra={"target_update_rate": 4},
        acts={"actor": "silu", "critic": "gelu", "encoder": "leaky_relu"})
    run("td7_tiny_acts_b", "td7", "Tiny-v0", 32, 16, 64, 50, 6, False, 52, extra={"target_update_rate": 3},
        acts={"actor": "gelu", "critic": "leaky_relu", "encoder": "silu"})
    run("td7_tiny_acts_c", "td7", "Tiny-v0", 32, 16, 64, 50, 8, True, 53, extra={"target_update_rate": 4},
        acts={"actor": "leaky_relu", "critic": "silu", "encoder": "gelu"})
    run("td3_tiny_acts_a", "td3", "Tiny-v0", 32, 16, 64, 50, 6, True, 54, acts={"actor": "silu", "critic": "gelu"})
    run("td3_tiny_acts_b", "td3", "Tiny-v0", 32, 16, 64, 50, 6, False, 55,
        acts={"actor": "gelu", "critic": "leaky_relu"})
    run("td3_tiny_acts_c", "td3", "Tiny-v0", 32, 16, 64, 50, 6, False, 56,
        acts={"actor": "leaky_relu", "critic": "silu"})
    # SAC: a with the automatic temperature and three unequal hidden layers, b with a fixed temperature
    run("sac_tiny_acts_a", "sac", "Tiny-v0", 32, 16, 64, 50, 6, False, 57,
        acts={"actor": "silu", "critic": "gelu"}, shape={"hidden_sizes": [32, 48, 32]})
    run("sac_tiny_acts_b", "sac", "Tiny-v0", 32, 16, 64, 50, 6, False, 58, extra={"tmp": 0.2},
        acts={"actor": "gelu", "critic": "leaky_relu"})
    run("sac_tiny_acts_c", "sac", "Tiny-v0", 32, 16, 64, 50, 6, False, 59,
        acts={"actor": "leaky_relu", "critic": "silu"})


if __name__ == "__main__":
    main()
