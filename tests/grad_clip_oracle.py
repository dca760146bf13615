"""Global gradient-norm clipping on the CPU oracles (TEST INFRASTRUCTURE).

``clip(oracle, max_norm)`` wraps the ``step`` of every ``oracle.agents.Adam`` that clips in a gradient step --
``opt_q`` (q1 + q2, one optimizer), ``opt_pi`` and TD7's ``opt_enc``; never SAC's temperature ``opt_t`` -- with
torch.nn.utils.clip_grad_norm_'s law (error_if_nonfinite False) on the gradients it is handed:

    total = norm of the per-tensor L2 norms,  coef = min(1, max_norm / (total + 1e-6)),  g <- g * coef

(multiplied also when coef == 1, as torch does) and appends ``(optimizer, total, coef)`` to the returned log, in
the order the optimizers step.  It works on the online oracles and on the offline test oracles alike (they
inherit the optimizers), in whatever precision the oracle runs; oracle/ itself does not change.  TD3's
``norm/policy`` is computed before ``opt_pi.step`` is called (oracle/agents.py), so it stays the norm before
clipping.  tests/test_grad_clip.py pins ``clipped`` bitwise to torch.nn.utils.clip_grad_norm_.
"""

from __future__ import annotations

import torch

NAMES = {"opt_q": "critics", "opt_pi": "policy", "opt_enc": "encoder"}
ORDER = ("critics", "policy", "encoder")  # rle_grad_clip_stats' order


def clipped(grads, max_norm):
    """(the clipped gradients, total, coef) -- clip_grad_norm_(norm_type=2, foreach=False) without the in-place write."""
    grads = [g.detach() for g in grads]
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in grads]), 2.0)
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return [g * coef for g in grads], total, coef


def clip(oracle, max_norm):
    """Wrap the oracle's optimizers in place; returns the log list the wrapped steps append to."""
    log = []
    for attr, name in NAMES.items():
        opt = getattr(oracle, attr, None)
        if opt is None:
            continue

        def step(grads, _opt=opt, _name=name, _plain=opt.step):
            gs, total, coef = clipped(list(grads), max_norm)
            log.append((_name, float(total), float(coef)))
            return _plain(gs)

        opt.step = step
    return log
