"""Cases, tolerances and CPU references of the random-stream tests (TEST INFRASTRUCTURE).

Shared by tests/test_rng_streams.py (CPU) and tests/test_rng_streams_gpu.py.  Every case is a Tiny-sized agent
(S 11, A 3, H 32) on a replay of 300 rows -- not a power of two -- whose engine seed (``cfg_seed``, the Philox key)
is chosen independently of the seed of its parameters and data (``pseed``).

``DELTA`` bounds |device normal - float64 Box-Muller| (DESIGN.md "Random streams"): 4 x the largest distance
measured over every draw of tests/test_rng_streams_gpu.py's direct read-outs.  ``reference(case)`` derives the
info tolerance ``T`` of the engine-against-engine test from it on the CPU oracle alone: a same-sign jitter of
DELTA on every eps / eps_pi element moves the info entries by ``r`` (relative); ``T = max(10 r, 1e-6)``.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import philox_ref as P
from oracle import agents, spec

ENV = "Tiny-v0"
S, A, _HI = spec.TASKS[ENV]
H = 32
NCAP = 300  # capacity = fill

# The largest |device - float64| over the 144,000 exploration draws and 10,500 fill draws of the GPU tests, on an
# MI355X: a fill_random state of +3.972347 (u1 0.000371456146, u2 0.00516319275; the act draws: 4.34e-7 at u1
# 0.00657212734, u2 0.988858402, a draw of +3.162383).  Two float32 ulp of a draw between 2 and 4; the margin of 4
# is for seeds that land elsewhere (a draw past 4 has twice the ulp).  A wrong draw is off by O(1).
MEASURED_DELTA = 4.76e-7
DELTA = 4 * MEASURED_DELTA
# SAC's draw is read back through tanh(eps * exp(-4)): out = tanhf(fl(eps * expf(-4))) with |out| <= 0.106, where
# one float32 ulp is 7.5e-9.  Two ulp of tanhf and the half ulp of the product, through atanh' <= 1.012 and the
# factor e^4 = 54.6, give 1.0e-6; two ulp of expf(-4) give 2.4e-7 |eps| <= 1.4e-6: 2.4e-6, rounded up to 4e-6.
SAC_READOUT = 4e-6

Case = namedtuple("Case", "alg B cfg_seed pseed n_steps use_lap extra")

_NOISE = {"target_policy_noise": 0.5, "noise_clip": 1.0}  # (twice the defaults: the smoothing noise weighs more)
CASES = {
    "td3-b17": Case("td3", 17, (1 << 40) | 12345, 31, 6, False, dict(_NOISE)),
    "td3-b32": Case("td3", 32, (0xC0FFEE << 32) | 7, 32, 6, False, dict(_NOISE)),
    # TD7: hard updates after steps 3 and 6 -- the smoothing noise reaches the losses from step 4 on
    "td7-b17": Case("td7", 17, (0x9E3779B9 << 32) | 0x80000001, 33, 7, True, dict(_NOISE, target_update_rate=3)),
    "td7-b32": Case("td7", 32, (1 << 63) | 5, 34, 7, True, dict(_NOISE, target_update_rate=3)),
    "sac-b17": Case("sac", 17, (3 << 32) | 0xFFFFFFFF, 35, 5, False, {}),
    "sac-b32": Case("sac", 32, (1 << 40) | 12345, 36, 5, False, {}),
}

INFO_KEYS = {"td7": ("train/encoder", "train/q_fn", "train/policy"),
             "td3": ("train/q_fn", "train/policy", "norm/policy"),
             "sac": ("train/q_fn", "tmp", "norm/tmp", "train/policy", "train/tmp", "entropy")}


def golden(case):
    """The synthetic golden (tests/test_engine_gpu.py _synthetic_golden's layout) of a case's parameters, data
    and hyper-parameters; it holds no tapes -- the draws come from philox_ref."""
    c = CASES[case]
    return {"meta_alg": np.array(c.alg), "meta_env": np.array(ENV),
            "meta": np.array([H, c.B, NCAP, NCAP, c.n_steps, int(c.use_lap), c.pseed]),
            "meta_extra_keys": np.array(list(c.extra), dtype="<U32"),
            "meta_extra_vals": np.array(list(c.extra.values()), np.float64)}


def ref_tapes(case, step0=0):
    c = CASES[case]
    return P.tapes(c.alg, c.cfg_seed, step0, c.n_steps, c.B, A)


def build_engine(case, plan=None):
    """(engine, replay) of a case (a name of CASES, or a Case): harness.engine_from_golden with the engine seed
    set apart."""
    from harness import ALGO, fill_replay
    from rl import _engine as E

    c = CASES[case] if isinstance(case, str) else case
    cfg = E.make_config(ALGO[c.alg], S, A, H, c.B, use_lap=c.use_lap, seed=c.cfg_seed, **c.extra)
    eng = E.Engine(cfg, plan)
    for net, params in spec.agent_params(c.alg, S, A, H, c.pseed).items():
        for name, v in params.items():
            eng.set_param(net, name, v)
    rep = E.Replay(NCAP, S, A, c.use_lap)
    fill_replay(rep, S, A, _HI, NCAP, c.pseed)
    if c.use_lap:
        p0 = spec.init_priorities(NCAP, c.pseed + 2)
        rep.set_priority(p0, float(p0.max()))
    eng.bind(rep)
    return eng, rep


def oracle_table(case, tp):
    """The float32 CPU oracle on tapes ``tp``: the per-step info table [n_steps, len(INFO_KEYS)], float64
    (NaN where a step logs nothing)."""
    from test_oracle import build_from_golden

    c = CASES[case]
    torch.set_num_threads(1)
    _, orc, rep, _, n, B = build_from_golden(golden(case))
    infos, _ = agents.run_steps(orc, c.alg, rep, tp, n, B)
    return np.array([[np.nan if i[k] is None else i[k] for k in INFO_KEYS[c.alg]] for i in infos], np.float64)


def rel_move(table, ref):
    """Largest relative distance of an info entry from the reference's (entries both NaN: none)."""
    assert np.array_equal(np.isnan(table), np.isnan(ref))
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(table - ref) / np.abs(ref)))


def mutations(case, tp):
    """Tapes with one wrong noise stream each: {name: tapes}.  ``roll``: a step's draws are the next step's;
    ``shift``: every draw is its neighbour's (row-major, within the step); ``flip``: columns reversed; for SAC
    the same of eps_pi, and ``swap``: eps and eps_pi exchanged."""
    out = {}
    for key in ("eps", "eps_pi") if "eps_pi" in tp else ("eps",):
        e = tp[key]
        n = e.shape[0]
        for name, m in (("roll", np.roll(e, -1, axis=0)), ("shift", np.roll(e.reshape(n, -1), 1, axis=1).reshape(e.shape)),
                        ("flip", e[:, :, ::-1])):
            out[f"{key}-{name}"] = dict(tp, **{key: np.ascontiguousarray(m)})
    if "eps_pi" in tp:
        out["swap"] = dict(tp, eps=tp["eps_pi"], eps_pi=tp["eps"])
    return out


_REF = {}


def reference(case):
    """{"tapes", "table" (the oracle on them), "r", "T"} of a case, computed once and shared (read-only)."""
    if case not in _REF:
        tp = ref_tapes(case)
        table = oracle_table(case, tp)
        jit = {k: (v + np.float32(DELTA) if k != "u" else v) for k, v in tp.items()}
        r = rel_move(oracle_table(case, jit), table)
        _REF[case] = {"tapes": tp, "table": table, "r": r, "T": max(10 * r, 1e-6)}
    return _REF[case]
