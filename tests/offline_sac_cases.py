"""Offline SAC (AWAC) parity cases (TEST INFRASTRUCTURE): the shapes, datasets, nets and the CPU reference that
tests/test_offline_sac.py (host) and tests/test_offline_sac_gpu.py (device) share.

A case is (S, A, hidden widths, B, seed).  Its dataset is 256 seeded transitions whose stored actions hold exact
+1, -1 and 0 entries (about an eighth of the elements each); its nets are ``oracle.spec.agent_params`` with the
policy head's bias changed so that log_std column 0 sits above ``max_log_std`` and column 1 below ``min_log_std``
for every row (both clamps closed, the remaining columns open).  The log-std bounds are [-2, 1], not the default
[-20, 2]: at sigma = e^-20 the one clamped column's (u - mu)^2 / sigma^2 ~ 1e18 would be the only thing any bound
relative to a tensor's largest element still sees.

``reference(case)`` runs ``AWACOracle`` four steps in float32 and in float64 (``edge_cases.float64_oracle``), once
per process.  ``shortfalls(a, b, n)`` lists where run ``a`` misses the criteria the engine is held to against run
``b`` -- those of tests/test_offline_td3_gpu.py and tests/harness.py: info columns rel 1e-3 (atol 1e-4), the Adam
moments after step 1 |d| <= 1e-4 |m| + 1e-4 max|m|, end parameters every element within 2 * 3e-4 * n + 1e-4 and
99% of each tensor within 1e-5.

Seeds.  Chosen on the CPU before any GPU run: 401 + the case's position; a seed at which the float32 oracle
misses the criteria against float64, or whose batches lack a +1, a -1 or a 0 action entry or a row at either
clamp, is replaced by the next of seed + 100 k that has them all (tests/test_offline_sac.py checks every case).
"""

from __future__ import annotations

import contextlib
from collections import namedtuple

import numpy as np
import torch

from oracle import agents, replay, spec

ENV = "OfflineSac-v0"
LMBDA = 0.3
MIN_LOG_STD, MAX_LOG_STD = -2.0, 1.0
N_STEPS = 4
NCAP = 256
LOSS_RTOL = 1e-3  # (tests/harness.py LOSS_RTOL; restated so that the host tests need no engine library)

Case = namedtuple("Case", "S A H hidden_sizes B seed note")

CASES = {
    "base": Case(11, 3, 32, None, 16, 401, "baseline"),
    "b17": Case(11, 3, 32, None, 17, 402, "a second row block with one valid row"),
    "b1": Case(11, 3, 32, None, 1, 403, "a single row"),
    "a24": Case(11, 24, 32, None, 17, 404, "sac_fwd_fused at its limit, 2A = 48"),
    "a25": Case(11, 25, 32, None, 17, 405, "2A = 50: the standalone rsample"),
    "h260": Case(16, 24, 260, [260, 260], 15, 406, "width % 16 != 0 and H > 256"),
}


@contextlib.contextmanager
def case_env(case):
    """oracle.spec.TASKS[ENV] = the case's (S, A, action bound 1) while the block runs."""
    c = CASES[case]
    assert ENV not in spec.TASKS
    spec.TASKS[ENV] = (c.S, c.A, 1.0)
    try:
        yield
    finally:
        del spec.TASKS[ENV]


def shape_kw(case):
    c = CASES[case]
    return {"hidden_sizes": list(c.hidden_sizes)} if c.hidden_sizes else {}


def nets(case):
    """The case's start parameters: agent_params with the policy head's log_std bias set past both clamps."""
    c = CASES[case]
    p = spec.agent_params("sac", c.S, c.A, c.H, c.seed, **shape_kw(case))
    head = max((k for k in p["policy"] if k.endswith(".bias")), key=lambda k: int(k.split(".")[1]))
    b = p["policy"][head].copy()
    assert b.shape == (2 * c.A,)
    b[c.A + 0] = MAX_LOG_STD + 3.0
    b[c.A + 1] = MIN_LOG_STD - 3.0
    p["policy"][head] = b
    return p


def dataset(case):
    """256 transitions (state, action, reward, next_state, notdone), fp32; actions in [-1, 1] with exact +1, -1
    and 0 entries."""
    c = CASES[case]
    rng = np.random.Generator(np.random.PCG64(c.seed + 1))
    a = rng.uniform(-1.0, 1.0, (NCAP, c.A)).astype(np.float32)
    pick = rng.random((NCAP, c.A))
    a[pick < 0.125] = 1.0
    a[(pick >= 0.125) & (pick < 0.25)] = -1.0
    a[(pick >= 0.25) & (pick < 0.375)] = 0.0
    return (rng.standard_normal((NCAP, c.S)).astype(np.float32), a, rng.standard_normal(NCAP).astype(np.float32),
            rng.standard_normal((NCAP, c.S)).astype(np.float32), (rng.random(NCAP) > 0.1).astype(np.float32))


def tapes(case, n=N_STEPS):
    c = CASES[case]
    return spec.tapes("sac", c.B, c.A, n, c.seed + 3)


def build_oracle(case, lmbda=LMBDA, online=False):
    """(oracle, replay) of a case: AWACOracle(lmbda), or the online SACOracle at tmp = 0 (online=True)."""
    from offline_sac_oracle import AWACOracle

    c = CASES[case]
    kw = dict(min_log_std=MIN_LOG_STD, max_log_std=MAX_LOG_STD)
    orc = agents.SACOracle(nets(case), c.A, tmp=0.0, **kw) if online else AWACOracle(nets(case), c.A, lmbda=lmbda, **kw)
    rep = replay.Replay(NCAP, c.S, c.A, np.ones(c.A, np.float32), np.zeros(c.A, np.float32), False)
    s, a, r, s2, nd = dataset(case)
    for i in range(NCAP):
        rep.append(s[i], a[i], float(r[i]), s2[i], float(nd[i]))
    return orc, rep


def _run(case, n, lmbda):
    from offline_sac_oracle import INFO_KEYS

    c = CASES[case]
    orc, rep = build_oracle(case, lmbda)
    tp = tapes(case, n)
    out = {"info": [], "ind": [], "m": None, "seen": {"+1": False, "-1": False, "0": False, "hi": False, "lo": False}}
    for t in range(n):
        i1, n1 = agents.run_steps(orc, "sac", rep, {k: v[t:t + 1] for k, v in tp.items()}, 1, c.B)
        out["info"] += i1
        out["ind"] += n1
        a, ls = orc.last["a"].numpy(), orc.last["log_std"].numpy()
        for key, hit in (("+1", (a == 1.0).any()), ("-1", (a == -1.0).any()), ("0", (a == 0.0).any()),
                         ("hi", (ls > MAX_LOG_STD).any()), ("lo", (ls < MIN_LOG_STD).any())):
            out["seen"][key] = out["seen"][key] or bool(hit)
        if t == 0:
            out["m"] = dict(agents.moments(orc))
    out["table"] = np.array([[i[k] for k in INFO_KEYS] for i in out["info"]], np.float64)
    out["params"] = {(net, k): v.detach().numpy().copy() for net, d in orc.nets().items() for k, v in d.items()}
    return out


_REF = {}


def reference(case, n=N_STEPS, lmbda=LMBDA):
    """{"f32": run, "f64": run, "tp": tapes} of a case, computed once and shared (read-only)."""
    key = (case, n, lmbda)
    if key not in _REF:
        from edge_cases import float64_oracle

        torch.set_num_threads(1)
        f32 = _run(case, n, lmbda)
        with float64_oracle():
            f64 = _run(case, n, lmbda)
        _REF[key] = {"f32": f32, "f64": f64, "tp": tapes(case, n)}
    return _REF[key]


def moment_shortfalls(got, ref):
    """got(key) -> array; ref: {key: array}.  The step-1 Adam-moment bound, every m and v tensor."""
    bad = []
    for key, m in ref.items():
        r = np.asarray(m, np.float64)
        d = np.abs(np.asarray(got(key), np.float64).reshape(r.shape) - r)
        lim = 1e-4 * np.abs(r) + 1e-4 * max(np.abs(r).max(), 1e-30)
        if not (d <= lim).all():
            bad.append(("moment", key, float(d.max()), float((d / lim).max())))
    return bad


def end_shortfalls(table, get_param, ref, n):
    """Info columns and end parameters of a run against the reference run `ref`."""
    bad = []
    table = np.asarray(table, np.float64)
    if table.shape != ref["table"].shape or not np.allclose(table, ref["table"], rtol=LOSS_RTOL, atol=1e-4):
        bad.append(("info", table.tolist(), ref["table"].tolist()))
    tol = 2 * 3e-4 * n + 1e-4
    for (net, name), v in ref["params"].items():
        d = np.abs(np.asarray(get_param(net, name), np.float64).reshape(v.shape) - v)
        if d.max() > tol:
            bad.append(("param", net, name, float(d.max())))
        if (d <= 1e-5).mean() < 0.99:
            bad.append(("bulk", net, name, float((d <= 1e-5).mean())))
    return bad


def shortfalls(a, b, n):
    """Where oracle run `a` misses the engine's criteria against oracle run `b` (empty: it meets them)."""
    bad = [("ind", t) for t in range(n) if not np.array_equal(a["ind"][t], b["ind"][t])]
    bad += moment_shortfalls(lambda k: a["m"][k], b["m"])
    bad += end_shortfalls(a["table"], lambda net, name: a["params"][(net, name)], b, n)
    return bad
