"""Gradient-norm clipping cases (TEST INFRASTRUCTURE): shape edges with a ``max_norm``.

A case is a source case -- a shape edge of tests/edge_cases.py, the "edge_odd" shape of
tests/test_offline_td3_gpu.py (offline TD3, alpha 2.5) or "b17" of tests/offline_sac_cases.py (AWAC) -- at the
source's own seed, plus the threshold every optimizer of a step is clipped to (tests/grad_clip_oracle.py).
``registered(name)`` puts an edge case into edge_cases' table while a test runs, as tests/more_acts.py does, so
the sweep's own engine builders take it as one of theirs.

The thresholds were chosen on the float32 CPU oracle before any GPU run, so that every case has a clipped update
(coef < 1) and the "mixed" ones also an unclipped one (coef == 1); tests/test_grad_clip.py asserts that from
the oracle's log.  ``total`` below is the unclipped float32 oracle's range over the case's steps (under
clipping it moves by a few percent at most: Adam is nearly scale-invariant):

    case             source, max_norm     critics total -> coef         policy             encoder
    clip-td7-odd     td7-odd, 0.8         0.65-0.90 -> 0.89-1 (mixed)   0.06-0.07 -> 1     0.87-0.97 -> 0.82-0.92
    clip-td7-b1      td7-b1, 2.0          1.35-5.8 -> 0.35-1 (mixed)    -> 1               1.2-2.2 -> 0.91-1
    clip-td7-odd_bc  td7-odd_bc, 0.05     -> 0.06-0.08                  0.07 -> 0.66-0.71  -> 0.05
    clip-td3-k49     td3-k49, 0.3         0.24-0.53 -> 0.57-1 (mixed)   -> 1
    clip-td3-deep6   td3-deep6, 0.1       0.036-0.31 -> 0.32-1 (mixed)  -> 1
    clip-td3-min     td3-min, 1.0         0.62-2.9 -> 0.35-1 (mixed)    -> 1
    clip-sac-a25     sac-a25, 10          16-27 -> 0.37-0.61            4.8-5.5 -> 1
    clip-sac-h260    sac-h260, 7          45-51 -> 0.14-0.16            9.5-10.3 -> 0.68-0.74
    clip-td3bc-odd   edge_odd (TD3+BC), 0.3  0.41-0.74 -> 0.40-0.74        1.2-1.9 -> 0.16-0.25
    clip-awac-b17    b17 (AWAC), 0.3      0.52-0.62 -> 0.49-0.57        39-206 -> 0.001-0.008

For the two offline cases max_norm is half the median unclipped critics' total over the case's steps, rounded to
one digit (tests/test_grad_clip.py recomputes it from the unclipped oracle).  Every case met the host criteria
(float32 against float64 oracle) at its source's seed: none was reseeded.
"""

from __future__ import annotations

import contextlib
from collections import namedtuple

import numpy as np
import torch

import edge_cases as EC
import grad_clip_oracle as GO
from oracle import agents, spec

ClipCase = namedtuple("ClipCase", "kind src max_norm mixed")

TD3BC_ALPHA = 2.5
TD3BC_SHAPE = (33, 5, 36, 31, True, 304)  # tests/test_offline_td3_gpu.py EDGES["edge_odd"]: S, A, H, B, use_lap, seed
TD3BC_STEPS = 5
TD3BC_NORM = 0.3   # unclipped critics' total 0.41-0.74 over the 5 steps, median 0.653
AWAC_NORM = 0.3    # unclipped critics' total 0.52-0.62 over the 4 steps, median 0.579

CLIP_CASES = {
    "clip-td7-odd": ClipCase("edge", "td7-odd", 0.8, True),
    "clip-td7-b1": ClipCase("edge", "td7-b1", 2.0, True),
    "clip-td7-odd_bc": ClipCase("edge", "td7-odd_bc", 0.05, False),
    "clip-td3-k49": ClipCase("edge", "td3-k49", 0.3, True),
    "clip-td3-deep6": ClipCase("edge", "td3-deep6", 0.1, True),
    "clip-td3-min": ClipCase("edge", "td3-min", 1.0, True),
    "clip-sac-a25": ClipCase("edge", "sac-a25", 10.0, False),
    "clip-sac-h260": ClipCase("edge", "sac-h260", 7.0, False),
    "clip-td3bc-odd": ClipCase("td3bc", "edge_odd", TD3BC_NORM, False),
    "clip-awac-b17": ClipCase("awac", "b17", AWAC_NORM, False),
}


def alg_of(name):
    c = CLIP_CASES[name]
    return EC.CASES[c.src].alg if c.kind == "edge" else {"td3bc": "td3", "awac": "sac"}[c.kind]


@contextlib.contextmanager
def registered(name):
    """edge_cases.CASES[name] = the source edge case (its shape and seed) while the block runs."""
    c = CLIP_CASES[name]
    assert c.kind == "edge" and name not in EC.CASES
    EC.CASES[name] = EC.CASES[c.src]
    try:
        yield EC.CASES[name]
    finally:
        del EC.CASES[name]


def td3bc_golden():
    S, A, H, B, lap, seed = TD3BC_SHAPE
    return {"meta_alg": np.array("td3"), "meta_env": np.array("edge_odd"),
            "meta": np.array([H, B, 256, 200, 0, int(lap), seed]),
            "meta_extra_keys": np.array([], dtype="<U32"), "meta_extra_vals": np.array([], np.float64)}


@contextlib.contextmanager
def td3bc_env():
    S, A = TD3BC_SHAPE[:2]
    assert "edge_odd" not in spec.TASKS
    spec.TASKS["edge_odd"] = (S, A, 1.0)
    try:
        yield
    finally:
        del spec.TASKS["edge_odd"]


def td3bc_tapes(n=TD3BC_STEPS):
    S, A, H, B, lap, seed = TD3BC_SHAPE
    rng = np.random.default_rng(9000 + seed)  # (tests/test_offline_td3_gpu.py _tapes)
    return {"u": rng.random((n, B), dtype=np.float32), "eps": rng.standard_normal((n, B, A), dtype=np.float32)}


def build(name):
    """(oracle, replay, tapes, n_steps, B, alg, info keys, use_lap) of a case, unclipped."""
    c = CLIP_CASES[name]
    if c.kind == "edge":
        from offline_oracle import build_offline
        from test_oracle import build_from_golden

        e = EC.CASES[c.src]
        g = EC.golden(c.src)
        with EC.edge_env(c.src):
            if e.bc_lambda:
                orc, rep, tp, n, B = build_offline(g, e.bc_lambda)
            else:
                _, orc, rep, tp, n, B = build_from_golden(g)
        return orc, rep, tp, n, B, e.alg, EC.info_keys(c.src), e.use_lap
    if c.kind == "td3bc":
        from offline_td3_oracle import INFO_KEYS, build_offline_td3

        with td3bc_env():
            orc, rep, _, _, B = build_offline_td3(td3bc_golden(), TD3BC_ALPHA)
        return orc, rep, td3bc_tapes(), TD3BC_STEPS, B, "td3", INFO_KEYS, TD3BC_SHAPE[4]
    import offline_sac_cases as SC
    from offline_sac_oracle import INFO_KEYS

    orc, rep = SC.build_oracle(c.src)
    return orc, rep, SC.tapes(c.src), SC.N_STEPS, SC.CASES[c.src].B, "sac", INFO_KEYS, False


@contextlib.contextmanager
def float64_oracle():
    """edge_cases.float64_oracle, and the offline TD3 oracle's own copy of the batch-tensor constructor with it."""
    import offline_td3_oracle

    with EC.float64_oracle():
        saved = offline_td3_oracle._tt
        offline_td3_oracle._tt = agents._tt
        try:
            yield
        finally:
            offline_td3_oracle._tt = saved


def run(name, max_norm):
    """One oracle run of a case clipped to ``max_norm`` (inf: unclipped, the log then holds the totals): the info
    table, indices, priorities, TD7 value bounds, the Adam moments (m and v) after step 1 -- and after step 2,
    where TD7's policy optimizer first steps -- the end parameters and the per-step clip log."""
    orc, rep, tp, n, B, alg, keys, lap = build(name)
    log = GO.clip(orc, max_norm)
    out = {"info": [], "ind": [], "prio": [], "vb": [], "m": None, "m2": None, "log": []}
    for t in range(n):
        k0 = len(log)
        i1, n1 = agents.run_steps(orc, alg, rep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
        out["info"] += i1
        out["ind"] += n1
        out["log"].append(list(log[k0:]))
        out["prio"].append(rep.priority.copy() if lap else None)
        if alg == "td7":
            out["vb"].append(np.array([orc.value_max, orc.value_min, orc.vt_max, orc.vt_min], np.float64))
        if t == 0:
            out["m"] = {k: v for k, v in agents.moments(orc).items() if not k.startswith("tmp.")}
        if t == 1 and alg == "td7":
            out["m2"] = {k: v for k, v in agents.moments(orc).items() if k.startswith("policy.")}
    out["table"] = np.array([[np.nan if i[k] is None else i[k] for k in keys] for i in out["info"]], np.float64)
    out["params"] = {(net, k): v.detach().numpy().copy() for net, d in orc.nets().items() for k, v in d.items()}
    if alg == "sac":
        out["log_alpha"] = orc.log_alpha.detach().numpy().copy()
    out["n"], out["keys"] = n, keys
    return out


_REF = {}


def reference(name):
    """{"f32", "f64": the clipped runs, "plain": the unclipped float32 run} of a case, computed once, shared."""
    if name not in _REF:
        torch.set_num_threads(1)
        c = CLIP_CASES[name]
        f32 = run(name, c.max_norm)
        plain = run(name, float("inf"))
        with float64_oracle():
            f64 = run(name, c.max_norm)
        _REF[name] = {"f32": f32, "f64": f64, "plain": plain}
    return _REF[name]


def stats_after(run_, t):
    """rle_grad_clip_stats' six numbers after step t + 1 of an oracle run: the last (total, coef) of each optimizer."""
    last = {}
    for step in run_["log"][:t + 1]:
        for name, total, coef in step:
            last[name] = (total, coef)
    return np.array([x for k in GO.ORDER for x in last.get(k, (np.nan, np.nan))], np.float64)


def moment_shortfalls(got, ref):
    """got(key) -> array; ref: {"net.param:m|v": array}.  The moment bound of DESIGN "Oracle and parity": every
    element within 1e-4 |ref| + 1e-4 max |ref| of its tensor."""
    bad = []
    for key, m in ref.items():
        r = np.asarray(m, np.float64)
        d = np.abs(np.asarray(got(key), np.float64).reshape(r.shape) - r)
        lim = 1e-4 * np.abs(r) + 1e-4 * max(np.abs(r).max(), 1e-30)
        if not (d <= lim).all():
            bad.append((key, float(d.max()), float((d / lim).max())))
    return bad
