"""Shape-edge cases over the config domain rle_create accepts (TEST INFRASTRUCTURE).

One table of named cases, each the smallest shape at which one of the step builder's switches
(engine.cpp actor_pre, sac_fwd_fused / sac_pre, td7_headdx, mlp_headdx, td7_fold, prelayer_shape,
prelayer_ok_dx, the two-stage pre-layer's 16-column segment, the deferred AvgL1Norm backward) or one
of its masks (Bv < B, widths that pad to 16, S or S + A one past a 16-column block) can still go
wrong.  ``golden(case)`` is the synthetic golden of a case (tests/test_engine_gpu.py _synthetic_golden's
layout, plus the net shape keys of conftest.shape_of); its environment is "Edge-v0", which exists in
oracle.spec.TASKS only inside ``edge_env(case)`` -- the table of real environments stays as it is.

``reference(case)`` runs the CPU oracle on the case twice, in float32 (what the goldens pin) and in
float64 (``float64_oracle()``: oracle.agents' two tensor constructors swapped, nothing else), once per
process, and is shared by tests/test_shape_edges.py and tests/test_shape_edges_gpu.py.
"""

from __future__ import annotations

import contextlib
from collections import namedtuple

import numpy as np
import torch

from oracle import agents, spec

ENV = "Edge-v0"

Case = namedtuple("Case", "alg S A H hidden_sizes zs_dim B use_lap n_steps seed extra bc_lambda note")


def _case(alg, S, A, H, B, seed, hidden_sizes=None, zs_dim=None, use_lap=None, bc_lambda=0.0, note=""):
    n_steps = {"td7": 7, "td3": 5, "sac": 4}[alg]
    # TD7: a hard update every 3 steps, so 7 steps hold policy steps (2, 4, 6) and two hard updates (3, 6)
    extra = {"target_update_rate": 3} if alg == "td7" else {}
    if use_lap is None:
        use_lap = alg != "sac"
    return Case(alg, S, A, H, hidden_sizes, zs_dim, B, use_lap, n_steps, seed, extra, bc_lambda, note)


# Seeds: 101 + the case's position, fixed before the engine ran any of them.  Three cases missed the host
# criteria of tests/test_shape_edges.py (float32 oracle against float64) at that seed and took the first of
# seed + 100 k that meets them: td7-h272 (204: one of 74k zs3 weights 1.9e-5 from float64 after 7 steps),
# td7-h512 (2805: at this width 5-20 of 3.2M elements land past 1e-5 for most seeds) and sac-min (217: with
# one row, log(1 - a^2 + 1e-6) of a saturated action is 2.5e-5 off in float32).  The three cases for the 64-row
# tiles (td7-w50, sac-w50, td3-w100: 122 - 124) met the host criteria at their first seed (worst step-1 moment
# distance 7.4e-7 / 8.1e-7 / 3.2e-7), and no (case, plan) pair of tests/plan_cases.py needed a reseed.
CASES = {
    "td7-b1": _case("td7", 11, 3, 32, 1, 101, note="one valid row, 15 masked"),
    "td7-min": _case("td7", 1, 1, 4, 17, 102, zs_dim=4, note="every dimension at its minimum; K = 1; 2 row blocks"),
    "td7-odd": _case("td7", 33, 17, 36, 31, 103, zs_dim=20, note="H % 16 != 0: no fold, standalone head; Z != H"),
    "td7-h272": _case("td7", 11, 3, 272, 16, 204, note="just past the H <= 256 fusions, fold still on"),
    "td7-h512": _case("td7", 11, 3, 512, 16, 2805, zs_dim=128, note="widest TD7; Z != H"),
    "td7-a32": _case("td7", 16, 32, 32, 16, 106, note="actor_pre at its limit"),
    "td7-a33": _case("td7", 16, 33, 32, 16, 107, note="one past actor_pre"),
    "td7-max_in": _case("td7", 1024, 128, 32, 16, 108, note="largest inputs: R = S + A = 1152, Z + A"),
    "td7-b1023": _case("td7", 11, 3, 32, 1023, 109, note="64 row blocks, the last with 15 valid rows"),
    "td7-odd_bc": _case("td7", 33, 17, 36, 31, 110, zs_dim=20, bc_lambda=0.1, note="offline term over Bv x A"),
    "td3-min": _case("td3", 1, 1, 4, 1, 111, use_lap=False, note="every dimension at its minimum"),
    "td3-k49": _case("td3", 49, 16, 20, 31, 112, note="one past the pre-layer's K <= 48, width % 16 != 0"),
    "td3-k48": _case("td3", 32, 16, 32, 16, 113, note="pre-layer at K = 48 for actor and critic"),
    "td3-a17": _case("td3", 11, 17, 32, 16, 114, note="one past the two-stage segment of 16"),
    "td3-a33": _case("td3", 11, 33, 32, 16, 115, note="one past actor_pre"),
    "td3-deep6": _case("td3", 11, 3, 32, 33, 116, hidden_sizes=[4, 36, 20, 64, 12, 32], note="six unequal hidden layers"),
    "sac-min": _case("sac", 1, 1, 4, 1, 217, note="every dimension at its minimum"),
    "sac-a24": _case("sac", 11, 24, 32, 17, 118, note="fused raw head + rsample at 2A = 48"),
    "sac-a25": _case("sac", 11, 25, 32, 17, 119, note="2A = 50: the standalone rsample"),
    "sac-h260": _case("sac", 16, 24, 260, 15, 120, hidden_sizes=[260, 260], note="R just past 256, % 16 != 0"),
    "sac-max_in": _case("sac", 1024, 128, 32, 16, 121, note="largest inputs"),
    # 64-row tiles (rle_plan wide, tests/plan_cases.py): a batch that pads to one 64-row block / to 112 rows
    "td7-w50": _case("td7", 11, 3, 64, 50, 122, note="pads to one 64-row block, 14 masked rows"),
    "sac-w50": _case("sac", 11, 3, 64, 50, 123, note="pads to one 64-row block, 14 masked rows"),
    "td3-w100": _case("td3", 11, 3, 64, 100, 124, note="pads to 112 rows: no whole 64-row blocks, wide_tiles declines"),
}

INFO_KEYS = {"td7": ("train/encoder", "train/q_fn", "train/policy"),
             "td3": ("train/q_fn", "train/policy", "norm/policy"),
             "sac": ("train/q_fn", "tmp", "norm/tmp", "train/policy", "train/tmp", "entropy")}
BC_KEYS = ("train/encoder", "train/q_fn", "train/policy", "train/bc", "train/q_abs")


def info_keys(case):
    c = CASES[case]
    return BC_KEYS if c.bc_lambda else INFO_KEYS[c.alg]


def capacity(case):
    """Replay capacity = fill: 256 rows (2048 for the batch of 1023)."""
    return 2048 if CASES[case].B > 256 else 256


@contextlib.contextmanager
def edge_env(case):
    """oracle.spec.TASKS["Edge-v0"] = the case's (S, A, action bound 1) while the block runs."""
    c = CASES[case]
    assert ENV not in spec.TASKS
    spec.TASKS[ENV] = (c.S, c.A, 1.0)
    try:
        yield
    finally:
        del spec.TASKS[ENV]


def golden(case):
    c = CASES[case]
    ncap = capacity(case)
    g = {"meta_alg": np.array(c.alg), "meta_env": np.array(ENV),
         "meta": np.array([c.H, c.B, ncap, ncap, c.n_steps, int(c.use_lap), c.seed]),
         "meta_extra_keys": np.array(list(c.extra), dtype="<U32"),
         "meta_extra_vals": np.array(list(c.extra.values()), np.float64)}
    if c.hidden_sizes is not None:
        g["meta_hidden"] = np.array(c.hidden_sizes)
    if c.zs_dim is not None:
        g["meta_zs"] = np.array(c.zs_dim)
    for k, v in spec.tapes(c.alg, c.B, c.A, c.n_steps, c.seed + 3).items():
        g["tape_" + k] = v
    return g


@contextlib.contextmanager
def float64_oracle():
    """The oracle in float64: oracle.agents._params / _tt (its parameter and batch tensors, hard-coded
    float32) swapped for float64 versions, and torch's default dtype for the tensors the agents create
    themselves (SAC's log_alpha).  Everything is put back on exit: the float32 path is untouched."""
    import offline_oracle

    def params64(d):
        return {k: torch.tensor(np.asarray(v), dtype=torch.float64).requires_grad_(True) for k, v in d.items()}

    def tt64(x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))

    saved = agents._params, agents._tt, offline_oracle._tt, torch.get_default_dtype()
    agents._params, agents._tt, offline_oracle._tt = params64, tt64, tt64
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        agents._params, agents._tt, offline_oracle._tt = saved[:3]
        torch.set_default_dtype(saved[3])


def _run(case):
    """One oracle run of a case (in whatever precision is in effect): per-step info table, indices,
    priorities and TD7 value bounds, the Adam first moments after step 1, the end parameters."""
    from offline_oracle import build_offline
    from test_oracle import build_from_golden

    c = CASES[case]
    g = golden(case)
    with edge_env(case):
        if c.bc_lambda:
            orc, rep, tp, n, B = build_offline(g, c.bc_lambda)
        else:
            _, orc, rep, tp, n, B = build_from_golden(g)
    out = {"info": [], "ind": [], "prio": [], "vb": [], "m": None}
    for t in range(n):
        i1, n1 = agents.run_steps(orc, c.alg, rep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
        out["info"] += i1
        out["ind"] += n1
        out["prio"].append(rep.priority.copy() if c.use_lap else None)
        if c.alg == "td7":
            out["vb"].append(np.array([orc.value_max, orc.value_min, orc.vt_max, orc.vt_min], np.float64))
        if t == 0:
            out["m"] = {k[:-2]: v for k, v in agents.moments(orc).items() if k.endswith(":m")}
    keys = info_keys(case)
    out["table"] = np.array([[np.nan if i[k] is None else i[k] for k in keys] for i in out["info"]], np.float64)
    out["params"] = {(net, k): v.detach().numpy().copy() for net, d in orc.nets().items() for k, v in d.items()}
    if c.alg == "sac":
        out["log_alpha"] = orc.log_alpha.detach().numpy().copy()
    return out


_REF = {}


def reference(case):
    """{"f32": run, "f64": run, "g": golden} of a case, computed once and shared (read-only)."""
    if case not in _REF:
        torch.set_num_threads(1)
        f32 = _run(case)
        with float64_oracle():
            f64 = _run(case)
        _REF[case] = {"f32": f32, "f64": f64, "g": golden(case)}
    return _REF[case]


def moment_distance(a, b):
    """max |a - b| over a tensor as a fraction of b's max magnitude (b: the float64 moments)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
