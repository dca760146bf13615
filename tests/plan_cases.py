"""Plans crossed with the shape-edge table (TEST INFRASTRUCTURE, no GPU call).

``PLANS``: a name -> ``E.make_plan`` keyword arguments.  ``PAIRS``: ``(case, plan, group)`` triples, ``case`` a key
of ``edge_cases.CASES``.  Three groups:

T (tile plan): the GEMM tile widths change (``tn_min``, ``pre_tn``, ``pl_tn``, the planner's own widening under
   ``level_cap=1``, the register-blocked weight-gradient tiles ``rb``, the 64-row tiles ``wide``), so the fp32
   summation order changes: checked against the oracle at the edge sweep's criteria.
F (fusion switches): one ``fuse_off`` bit at a time on a case where that fusion is on by default, every bit off,
   every bit off under 64-wide tiles, and the opt-in ``priosample``: the standalone ops run, checked against the
   oracle.
S (schedule only): the tiles are pinned with ``tn_min=64`` in both arms (nothing is left to widen, so ``level_cap``
   is free) and one scheduling / launch field changes: the same ops in other levels, so every float must be
   bit-identical to the ``tn64`` run of the same case.

``MULTI``: ``(case, base plan, steps_per_graph)`` triples for rle_step(20) against 20 x rle_step(1); TD7 cases run
with ``target_update_rate`` 250 there (the table's 3 puts a hard update into every window, so its bursts never
replay a multi-step TD7 program).

Which algorithm's step builder reads which ``fuse_off`` / ``fuse_on`` bit is restated in ``READS``
(tests/test_plan_edges.py holds the table to it).
"""

from __future__ import annotations

# engine.cpp: td7_fold / actor_pre / td7_qdot / td7_headdx / td7_nb_defer / norm_fin / nb rows / end_split /
# prio_sample_fused; mlp_critic_fwd, mlp_actor_fwd, mlp_policy, mlp_actor_backward, pi_polyak_fused
READS = {
    "td7": ("pre", "qdot", "headdx", "nbdefer", "fold", "endsplit", "normfin", "nbrows", "priosample"),
    "td3": ("prelayer", "pre", "twostage", "pipolyak", "headdx", "endsplit", "priosample"),
    "sac": ("prelayer", "sacfwd", "sacbwd", "sacpre", "headdx", "endsplit"),
}
OPT_IN = ("priosample",)
ALL_OFF = ("prelayer", "pre", "qdot", "headdx", "nbdefer", "sacfwd", "sacbwd", "fold", "pipolyak", "endsplit",
           "twostage", "sacpre", "normfin", "nbrows")

# the rebalance weights of rle_plan (include/rle.h): seven fields
WEIGHTS = ("tiny_w", "uni_w", "tiny_wg", "pl_w", "lap_w", "head_w", "adam_w")

PLANS = {
    # ---- T
    "tn16": dict(tn_min=16), "tn32": dict(tn_min=32), "tn64": dict(tn_min=64),
    "tn32rb": dict(tn_min=32, rb=1), "tn64rb": dict(tn_min=64, rb=1),
    "cap1": dict(level_cap=1),
    "pre16": dict(pre_tn=16), "pre32": dict(pre_tn=32), "pre64": dict(pre_tn=64),
    "pl16": dict(pl_tn=16), "pl32": dict(pl_tn=32), "pl64": dict(pl_tn=64),
    "wide64": dict(wide=64), "wide32": dict(wide=32),
    # ---- F
    **{"off-" + b: dict(fuse_off=[b]) for b in ALL_OFF},
    "alloff": dict(fuse_off=list(ALL_OFF)),
    "alloff-tn64": dict(fuse_off=list(ALL_OFF), tn_min=64),
    "priosample": dict(fuse_on=["priosample"]),
    # ---- S (every one over tn_min=64, the reference arm's plan)
    **{f"s-balance{v}": dict(tn_min=64, balance=v) for v in (0, 1, 2, 3)},
    "s-lpt0": dict(tn_min=64, lpt=0),
    "s-schedcap8": dict(tn_min=64, sched_cap=1, level_cap=8),
    "s-cap1": dict(tn_min=64, level_cap=1),
    "s-flat1": dict(tn_min=64, flat_div=1), "s-flat1000": dict(tn_min=64, flat_div=1000),
    "s-w0": dict(tn_min=64, **{w: 0 for w in WEIGHTS}),
    "s-w1000": dict(tn_min=64, **{w: 1000 for w in WEIGHTS}),
    "s-dispatch0": dict(tn_min=64, dispatch=0), "s-dispatch2": dict(tn_min=64, dispatch=2),
    "s-dpf0": dict(tn_min=64, dpf=0), "s-xcd0": dict(tn_min=64, xcd=0),
}
S_REFERENCE = "tn64"

NEW_CASES = ("td7-w50", "sac-w50", "td3-w100")


def _cross(cases, plans, group):
    return [(c, p, group) for c in cases for p in plans]


PAIRS = (
    # ---- T
    _cross(("td7-odd", "td7-h272", "td7-min", "td7-b1", "td7-odd_bc", "td3-k49", "td3-deep6", "sac-h260", "sac-a25"),
           ("tn32", "tn64", "tn64rb"), "T")
    + _cross(("td7-b1023",), ("tn32rb", "tn64rb", "wide32"), "T")
    + [("td7-h512", "cap1", "T")]
    + _cross(("td3-k48", "td3-a17"), ("pl16", "pl32", "pre16"), "T")
    + _cross(("sac-a24",), ("pre16", "pre64", "pl16"), "T")
    + _cross(NEW_CASES, ("wide64", "wide32", "tn64rb"), "T")
    # (the remaining width of each field, so 16 / 32 / 64 of tn_min, pre_tn and pl_tn are all requested by name)
    + [("td7-w50", "tn16", "T"), ("td3-k48", "pre32", "T"), ("sac-a24", "pl64", "T")]
    # ---- F: one bit off (TD7 reads no prelayer bit), all off, all off under 64-wide tiles, the opt-in sampler
    + _cross(("td7-a32", "td7-b1"), ["off-" + b for b in READS["td7"] if b not in OPT_IN], "F")
    + _cross(("td3-k48",), ["off-" + b for b in READS["td3"] if b not in OPT_IN], "F")
    + _cross(("sac-a24",), ["off-" + b for b in READS["sac"]], "F")
    + _cross(("td7-odd", "td7-odd_bc", "td7-b1023", "td3-a17", "td3-deep6", "sac-a25", "sac-h260"), ("alloff",), "F")
    + _cross(("td7-odd", "sac-h260"), ("alloff-tn64",), "F")
    + _cross(("td7-odd", "td7-b1", "td3-k49"), ("priosample",), "F")
    # ---- S
    + _cross(("td7-odd", "td3-k49", "sac-a25", "td7-w50"), [p for p in PLANS if p.startswith("s-")], "S")
)

SPG = (0, 2, 4, 5, 10, 16, -1)  # (-1: the algorithm's default)
MULTI = ([(c, base, k) for c in ("td7-odd", "td3-k49", "sac-a25") for base in (None, "tn64") for k in SPG]
         + [("td7-b1023", base, k) for base in (None, "tn64") for k in (-1, 4)])
MULTI_EXTRA = {"td7": {"target_update_rate": 250}}


def pair_id(pair):
    return f"{pair[0]}-{pair[1]}"


def pairs(*groups):
    return [p for p in PAIRS if p[2] in groups]


def make(E, name, **more):
    """The rle_plan of a named plan (None: the default plan), with further fields changed."""
    kw = dict(PLANS[name]) if name else {}
    kw.update(more)
    return E.make_plan(**kw) if kw else None
