"""The plan table (tests/plan_cases.py) on the GPU: every (edge case, plan) pair builds clean under the address
audit and the hazard check, takes the path the plan asks for, and

  T / F pairs (tile widths, register-blocked and 64-row tiles, fusions switched off, the opt-in sampler) train like
     the CPU oracle at the shape-edge sweep's own criteria (test_shape_edges_gpu.check_trains_like_the_oracle:
     indices exact; step-1 Adam first moments within max(1e-5, 4 d32) of the float64 oracle; info at LOSS_RTOL;
     priorities, untouched rows, value bounds; parameters at 2 lr n + 1e-4 and bulk 0.99; SAC log_alpha);
  S pairs (one scheduling / launch field changed over tiles pinned at 64) are bit-identical to the ``tn64`` run of
     the same case: parameters and both Adam moments, indices, priorities, counters, value bounds, info rows;
  rle_step(20) under steps_per_graph 0 / 2 / 4 / 5 / 10 / 16 / default is bit-identical to 20 x rle_step(1).

The oracle runs of a case are computed once (edge_cases.reference) and requested in a fixture, so whichever test
touches a case first pays for them in its setup, not in its call.
"""

import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
import plan_cases as PC  # noqa: E402
from edge_cases import CASES, capacity, golden, reference  # noqa: E402
from test_normbwd_rows_gpu import _bits  # noqa: E402
from test_shape_edges_gpu import _engine, check_trains_like_the_oracle  # noqa: E402

ALL = list(PC.PAIRS)


@pytest.fixture
def oracle_runs(request):
    return reference(request.node.callspec.params["pair"][0])


@pytest.mark.parametrize("pair", PC.pairs("T", "F"), ids=PC.pair_id)
def test_pair_trains_like_the_oracle(pair, oracle_runs):
    case, plan, group = pair
    w = check_trains_like_the_oracle(case, PC.make(E, plan))
    print(f"PLAN {group} {case} {plan}: gradient {w['gradient']:.2e} bulk {w['bulk']:.4f} far {w['far']:.2e}")


# ---- builds: audit, hazards, paths ------------------------------------------------------------------------------

_BUILT = {}


def _built(case, plan, monkeypatch):
    """{"plan": the resolved plan, "d": {which: description with workgroup counts}} of (case, plan), every step
    program built under RLE_AUDIT + RLE_HAZARD, no step run; {"error": message} when the build fails.  Once per
    pair (and per default / reference arm)."""
    key = (case, plan)
    if key not in _BUILT:
        for k in ("RLE_AUDIT", "RLE_HAZARD", "RLE_DESC_WG"):
            monkeypatch.setenv(k, "1")
        try:
            eng, rep = _engine(case, PC.make(E, plan), golden(case))
            _BUILT[key] = {"plan": eng.plan(), "d": {w: eng.describe(w) for w in (0, 1, 2, 3)}}
            eng.close()
            rep.close()
        except RuntimeError as e:
            _BUILT[key] = {"error": str(e)}
    return _BUILT[key]


@pytest.mark.parametrize("pair", ALL, ids=PC.pair_id)
def test_pair_programs_pass_audit_and_hazard_checks(pair, monkeypatch):
    """RLE_AUDIT + RLE_HAZARD while every step program of the pair is built: each GEMM's address replay (partial
    32- / 64-wide tiles, 64-row tiles over masked rows) stays inside live allocations, and no level of the
    rescheduled programs holds two ops touching one byte."""
    case, plan, _ = pair
    b = _built(case, plan, monkeypatch)
    assert "error" not in b, b
    assert b["d"][0] and b["d"][1]


_GEMM = re.compile(r"gemm\[(\d+)x(\d+)x(\d+) ([^\]]+)\]/(\d+)")


def _gemms(b, which=(0, 1)):
    """(M, N, R, epilogue tag, workgroups) of every GEMM of the policy and plain step programs (the hard update's
    fold GEMMs are built outside the tile planner)."""
    return [(int(m[0]), int(m[1]), int(m[2]), m[3], int(m[4])) for w in which for m in _GEMM.findall(b["d"][w])]


def _widths(M, N, tag, wg):
    """The tile widths a GEMM's workgroup count is consistent with: forward / DX (M / 16) ceil(N / tn), weight
    gradient ceil(M / 16) (ceil(N / tn) + 1) (one more tile column: the bias)."""
    if tag.startswith("adam"):
        return {t for t in (16, 32, 64) if -(-M // 16) * (-(-N // t) + 1) == wg}
    return {t for t in (16, 32, 64) if (M // 16) * -(-N // t) == wg}


def _count(b, pattern, which=(0, 1)):
    return sum(len(re.findall(pattern, b["d"][w])) for w in which)


def _bare(name):  # a standalone op (not a GEMM epilogue tag), with its workgroup count behind it
    return r"(?m)[: ]\*?%s/\d+( |$)" % name


def _levels(b, which=0):
    return len(b["d"][which].splitlines())


def _check_tiles(case, plan, b):
    kw, alg = PC.PLANS[plan], CASES[case].alg
    for k, v in kw.items():
        assert b["plan"][k] == v, (k, b["plan"])
    gemms = _gemms(b)
    wide = [g for g in gemms if g[3].endswith(".w")]
    if "wide" in kw:
        assert b["plan"]["rb"] == 1  # (the register-blocked weight gradients come with the 64-row tiles)
        if case == "td3-w100":  # 112 rows: wide_tiles declines, the 16-row tiles run
            assert not wide, wide
        else:
            assert wide, b["d"][0]
            for M, N, R, tag, wg in wide:
                assert M % 64 == 0 and N % kw["wide"] == 0 and wg == (M // 64) * (N // kw["wide"]), (M, N, tag, wg)
        return
    assert not wide
    if "tn_min" in kw or "level_cap" in kw:
        tn = kw.get("tn_min", 64)  # (level_cap=1: the planner's own pass widens every tile to 64)
        seen = 0
        for M, N, R, tag, wg in gemms:
            ok = {t for t in (16, 32, 64) if t >= tn}  # (a minimum: the planner may still widen an over-full level)
            if tn == 64 and alg != "td7" and tag in ("st", "st+sacpre"):
                ok.add(32)  # (TD3 / SAC: a pre-layer source is at most 32 wide, FwdOpt::pl_src)
            ws = _widths(M, N, tag, wg)
            assert ws & ok, (M, N, tag, wg, sorted(ws), sorted(ok))
            seen += ws <= ok and N > 16
        # (td7-min: every width is at most 16, one tile column whatever the plan: only plan() shows it)
        assert seen or max(g[1] for g in gemms) <= 16 or tn == 16, b["d"][0]
    if "pl_tn" in kw:
        pl = [g for g in gemms if "+pl" in g[3]]
        assert pl
        for M, N, R, tag, wg in pl:
            assert kw["pl_tn"] in _widths(M, N, tag, wg), (M, N, tag, wg)
    if "pre_tn" in kw and CASES[case].alg == "sac":
        pre = [g for g in gemms if g[3] == "st+sacpre"]
        assert pre
        for M, N, R, tag, wg in pre:
            assert kw["pre_tn"] in _widths(M, N, tag, wg), (M, N, tag, wg)
    if "pre_tn" in kw and CASES[case].alg == "td3":
        # TD3's pre-GEMM consumers carry the plain "st" tag: at pre_tn 16 no forward GEMM is left wider than 16
        # (td3-k48 at 32: H = 32 is one tile column at 32 and at 64, so only plan() tells them apart)
        wider = [g for g in gemms if g[3] == "st" and g[1] > 16 and 16 not in _widths(g[0], g[1], g[3], g[4])]
        assert bool(wider) == (kw["pre_tn"] > 16), wider


# F pairs: what the description loses and gains with a bit off.  (default arm, plan arm) -> None, by bit; the
# vocabulary is test_shape_edges_gpu.PATHS'.  actor_pre and the folded zsa3 have no tag: without `pre` the actor's
# output layer is an op of its own (more levels), without `fold` the hard update loses its foldbias ops.
def _f_pre(alg, d, p):
    assert _levels(p) > _levels(d) and _levels(p, 1) > _levels(d, 1)
    if alg == "td3":  # (the two-stage prologue sits behind the pre-GEMM target action)
        assert _count(d, r"qdot\+pl2\]") and not _count(p, r"qdot\+pl2\]")


def _f_qdot(alg, d, p):
    assert _count(d, r" qdot\]") and not _count(p, r"qdot")
    assert _count(d, r"head\+dx") and not _count(p, r"head\+dx") and _count(p, _bare("head"))  # (head+dx reads partials)


def _f_headdx(alg, d, p):
    assert _count(d, r"head\+dx") and not _count(d, _bare("head"))
    assert not _count(p, r"head\+dx") and _count(p, _bare("head"))


def _f_nbdefer(alg, d, p):
    assert _count(d, r"nbdot\]") and _count(d, r"adam\+nbr?\]")
    assert not _count(p, r"nbdot\]") and not _count(p, r"adam\+nb") and _count(p, _bare("normbwd")) > _count(d, _bare("normbwd"))


def _f_fold(alg, d, p):
    assert _count(d, _bare("foldbias"), (2,)) and not _count(p, _bare("foldbias"), (2,))
    assert _levels(p) > _levels(d)


def _f_endsplit(alg, d, p):
    assert _count(d, _bare("end"), (0,)) == 2 and _count(p, _bare("end"), (0,)) == 1
    assert _count(d, _bare("end"), (1,)) == 2 and _count(p, _bare("end"), (1,)) == 1


def _f_normfin(alg, d, p):  # (the finalizing ops are normbwd-kind ops; without them the row-major partials go too)
    assert _count(p, _bare("normbwd")) < _count(d, _bare("normbwd"))
    assert _count(d, r"adam\+nbr\]") and not _count(p, r"adam\+nbr\]") and _count(p, r"adam\+nb\]")


def _f_nbrows(alg, d, p):
    assert _count(d, r"adam\+nbr\]") and not _count(d, r"adam\+nb\]")
    assert not _count(p, r"adam\+nbr\]") and _count(p, r"adam\+nb\]") == _count(d, r"adam\+nbr\]")
    assert _count(p, _bare("normbwd")) == _count(d, _bare("normbwd"))


def _f_prelayer(alg, d, p):
    assert _count(d, r"\+pl") and not _count(p, r"\+pl") and _levels(p) > _levels(d)


def _f_twostage(alg, d, p):
    assert _count(d, r"qdot\+pl2\]") and not _count(p, r"qdot\+pl2\]") and _count(p, r"qdot\+pl\]") == _count(d, r"qdot\+pl\]")


def _f_pipolyak(alg, d, p):
    assert _count(p, _bare("polyak"), (0,)) == _count(d, _bare("polyak"), (0,)) + 1


def _f_sacfwd(alg, d, p):
    assert _count(d, r"sacfwd\]") and not _count(d, _bare("sacfwd"))
    assert not _count(p, r"sacfwd\]") and _count(p, _bare("sacfwd")) and not _count(p, r"st\+sacpre")


def _f_sacbwd(alg, d, p):
    assert _count(d, r"sacbwd\]") and not _count(d, _bare("sacbwd"))
    assert not _count(p, r"sacbwd\]") and _count(p, _bare("sacbwd"))


def _f_sacpre(alg, d, p):
    assert _count(d, r"st\+sacpre") and not _count(p, r"st\+sacpre") and _count(p, r"sacfwd\]") == _count(d, r"sacfwd\]")


def _f_priosample(alg, d, p):
    """Fused: the sampler runs first (it applies the pending update to what it reads), the OP_PRIORITY that persists
    the update after it; by default the priority op precedes the sampler."""
    def order(b):
        lines = b["d"][1].splitlines()
        prio = [i for i, x in enumerate(lines) if re.search(_bare("prio"), x)]
        samp = [i for i, x in enumerate(lines) if re.search(_bare("sgather"), x)]
        assert len(prio) == 1 and len(samp) == 1, b["d"][1]
        return prio[0], samp[0]

    pd, sd = order(d)
    pp, sp = order(p)
    assert pd < sd and sp < pp, (pd, sd, pp, sp)


F_CHECKS = {"pre": _f_pre, "qdot": _f_qdot, "headdx": _f_headdx, "nbdefer": _f_nbdefer, "fold": _f_fold,
            "endsplit": _f_endsplit, "normfin": _f_normfin, "nbrows": _f_nbrows, "prelayer": _f_prelayer,
            "twostage": _f_twostage, "pipolyak": _f_pipolyak, "sacfwd": _f_sacfwd, "sacbwd": _f_sacbwd,
            "sacpre": _f_sacpre}
FUSED_TAGS = r"head\+dx|\+pl|nbdot|adam\+nb|sacfwd\]|sacbwd\]|st\+sacpre"


def _check_fusions(case, plan, d, p):
    alg = CASES[case].alg
    kw = PC.PLANS[plan]
    assert sorted(p["plan"]["fuse_off"]) == sorted(kw.get("fuse_off", ())), p["plan"]
    assert sorted(p["plan"]["fuse_on"]) == sorted(kw.get("fuse_on", ())), p["plan"]
    if plan == "priosample":
        return _f_priosample(alg, d, p)
    if plan.startswith("off-"):
        return F_CHECKS[plan[4:]](alg, d, p)
    # every bit off: no fused tag is left in any program, each step ends in one op, the standalone ops run
    assert plan in ("alloff", "alloff-tn64")
    assert not _count(p, FUSED_TAGS, (0, 1, 2, 3)) and not _count(p, _bare("foldbias"), (2,)), p["d"]
    # (the offline term's Q(s, pi(s)) always comes from q-dot partials: two qdot GEMMs stay in td7-odd_bc's policy step)
    assert _count(p, r"qdot", (0,)) == (2 if CASES[case].bc_lambda else 0) and not _count(p, r"qdot", (1, 2)), p["d"][0]
    assert _count(p, _bare("end"), (0,)) == 1 == _count(p, _bare("end"), (1,))
    assert _count(p, _bare("head"))
    if alg == "td7":
        assert _count(p, _bare("normbwd"))
        if case == "td7-b1023":  # every norm backward standalone, over all 1,024 rows (4 rows per workgroup)
            assert set(re.findall(r"normbwd/(\d+)", p["d"][0])) == {"256"}, p["d"][0]
    if alg == "td3":
        assert _count(p, _bare("polyak"), (0,)) == _count(d, _bare("polyak"), (0,)) + 1
    if alg == "sac":
        assert _count(p, _bare("sacfwd")) and _count(p, _bare("sacbwd"))
    if "tn_min" in kw:
        assert p["plan"]["tn_min"] == kw["tn_min"]
        assert all(kw["tn_min"] in _widths(M, N, tag, wg) for M, N, R, tag, wg in _gemms(p))


# S pairs: where the field moves an op at these shapes, the description differs from the reference arm's.  Honestly
# identical programs (nothing asserted of the descriptions): `balance` at the algorithm's own default (TD7 3, TD3 1,
# SAC 2) and SAC at 1 (its levels hold no item mode 1 would move that mode 2 does not); `level_cap` 1 and `flat_div`
# 1 / 1000 without sched_cap (they steer the planner's widening pass only, and with the tiles pinned at 64 nothing
# is left to widen); `dispatch`, `dpf`, `xcd` (launch path, descriptor prefetch and tile order: not part of the
# description, the same ops in the same levels).
BALANCE_DEFAULT = {"td7": 3, "td3": 1, "sac": 2}


def _s_moves(alg, plan):
    kw = PC.PLANS[plan]
    if "balance" in kw:
        return kw["balance"] != BALANCE_DEFAULT[alg] and not (alg == "sac" and kw["balance"] == 1)
    return bool(set(kw) & {"lpt", "sched_cap", *PC.WEIGHTS})


def _check_schedule(case, plan, ref, p):
    kw = PC.PLANS[plan]
    for k, v in kw.items():
        assert p["plan"][k] == v, (k, p["plan"])
    # the same GEMMs with the same tiles in both arms, whatever their levels
    assert sorted(_gemms(p)) == sorted(_gemms(ref))
    if _s_moves(CASES[case].alg, plan):
        assert p["d"][0] != ref["d"][0] or p["d"][1] != ref["d"][1], (plan, p["d"][0])


@pytest.mark.parametrize("pair", ALL, ids=PC.pair_id)
def test_pair_takes_the_intended_path(pair, monkeypatch):
    """A sanitised plan must not silently be the default: rle_get_plan reports the fields asked for, and the
    program descriptions (with each op's workgroup count, RLE_DESC_WG) show the tiles, the standalone ops or the
    moved ops."""
    case, plan, group = pair
    b = _built(case, plan, monkeypatch)
    assert "error" not in b, b
    if group == "T":
        _check_tiles(case, plan, b)
    elif group == "F":
        _check_fusions(case, plan, _built(case, None, monkeypatch), b)
    else:
        _check_schedule(case, plan, _built(case, PC.S_REFERENCE, monkeypatch), b)


# ---- bitwise: schedule-only fields, multi-step programs ---------------------------------------------------------

def _snapshot(case, eng, rep, infos):
    c = CASES[case]
    out = {"info": np.asarray(infos, np.float32), "ind": eng.last_indices(), "counters": eng.counters(),
           "state": eng.state_export(E.STATE_ALL).copy()}
    if c.use_lap:
        out["prio"] = rep.get_priority(capacity(case)).copy()
    if c.alg == "td7":
        out["vb"] = eng.value_bounds().copy()
    return out


def _assert_bitwise(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        nbad = int((_bits(a[k]) != _bits(b[k])).sum())
        assert nbad == 0, (what, k, nbad, a[k].size)


_TAPED = {}


def _taped_run(case, plan):
    """The edge sweep's trajectory (step 1 alone, the rest as one burst, on the case's tapes) under a named plan;
    no oracle."""
    key = (case, plan)
    if key in _TAPED:
        return _TAPED[key]
    g = golden(case)
    n = CASES[case].n_steps
    eng, rep = _engine(case, PC.make(E, plan), g)
    eng.set_tapes(u=g["tape_u"], eps=g["tape_eps"], eps_pi=g.get("tape_eps_pi"))
    infos = [eng.step(1)[0].copy()]
    first = _snapshot(case, eng, rep, infos)
    infos += [r.copy() for r in eng.step(n - 1)]
    eng.set_tapes()
    out = _snapshot(case, eng, rep, infos)
    out.update({k + "_1": v for k, v in first.items()})
    eng.close()
    rep.close()
    if plan == PC.S_REFERENCE:
        _TAPED[key] = out
    return out


@pytest.mark.parametrize("pair", PC.pairs("S"), ids=PC.pair_id)
def test_schedule_fields_change_no_float(pair):
    """The same ops on the same tiles, only in other levels, launches or tile orders: parameters, Adam moments,
    indices, priorities, counters, value bounds and info rows after step 1 and after the last step are the bits of
    the ``tn64`` run.  (The loss partials are indexed by output tile, so no level change reorders their sum.)"""
    case, plan, _ = pair
    _assert_bitwise(_taped_run(case, PC.S_REFERENCE), _taped_run(case, plan), pair)


_SINGLE = {}


def _twenty(case, base, k, single):
    c = CASES[case]
    g = dict(golden(case))
    extra = PC.MULTI_EXTRA.get(c.alg)
    if extra:  # (as test_multistep_graphs_equal_single_steps' @tur250)
        g["meta_extra_keys"] = np.array(list(extra), dtype="<U32")
        g["meta_extra_vals"] = np.array(list(extra.values()), np.float64)
    more = {} if single or k == -1 else {"steps_per_graph": k}
    eng, rep = _engine(case, PC.make(E, base, **more), g)
    l0 = eng.launch_count()
    infos = [eng.step(1)[0].copy() for _ in range(20)] if single else eng.step(20)
    out = _snapshot(case, eng, rep, infos)
    spg, launches = eng.plan()["steps_per_graph"], eng.launch_count() - l0
    eng.close()
    rep.close()
    return out, spg, launches


@pytest.mark.parametrize("case,base,k", PC.MULTI, ids=[f"{c}-{b or 'default'}-spg{k}" for c, b, k in PC.MULTI])
def test_multistep_program_equals_single_steps(case, base, k):
    """rle_step(20) (the K-step program, its remainder programs and single steps around them) against 20 x
    rle_step(1) from the same start: bit-identical.  TD7 runs with target_update_rate 250, so no hard update breaks
    the 20 steps up and its K-step programs replay at the edge shape."""
    alg = CASES[case].alg
    if (case, base) not in _SINGLE:
        _SINGLE[case, base] = _twenty(case, base, -1, True)
    one, _, launches_one = _SINGLE[case, base]
    got, spg, launches = _twenty(case, base, k, False)
    assert spg == ({"td7": 6, "td3": 16, "sac": 8}[alg] if k == -1 else k)
    # the path: a multi-step program saves launches (SAC's runs as many levels per step as its single-step one)
    if k in (0, 1):
        assert launches == launches_one, (launches, launches_one)
    elif alg == "sac":
        assert 0 < launches <= launches_one, (launches, launches_one)
    else:
        assert 0 < launches < launches_one, (launches, launches_one)
    _assert_bitwise(one, got, (case, base, k))
