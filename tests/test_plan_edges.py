"""The plan table (tests/plan_cases.py) on the host: every plan is a plan, every pair names a case, and the table
covers the fields, widths and batches it was written for.  No GPU."""

import pytest

from edge_cases import CASES
import plan_cases as PC


def _E():
    return pytest.importorskip("rl._engine")


def _r16(b):
    return -(-b // 16) * 16


def test_every_plan_is_made_of_plan_fields_and_fuse_names():
    E = _E()
    fields = {k for k, _ in E.Plan._fields_}
    for name, kw in PC.PLANS.items():
        for k, v in kw.items():
            if k in ("fuse_off", "fuse_on"):
                assert v and set(v) <= set(E.FUSE), (name, k, v)
            else:
                assert k in fields and isinstance(v, int), (name, k)
        if "fuse_on" in kw:
            assert set(kw["fuse_on"]) <= set(PC.OPT_IN), name
        assert not set(kw.get("fuse_off", ())) & set(PC.OPT_IN), name
    assert set(PC.ALL_OFF) == set(E.FUSE) - set(PC.OPT_IN)
    assert set(PC.WEIGHTS) == {k for k in fields if k.endswith("_w") or k == "tiny_wg"}
    for alg, bits in PC.READS.items():
        assert set(bits) <= set(E.FUSE), alg
    assert set().union(*PC.READS.values()) == set(E.FUSE)  # (no bit that nobody reads)


def test_every_pair_names_a_case_and_a_plan_once():
    assert len(set(PC.PAIRS)) == len(PC.PAIRS)
    assert len({(c, p) for c, p, _ in PC.PAIRS}) == len(PC.PAIRS)
    for case, plan, group in PC.PAIRS:
        assert case in CASES and plan in PC.PLANS and group in "TFS", (case, plan, group)
    for case, base, k in PC.MULTI:
        assert case in CASES and (base is None or base in PC.PLANS) and k in PC.SPG, (case, base, k)
    assert len(set(PC.MULTI)) == len(PC.MULTI)
    used = {p for _, p, _ in PC.PAIRS} | {b for _, b, _ in PC.MULTI if b} | {PC.S_REFERENCE}
    assert used == set(PC.PLANS), set(PC.PLANS) - used
    assert set(PC.NEW_CASES) <= set(CASES)


def test_every_fuse_bit_is_switched_alone_for_each_algorithm_that_reads_it():
    """engine.cpp's readers restated (plan_cases.READS): TD7's builder reads pre / qdot / headdx / nbdefer / fold /
    endsplit / normfin / nbrows (and the opt-in priosample), TD3's prelayer / pre / twostage / pipolyak / headdx /
    endsplit (priosample), SAC's prelayer / sacfwd / sacbwd / sacpre / headdx / endsplit (no LAP: no priosample)."""
    alone = {}
    for case, plan, group in PC.pairs("F"):
        kw = PC.PLANS[plan]
        bits = list(kw.get("fuse_off", ())) + list(kw.get("fuse_on", ()))
        if len(bits) == 1 and set(kw) <= {"fuse_off", "fuse_on"}:
            alone.setdefault(CASES[case].alg, set()).add(bits[0])
    for alg, bits in PC.READS.items():
        assert alone.get(alg, set()) == set(bits), (alg, set(bits) ^ alone.get(alg, set()))
    # the opt-in sampler needs a LAP replay; B = 31 draws duplicate indices from 256 rows (last writer wins)
    for case, plan, _ in PC.pairs("F"):
        if plan == "priosample":
            assert CASES[case].use_lap, case
    assert ("td3-k49", "priosample", "F") in PC.PAIRS and CASES["td3-k49"].B == 31


def test_single_bit_pairs_sit_on_cases_where_the_fusion_is_on_by_default():
    """engine.cpp's predicates restated on the cases of the one-bit-off pairs."""
    c = CASES
    for name in ("td7-a32", "td7-b1"):
        x = c[name]
        assert x.A <= 32                                                      # actor_pre
        assert x.H % 16 == 0 and x.H <= 256 and x.zs_dim is None              # td7_fold, td7_headdx (B pads to 16)
        assert _r16(x.B) <= 256                                               # row-major dot partials (nbrows)
    x = c["td3-k48"]
    assert x.S + x.A <= 48 and x.A <= 16 and x.H % 16 == 0 and x.H <= 256 and x.hidden_sizes is None
    x = c["sac-a24"]
    assert 2 * x.A <= 48 and x.S <= 48 and x.H % 16 == 0 and x.H <= 256 and x.hidden_sizes is None


def test_every_tile_width_and_both_wide_values_appear():
    E = _E()
    seen = {"tn_min": set(), "pre_tn": set(), "pl_tn": set(), "wide": set(), "rb": set()}
    for _, plan, group in PC.pairs("T"):
        for k in seen:
            if k in PC.PLANS[plan]:
                seen[k].add(PC.PLANS[plan][k])
    assert seen["tn_min"] == {16, 32, 64} == seen["pre_tn"] == seen["pl_tn"], seen
    assert seen["wide"] == {32, 64} and seen["rb"] == {1}, seen
    # resolve_plan keeps these values as they are (a sanitised plan must not silently be another one)
    for name in ("tn32", "tn64", "pre16", "pre64", "pl16", "pl32", "wide32", "wide64", "tn64rb"):
        p = E.make_plan(**PC.PLANS[name])
        for k, v in PC.PLANS[name].items():
            assert getattr(p, k) == v, (name, k)


def test_table_restates_the_wide_and_rb_edges():
    c = CASES
    # wide_tiles: whole 64-row blocks of the batch padded to 16 rows, N a multiple of the tile width
    for name in ("td7-w50", "sac-w50"):
        assert _r16(c[name].B) == 64 and c[name].B < 64 and c[name].H % 64 == 0
    assert _r16(c["td3-w100"].B) % 64 != 0 and c["td3-w100"].H % 64 == 0
    assert _r16(c["td7-b1023"].B) == 1024 and c["td7-b1023"].B % 16 == 15  # (64 row blocks, the last one masked)
    wide = {case for case, plan, _ in PC.pairs("T") if "wide" in PC.PLANS[plan]}
    assert wide == {"td7-w50", "sac-w50", "td3-w100", "td7-b1023"}
    # rb: the four waves split the batch's 16-row blocks; B <= 16 leaves three of them without one, 17..32 two
    for plan in ("tn32rb", "tn64rb"):
        batches = [c[case].B for case, p, _ in PC.pairs("T") if p == plan]
        assert batches, plan
    batches = [c[case].B for case, p, _ in PC.pairs("T") if PC.PLANS[p].get("rb") == 1]
    assert any(b <= 16 for b in batches) and any(17 <= b <= 32 for b in batches), batches
    # 32- and 64-wide tiles over widths that are no whole number of tiles
    partial = {c[case].H for case, p, _ in PC.pairs("T") if PC.PLANS[p].get("tn_min", 0) >= 32}
    assert {272, 36, 20, 260, 4} <= partial, partial


def test_schedule_pairs_pin_the_tiles():
    """Group S: every plan holds tn_min=64 (as the reference arm), so no tile is left to widen and level_cap, flat_div
    and the scheduler's fields cannot reach a summation order."""
    assert PC.PLANS[PC.S_REFERENCE] == dict(tn_min=64)
    s_plans = {p for _, p, _ in PC.pairs("S")}
    for p in s_plans:
        kw = PC.PLANS[p]
        assert kw["tn_min"] == 64 and len(kw) >= 2 and "fuse_off" not in kw and "fuse_on" not in kw, p
        assert not set(kw) & {"pre_tn", "pl_tn", "wide", "rb", "steps_per_graph"}, p
    for case in ("td7-odd", "td3-k49", "sac-a25", "td7-w50"):
        assert {p for c, p, _ in PC.pairs("S") if c == case} == s_plans
    fields = set().union(*(PC.PLANS[p] for p in s_plans)) - {"tn_min"}
    assert fields == {"balance", "lpt", "sched_cap", "level_cap", "flat_div", "dispatch", "dpf", "xcd", *PC.WEIGHTS}
    assert {PC.PLANS[p]["balance"] for p in s_plans if "balance" in PC.PLANS[p]} == {0, 1, 2, 3}
    for w in PC.WEIGHTS:
        assert {PC.PLANS[p][w] for p in s_plans if w in PC.PLANS[p]} == {0, 1000}


def test_multistep_table():
    by_case = {}
    for case, base, k in PC.MULTI:
        by_case.setdefault(case, set()).add((base, k))
    full = {(b, k) for b in (None, "tn64") for k in (0, 2, 4, 5, 10, 16, -1)}
    assert by_case == {"td7-odd": full, "td3-k49": full, "sac-a25": full,
                       "td7-b1023": {(b, k) for b in (None, "tn64") for k in (-1, 4)}}
    assert PC.MULTI_EXTRA["td7"] == {"target_update_rate": 250}  # (no hard update in 20 steps: the K-step graphs replay)
    assert all(CASES[c].extra == {"target_update_rate": 3} for c in by_case if CASES[c].alg == "td7")
