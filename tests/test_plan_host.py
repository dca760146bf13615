"""The program planner (csrc/plan.cpp) on the host alone: the level scheduler through rle_schedule_plan and the
hazard check's conflict sweep through rle_hazard_scan, on small made-up programs.  No GPU.  Every expected value
is worked out by hand from the rules as plan.cpp states them (Prog::schedule, Prog::rebalance, Prog::op_weight,
hazard_scan); the comments carry the arithmetic."""

import ctypes
import random
import threading

import pytest

from rl import _engine

# ops.h, restated: the op kinds and the GEMM epilogue the scheduler's weights look at
OP_GEMM, OP_SAMPLE_GATHER, OP_HEAD, OP_STEP_END, OP_COPY = 1, 4, 5, 9, 11
EPI_STORE, EPI_ADAM = 0, 1
NO_CAP = 1 << 30
# rle_plan's scheduling fields, at the values PlanOptions starts from (no rebalance, program order)
KNOBS = dict(balance=0, tiny_w=30, uni_w=60, tiny_wg=2, pl_w=0, lap_w=60, head_w=60, adam_w=8, lpt=0)


def gemm(wg, weight=None, R=None, tn=64, epi=EPI_STORE, pre=0):
    """A GEMM op; its weight is R * tn / 1024 (+ adam_w with the Adam epilogue, + pl_w with has_pre >= 3)."""
    if R is None:
        R = weight * 1024 // tn
        assert R * tn // 1024 == weight
    return (OP_GEMM, wg, (R, tn, epi, pre))


def copy(wg):  # weight 8, as every kind without a rule of its own
    return (OP_COPY, wg, (0, 0, 0, 0))


def head(wg):  # weight head_w
    return (OP_HEAD, wg, (0, 0, 0, 0))


def gather(wg, lap):  # weight lap_w, or uni_w for the uniform sampler
    return (OP_SAMPLE_GATHER, wg, (lap, 0, 0, 0))


def step_end(mode, wg=1):  # weight tiny_w (8 when tiny_w is 0) unless mode is 1: then 8
    return (OP_STEP_END, wg, (mode, 0, 0, 0))


def item(ops, rd=(), wr=()):
    return (ops if isinstance(ops, list) else [ops], list(rd), list(wr))


def schedule(items, wg_cap=NO_CAP, **knobs):
    """[(level, position in the level, wg_begin)] per op, ops numbered through the items in order."""
    lib = _engine.lib()
    plan = _engine.Plan()
    for k, v in {**KNOBS, **knobs}.items():
        setattr(plan, k, v)
    of, kind, wg, attr, rd_off, rd, wr_off, wr = [], [], [], [], [0], [], [0], []
    for i, (ops, r, w) in enumerate(items):
        for k, n, a in ops:
            of.append(i), kind.append(k), wg.append(n), attr.extend(a)
        rd.extend(r), wr.extend(w)
        rd_off.append(len(rd)), wr_off.append(len(wr))
    arr = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
    n = len(kind)
    level, pos, begin = arr([-1] * n), arr([-1] * n), arr([-1] * n)
    rc = lib.rle_schedule_plan(arr(of), arr(kind), arr(wg), arr(attr), n, arr(rd_off), arr(rd), arr(wr_off), arr(wr),
                               len(items), ctypes.byref(plan), wg_cap, level, pos, begin)
    assert rc == 0, lib.rle_last_error()
    return [(level[q], pos[q], begin[q]) for q in range(n)]


def levels(items, **kw):
    return [lv for lv, _, _ in schedule(items, **kw)]


def test_entry_points_report_bad_input():
    """An unresolved plan field (-1 = "default" elsewhere) and an empty byte range are errors, not guesses."""
    lib = _engine.lib()
    with pytest.raises(AssertionError):
        schedule([item(copy(1))], lpt=-1)
    assert b"resolved" in lib.rle_last_error()
    with pytest.raises(AssertionError):
        scan([(0x2000, 0x2000, W, 0)], [0])
    assert b"lo < hi" in lib.rle_last_error()


# ---------------------------------------------------------------- dependencies

def test_raw_chain_takes_one_level_per_link():
    assert levels([item(copy(1), wr=[1]), item(copy(1), rd=[1], wr=[2]), item(copy(1), rd=[2])]) == [0, 1, 2]


def test_two_readers_of_one_resource_share_a_level():
    assert levels([item(copy(1), wr=[1]), item(copy(1), rd=[1]), item(copy(1), rd=[1])]) == [0, 1, 1]


def test_writer_goes_one_past_the_later_of_two_readers():
    """WAR: resource 1 is written on level 0 and read on levels 1 and 2 (the second reader also waits for
    resource 2); its next writer lands on level 3, not 2."""
    prog = [item(copy(1), wr=[1]), item(copy(1), rd=[1], wr=[2]), item(copy(1), rd=[1, 2]), item(copy(1), wr=[1])]
    assert levels(prog) == [0, 1, 2, 3]


def test_waw_pair_is_ordered():
    assert levels([item(copy(1), wr=[1]), item(copy(1), wr=[1])]) == [0, 1]


def test_negative_resource_ids_create_no_edge():
    assert levels([item(copy(1), wr=[-1]), item(copy(1), rd=[-1], wr=[-1]), item(copy(1), rd=[-1])]) == [0, 0, 0]


# ---------------------------------------------------------------- 12 ops per level

def test_thirteenth_independent_op_opens_a_second_level():
    got = schedule([item(copy(2)) for _ in range(13)])
    assert got[:12] == [(0, q, 2 * q) for q in range(12)]
    assert got[12] == (1, 0, 0)


def test_group_that_does_not_fit_is_deferred_whole():
    """Ten ops on level 0; a group of three would make 13, so all three go to level 1; a later group of two still
    fits level 0 (12 ops) behind the ten."""
    prog = [item(copy(1)) for _ in range(10)] + [item([copy(1), copy(1), copy(1)]), item([copy(1), copy(1)])]
    got = schedule(prog)
    assert got[10:13] == [(1, 0, 0), (1, 1, 1), (1, 2, 2)]
    assert got[13:] == [(0, 10, 10), (0, 11, 11)]


# ---------------------------------------------------------------- wg_cap

def test_item_that_takes_a_level_over_the_cap_is_deferred():
    """cap 100: 60 + 50 > 100, so the second item goes to level 1; 60 + 40 = 100 still fits level 0."""
    got = schedule([item(copy(60)), item(copy(50)), item(copy(40))], wg_cap=100)
    assert got == [(0, 0, 0), (1, 0, 0), (0, 1, 60)]


def test_item_larger_than_the_cap_takes_an_empty_level():
    """500 workgroups against a cap of 100: placed on the first empty level (an op alone may exceed the cap), and
    nothing joins it there."""
    assert levels([item(copy(500)), item(copy(10)), item(copy(500))], wg_cap=100) == [0, 1, 2]


# ---------------------------------------------------------------- balance

def window_prog(x, chain_weights=(64, 64, 64, 64), chain_wg=(100, 20, 10, 50), c2=None):
    """A chain c0 -> c1 -> c2 -> c3 on levels 0 .. 3 and an item x without producers (level 0 as soon as possible)
    whose only consumer y also reads c3's output (level 4): x may move to levels 1 .. 3.  Program order c0, x,
    c1, c2, c3, y; returns x's op index too."""
    c = [gemm(wg, w) for w, wg in zip(chain_weights, chain_wg)]
    prog = [item(c[0], wr=[1]), item(x, wr=[9]), item(c[1], rd=[1], wr=[2]), item(c2 or c[2], rd=[2], wr=[3]),
            item(c[3], rd=[3], wr=[4]), item(copy(5), rd=[9, 4])]
    return prog, 1


def test_balance_0_moves_nothing():
    prog, x = window_prog(copy(30))
    assert levels(prog, balance=0) == [0, 0, 1, 2, 3, 4]


def test_balance_1_moves_an_item_with_slack_to_the_lightest_level_of_its_window():
    """x (30 workgroups, weight 8) shares level 0 with c0: 130 workgroups.  Levels 1, 2, 3 hold 20, 10, 50, each
    with an op of weight 64 >= 8, and 50, 40, 80 < 130 with x: level 2, the one with the fewest, takes it.  x
    comes before c2 in program order, so it leads the level."""
    prog, x = window_prog(copy(30))
    got = schedule(prog, balance=1)
    assert [lv for lv, _, _ in got] == [0, 2, 1, 2, 3, 4]
    assert got[x] == (2, 0, 0) and got[3] == (2, 1, 30)


def test_balance_1_skips_a_level_whose_heaviest_op_is_lighter_than_the_item():
    """c2 weighs 4 < 8: level 2 is out, and of levels 1 (20) and 3 (50) the lighter takes x."""
    prog, x = window_prog(copy(30), chain_weights=(64, 64, 4, 64))
    assert levels(prog, balance=1)[x] == 1


def test_balance_1_skips_a_level_without_room_for_the_items_ops():
    """c2 as a group of 12 one-workgroup ops: level 2 has the fewest workgroups (12) but no op slot left."""
    prog, x = window_prog(copy(30), c2=[gemm(1, 64) for _ in range(12)])
    assert levels(prog, balance=1)[x] == 1


def slack_one(c0_wg, x_wg, c1_wg):
    """c0 and x on level 0, c1 on level 1, x's consumer y on level 2: level 1 is x's whole window."""
    return [item(gemm(c0_wg, 64), wr=[1]), item(copy(x_wg), wr=[9]), item(gemm(c1_wg, 64), rd=[1], wr=[2]),
            item(copy(5), rd=[9, 2])]


def test_balance_1_keeps_the_target_within_1024_workgroups():
    """min(wg_cap, 1024) with no wg_cap: 1004 + 20 = 1024 is allowed, 1005 + 20 is not."""
    assert levels(slack_one(2000, 20, 1004), balance=1) == [0, 1, 1, 2]
    assert levels(slack_one(2000, 20, 1005), balance=1) == [0, 0, 1, 2]
    assert levels(slack_one(2000, 20, 1004), balance=1, wg_cap=2048) == [0, 1, 1, 2]


def test_balance_1_target_must_end_strictly_below_the_source():
    """Level 0 holds 20 + 30 = 50 workgroups: level 1 with x would hold 49 (moves) or 50 (stays)."""
    assert levels(slack_one(20, 30, 19), balance=1) == [0, 1, 1, 2]
    assert levels(slack_one(20, 30, 20), balance=1) == [0, 0, 1, 2]


def test_balance_2_leaves_an_item_with_an_adam_gemm():
    """x as a GEMM with the Adam epilogue (weight 64 * 16 / 1024 + adam_w = 9 <= 64): moved by balance 1, kept
    by balance 2 and 3."""
    prog, x = window_prog(gemm(30, R=64, tn=16, epi=EPI_ADAM))
    assert levels(prog, balance=1)[x] == 2
    assert levels(prog, balance=2)[x] == 0
    assert levels(prog, balance=3)[x] == 0
    prog, x = window_prog(gemm(30, R=64, tn=16, epi=EPI_STORE))  # (the same GEMM without Adam moves under 2)
    assert levels(prog, balance=2)[x] == 2


def test_balance_3_needs_a_target_op_twice_as_heavy():
    """x weighs 8.  c2 at weight 15 < 16 bars level 2 under balance 3 (x goes to level 1, the lighter of the
    rest), not under balance 2; at weight 16 level 2 takes it under balance 3 too."""
    prog, x = window_prog(copy(30), chain_weights=(64, 64, 15, 64))
    assert levels(prog, balance=2)[x] == 2
    assert levels(prog, balance=3)[x] == 1
    prog, x = window_prog(copy(30), chain_weights=(64, 64, 16, 64))
    assert levels(prog, balance=3)[x] == 2


# ---------------------------------------------------------------- tiny-op move

def tiny_prog(mode):
    """One-workgroup chain c0 .. c3 of weights 16, 16, 64, 64 on levels 0 .. 3, and a step-end op e beside c0 whose
    consumer y sits on level 4.  Level 0 holds 2 workgroups, so no level can end below it with e: the first
    rebalance rule never applies."""
    w = (16, 16, 64, 64)
    return [item(gemm(1, w[0]), wr=[1]), item(step_end(mode), wr=[9]), item(gemm(1, w[1]), rd=[1], wr=[2]),
            item(gemm(1, w[2]), rd=[2], wr=[3]), item(gemm(1, w[3]), rd=[3], wr=[4]), item(copy(1), rd=[9, 4])]


def test_tiny_op_moves_under_the_first_heavier_op_of_its_window():
    """e weighs tiny_w = 30, the heaviest of level 0 (c0: 16).  Level 1's heaviest is 16, level 2's 64: level 2."""
    assert levels(tiny_prog(0), balance=1) == [0, 2, 1, 2, 3, 4]
    assert levels(tiny_prog(2), balance=1)[1] == 2
    assert levels(tiny_prog(0), balance=0)[1] == 0  # (the move is part of the rebalance pass)


def test_tiny_op_stays_with_tiny_w_0_or_tiny_wg_0():
    assert levels(tiny_prog(0), balance=1, tiny_w=0)[1] == 0
    assert levels(tiny_prog(0), balance=1, tiny_wg=0)[1] == 0
    # mode 1 (counters only) weighs 8 < c0's 16: not the heaviest of its level, so it stays as well
    assert levels(tiny_prog(1), balance=1)[1] == 0


# ---------------------------------------------------------------- lpt

LPT_OPS = [copy(3), gemm(5, 64), head(2), copy(7), gemm(4, R=512, tn=32), gather(6, lap=1)]  # weights 8 64 60 8 16 60


def test_lpt_sorts_each_level_heaviest_first_and_keeps_program_order_among_equals():
    """Weights 8, 64, 60, 8, 16, 60 -> order op 1, 2, 5 (60 = 60: program order), 4, 0, 3 (8 = 8); their workgroup
    counts 5, 2, 6, 4, 3, 7 give wg_begin 0, 5, 7, 13, 17, 20."""
    got = schedule([item(op) for op in LPT_OPS], lpt=1)
    assert got == [(0, 4, 17), (0, 0, 0), (0, 1, 5), (0, 5, 20), (0, 3, 13), (0, 2, 7)]


def test_without_lpt_a_level_keeps_program_order():
    got = schedule([item(op) for op in LPT_OPS], lpt=0)
    assert got == [(0, 0, 0), (0, 1, 3), (0, 2, 8), (0, 3, 10), (0, 4, 17), (0, 5, 21)]


def test_lpt_weights_follow_the_plans_knobs():
    """Adam GEMM 512 * 32 / 1024 + adam_w 8 = 24; pre-layer GEMM 16 + pl_w 10 = 26; uniform gather uni_w 25; both
    step ends 8 (tiny_w 0 counts as 8; mode 1 always does), in program order."""
    ops = [gemm(1, R=512, tn=32, epi=EPI_ADAM), step_end(0), gemm(1, R=512, tn=32, pre=3), step_end(1), gather(1, lap=0)]
    got = schedule([item(op) for op in ops], lpt=1, adam_w=8, pl_w=10, uni_w=25, tiny_w=0)
    assert [p for _, p, _ in got] == [2, 3, 0, 4, 1]


# ---------------------------------------------------------------- re-entrancy

def test_scheduler_is_reentrant():
    """Two host threads schedule the same program at once (ctypes drops the GIL): both get the lone call's answer.
    The planner has no state of its own, so one engine's build cannot pick up another thread's."""
    prog, _ = window_prog(copy(30))
    prog += [item(op) for op in LPT_OPS]
    alone = schedule(prog, balance=3, lpt=1)
    start = threading.Barrier(2)
    got = [[], []]

    def work(slot):
        start.wait()
        for _ in range(200):
            got[slot].append(schedule(prog, balance=3, lpt=1))

    threads = [threading.Thread(target=work, args=(s,)) for s in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(len(g) == 200 and all(r == alone for r in g) for g in got)


# ---------------------------------------------------------------- conflict scan

R, W = 0, 1


def scan(recs, items):
    """recs: (lo, hi, write, op); items[op]: its program item.  None, or the conflicting pair of ops."""
    lib = _engine.lib()
    n = len(recs)
    u64 = lambda v: (ctypes.c_ulonglong * max(n, 1))(*v)
    i32 = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
    a, b = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib.rle_hazard_scan(u64([r[0] for r in recs]), u64([r[1] for r in recs]), i32([r[2] for r in recs]),
                             i32([r[3] for r in recs]), n, i32(items), len(items), ctypes.byref(a), ctypes.byref(b))
    assert rc in (0, 1), lib.rle_last_error()
    assert (rc == 0) == (a.value == -1 and b.value == -1)
    return (a.value, b.value) if rc else None


def test_overlapping_reads_do_not_conflict():
    assert scan([(0x1000, 0x2000, R, 0), (0x1800, 0x2800, R, 1)], [0, 1]) is None


@pytest.mark.parametrize("first,second", [(W, R), (R, W), (W, W)])
def test_write_against_read_or_write_of_another_item_is_reported(first, second):
    assert scan([(0x1000, 0x2000, first, 0), (0x1800, 0x2800, second, 1)], [0, 1]) == (0, 1)
    # the pair is in address order: the range that begins lower first
    assert scan([(0x1800, 0x2800, first, 0), (0x1000, 0x2000, second, 1)], [0, 1]) == (1, 0)


def test_ops_of_one_item_are_exempt():
    assert scan([(0x1000, 0x2000, W, 0), (0x1800, 0x2800, W, 1)], [3, 3]) is None
    assert scan([(0x1000, 0x2000, W, 0), (0x1800, 0x2800, R, 0)], [0]) is None  # (and an op against itself)


def test_ranges_that_only_touch_do_not_conflict():
    assert scan([(0x1000, 0x2000, W, 0), (0x2000, 0x3000, W, 1)], [0, 1]) is None
    assert scan([(0x1000, 0x2001, W, 0), (0x2000, 0x3000, R, 1)], [0, 1]) == (0, 1)  # (one shared byte does)


# op 0 (item 0) stores a long range; op 3 (item 2) reads short ranges below it, op 1 (item 0 as well: exempt)
# short ranges inside it, which enter and leave the active list while the long range stays; then op 2 (item 1)
# reads inside the long range, and op 3 once more past its end
ACTIVE_LIST = [(0x100, 0x200, R, 3), (0x300, 0x400, R, 3), (0x1000, 0x9000, W, 0), (0x2000, 0x2100, R, 1),
               (0x3000, 0x3100, R, 1), (0x4000, 0x4100, R, 1), (0x8000, 0x8100, R, 2), (0x9000, 0x9100, R, 3)]
ACTIVE_ITEMS = [0, 0, 1, 2]


def test_long_range_stays_active_across_short_ones():
    assert scan(ACTIVE_LIST, ACTIVE_ITEMS) == (0, 2)
    assert scan(ACTIVE_LIST[:6] + ACTIVE_LIST[7:], ACTIVE_ITEMS) is None  # (without op 2's read: clean)


def test_record_order_does_not_matter():
    rng = random.Random(5)
    for _ in range(20):
        recs = ACTIVE_LIST[:]
        rng.shuffle(recs)
        assert scan(recs, ACTIVE_ITEMS) == (0, 2)
    assert scan(ACTIVE_LIST[::-1], ACTIVE_ITEMS) == (0, 2)
    assert scan([], []) is None
