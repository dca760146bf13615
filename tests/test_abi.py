"""CPU-side checks of the C-ABI boundary: library loads, every declared symbol exported."""

import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "rle.h")


def declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"\b(rle_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_entry_points():
    names = declared()
    for n in ("rle_create", "rle_step", "rle_replay_create", "rle_replay_append", "rle_set_tapes",
              "rle_act", "rle_last_error"):
        assert n in names


def test_library_exports_every_symbol():
    from rl import _engine

    if not os.path.exists(_engine.LIB_PATH):
        pytest.fail("librle.so not built (run __graft_entry__.build())")
    lib = _engine.lib()  # loads without a GPU (no HIP calls at load)
    for n in declared():
        assert hasattr(lib, n), n
    assert set(_engine.SIGNATURES) == set(declared())


def test_errors_are_reported_not_raised_across_abi():
    from rl import _engine

    lib = _engine.lib()
    import ctypes

    out = ctypes.c_void_p()
    rc = lib.rle_replay_create(0, -5, 3, 2, 0, ctypes.byref(out))
    assert rc == -1
    assert b"bad args" in lib.rle_last_error()


def test_aql_wait_policy_releases_the_host_core():
    """rle_step's AQL wait (dispatch.cpp aql_wait_step): sleep while more than the 150 us spin tail of the
    expected duration remains (slices <= 2 ms), spin for the tail, time out past the limit (the engine's
    queue is then closed: aql_submit refuses every later packet).  No GPU: the policy alone."""
    import ctypes

    from rl import _engine

    lib = _engine.lib()
    sl = ctypes.c_double()

    def plan(expected, elapsed, timeout=60.0):
        return lib.rle_aql_wait_plan(expected, elapsed, timeout, ctypes.byref(sl)), sl.value

    assert plan(250_000.0, 0.0) == (1, 2000.0)          # a 2000-step burst: sleep in 2 ms slices
    act, us = plan(250_000.0, 249_000.0)
    assert act == 1 and abs(us - 850.0) < 1e-6          # ... up to 150 us before the expected end
    assert plan(250_000.0, 249_900.0)[0] == 0           # then spin
    assert plan(100.0, 0.0)[0] == 0                     # short flushes never sleep
    assert plan(250_000.0, 400_000.0)[0] == 0           # overran the estimate: spin, no more sleeping
    assert plan(250_000.0, 61e6)[0] == 2                # past 60 s: time out
    assert plan(250_000.0, 1.5e6, timeout=1.0)[0] == 2


def test_aql_failed_queue_fails_fast_and_doorbells_stay_in_one_ring_pass():
    """A queue closed by a timed-out burst refuses new bursts and completes at once (so rle_destroy and every
    later entry point return instead of waiting another 60 s), also for engines sharing its hardware queue;
    doorbell groups never straddle the ring's end (dispatch.cpp aql_doorbell_after, the rocprofv3 crash of
    profiles/r05_prof_crash.txt).  No GPU: rle_aql_selftest reaches no HSA call."""
    from rl import _engine

    lib = _engine.lib()
    assert lib.rle_aql_selftest() == 0, lib.rle_last_error()


# ops.h, restated: kLevelOps ops per launch, at most kMaxLevelWG workgroups in one (8 of them the prefetch
# workgroups), kThreads threads per workgroup; OP_GEMM is kind 1 and carries a variant id, any other kind k has k >> 4.
LEVEL_OPS, MAX_LEVEL_WG, THREADS, PREFETCH_WG, OP_GEMM = 12, 0xfffe, 256, 8, 1
D_OPS, NEXT_OPS, KS = 0x7f0000100000, 0x7f0000900000, 3


def _level_plan(kind, vid, wg_begin, nwg, next_nops):
    """rle_level_plan's packets as dicts, with its return code and the size of an op descriptor."""
    import ctypes

    from rl import _engine

    lib = _engine.lib()
    nops = len(kind)
    arr = lambda v: (ctypes.c_int * nops)(*v)
    out = (ctypes.c_uint * (22 * 8))()
    n, op_bytes = ctypes.c_int(-1), ctypes.c_int()
    rc = lib.rle_level_plan(arr(kind), arr(vid), arr(wg_begin), nops, nwg, D_OPS, NEXT_OPS, next_nops, KS, out, 8,
                            ctypes.byref(n), ctypes.byref(op_bytes))
    packets = []
    for i in range(max(n.value, 0)):
        w = out[22 * i:22 * i + 22]
        addr = lambda j: w[j] | (w[j + 1] << 32)
        packets.append(dict(entry=w[:12], ops=addr(12), trace=addr(14), next=addr(16), next_lines=w[18], grid=w[20],
                            ks=w[21]))
    return rc, packets, op_bytes.value


def _level(nops):
    """A level of nops ops of 1 .. 7 workgroups: GEMMs with distinct variant ids, and kinds up to 16 (OP_BC)."""
    kind = [OP_GEMM if q % 3 == 0 else 2 + q % 15 for q in range(nops)]
    vid = [100 + 7 * q if k == OP_GEMM else -1 for q, k in enumerate(kind)]
    count = [1 + (5 * q) % 7 for q in range(nops)]
    wg_begin = [sum(count[:q]) for q in range(nops)]
    return kind, vid, wg_begin, sum(count)


@pytest.mark.parametrize("nops,nlaunch", [(1, 1), (12, 1), (13, 2), (25, 3)])
def test_level_planner_splits_packs_and_prefetches(nops, nlaunch):
    """dispatch.cpp level_launches, the one place that knows the format of a level launch (no GPU): a level of
    more than 12 ops is split into launches of 12; each launch's op table holds its ops relative to its first
    workgroup, 0xffff past the last; a launch prefetches the ops of the launch after it -- the rest of its own
    level, then the next level's first 12 -- with 8 leading workgroups and bit 31 of entry 0."""
    kind, vid, wg_begin, nwg = _level(nops)
    next_nops = 30
    rc, packets, op_bytes = _level_plan(kind, vid, wg_begin, nwg, next_nops)
    assert rc == 0 and len(packets) == nlaunch
    assert op_bytes % 64 == 0
    lines = op_bytes // 64
    for i, p in enumerate(packets):
        q0, q1 = LEVEL_OPS * i, min(LEVEL_OPS * (i + 1), nops)
        w0, w1 = wg_begin[q0], wg_begin[q1] if q1 < nops else nwg
        assert p["ks"] == KS and p["trace"] == 0
        assert p["ops"] == D_OPS + q0 * op_bytes
        for q in range(LEVEL_OPS):
            e = p["entry"][q] & 0x7fffffff if q == 0 else p["entry"][q]
            if q0 + q < q1:
                k = kind[q0 + q]
                v = vid[q0 + q] if k == OP_GEMM else k >> 4
                assert e == (wg_begin[q0 + q] - w0) | (k & 15) << 16 | v << 20, (i, q)
            else:
                assert e == 0xffff, (i, q)
        last = i + 1 == nlaunch
        following = min(next_nops, LEVEL_OPS) if last else min(nops - q1, LEVEL_OPS)
        assert p["next"] == (NEXT_OPS if last else D_OPS + q1 * op_bytes)
        assert p["next_lines"] == min(following * lines, 2 * THREADS) > 0
        assert p["entry"][0] >> 31 == 1
        assert p["grid"] == w1 - w0 + PREFETCH_WG
    if nops == 13:
        assert packets[0]["next"] == D_OPS + 12 * op_bytes and packets[0]["next_lines"] == min(lines, 2 * THREADS)
        assert packets[1]["next"] == NEXT_OPS and packets[1]["next_lines"] == min(12 * lines, 2 * THREADS)
        assert _level_plan(kind, vid, wg_begin, nwg, 5)[1][1]["next_lines"] == min(5 * lines, 2 * THREADS)


def test_level_planner_without_a_next_level_and_at_the_workgroup_bound():
    """Nothing to prefetch: no bit 31 and the grid is exactly the level's workgroups.  A launch may have
    kMaxLevelWG - 8 workgroups (the prefetch workgroups count against the 16-bit field); one more is the
    error it always was, with no packet returned."""
    kind, vid, wg_begin, nwg = _level(12)
    rc, packets, _ = _level_plan(kind, vid, wg_begin, nwg, 0)
    assert rc == 0 and len(packets) == 1
    assert packets[0]["entry"][0] >> 31 == 0 and packets[0]["next_lines"] == 0 and packets[0]["grid"] == nwg

    from rl import _engine

    rc, packets, _ = _level_plan([OP_GEMM], [3], [0], MAX_LEVEL_WG - 8, 4)
    assert rc == 0 and packets[0]["grid"] == MAX_LEVEL_WG
    rc, packets, _ = _level_plan([OP_GEMM], [3], [0], MAX_LEVEL_WG - 7, 4)
    assert rc == -2 and packets == [], _engine.lib().rle_last_error()  # RLE_EHIP
    # ... also when it is a later launch of the level that is too large: nothing of the level is returned
    kind, vid, wg_begin, nwg = _level(13)
    rc, packets, _ = _level_plan(kind, vid, wg_begin, wg_begin[12] + MAX_LEVEL_WG - 7, 4)
    assert rc == -2 and packets == []


def test_level_planner_is_reentrant():
    """Two host threads plan the same level at once (ctypes drops the GIL), each into its own list: both get
    the list a lone call gets.  The planner has no state of its own -- nothing global or thread-local records
    launches -- so one engine's capture cannot pick up another thread's launches."""
    import threading

    kind, vid, wg_begin, nwg = _level(25)
    alone = _level_plan(kind, vid, wg_begin, nwg, 9)
    assert alone[0] == 0 and len(alone[1]) == 3
    start = threading.Barrier(2)
    got = [[], []]

    def work(slot):
        start.wait()
        for _ in range(200):
            got[slot].append(_level_plan(kind, vid, wg_begin, nwg, 9))

    threads = [threading.Thread(target=work, args=(s,)) for s in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(len(g) == 200 and all(r == alone for r in g) for g in got)


def test_ctypes_structs_match_the_header_layout(tmp_path):
    """rl/_engine.py Config / Plan mirror rle_config / rle_plan field by field: a C program compiled against
    include/rle.h prints each struct's size and every field's offset (gcc on the host, no GPU)."""
    import ctypes
    import shutil
    import subprocess

    from rl import _engine

    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = []
    for cname, cls in (("rle_config", _engine.Config), ("rle_plan", _engine.Plan)):
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, *_ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rle.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.splitlines())
    for cname, cls in (("rle_config", _engine.Config), ("rle_plan", _engine.Plan)):
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, *_ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_create_rejects_bad_activation_codes_before_any_hip_call():
    """rle_create validates rle_config.act_* (RLE_ACT_DEFAULT..RLE_ACT_IDENTITY; act_encoder is TD7's) before it
    touches a device, so the errors come back through the ABI on a host without a GPU."""
    import ctypes

    from rl import _engine as E

    lib = E.lib()
    out = ctypes.c_void_p()
    cfg = E.make_config(E.RLE_TD7, 17, 6, 32, 16)
    cfg.act_actor = 7
    assert lib.rle_create(ctypes.byref(cfg), ctypes.byref(out)) == -1
    assert b"activation" in lib.rle_last_error()
    cfg = E.make_config(E.RLE_TD3, 17, 6, 32, 16, act_encoder="elu")
    assert lib.rle_create(ctypes.byref(cfg), ctypes.byref(out)) == -1
    assert b"act_encoder" in lib.rle_last_error()
    with pytest.raises(ValueError, match="activation"):
        E.make_config(E.RLE_SAC, 17, 6, 32, 16, act_critic="tanh")
