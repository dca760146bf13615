#!/usr/bin/env python
"""Replay I/O measurements (DESIGN.md "Replay save / restore"): writes profiles/replay_io.json.

  sample   replay.sample(B) host latency, Humanoid shapes, 65,536-row LAP ring, B = 256 and 1024:
           median of 200 calls after 20 warm-ups.  Runs on any commit (the parent's per-row gather
           too): `--only sample --out parent.json` there, then `--parent parent.json` here.
  io       export / import of a 1M-row Humanoid LAP ring end to end into / out of NumPy arrays,
           against one pinned hipMemcpy of the same byte count in the same process (the floor).
  copy     copy.deepcopy of the same ring against one device-to-device hipMemcpy of its bytes.

usage: python tools/replay_io_bench.py [--only sample,io,copy] [--rows 1000000] [--parent FILE] [--out FILE]
"""

from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sac-td3-td7_amd"))

import torch  # noqa: E402

from rl import _engine as E  # noqa: E402
from rl.replay_memory import LAPReplayMemory  # noqa: E402

S, A = 376, 17  # Humanoid-v4


def _median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def bench_sample():
    rep = LAPReplayMemory(65536, "Humanoid-v4")
    rep.dev.fill_random(65536, 1)
    out = {}
    for B in (256, 1024):
        torch.manual_seed(0)
        med, best = _median_ms(lambda: rep.sample(B), 200, 20)
        u = torch.rand(B).numpy()
        ind_ms, _ = _median_ms(lambda: rep.dev.sample_indices(u), 200, 20)
        ind = rep.dev.sample_indices(u)
        gat_ms, _ = _median_ms(lambda: rep.dev.gather(ind), 200, 20)
        out[f"B{B}"] = {"sample_ms_median": med, "sample_ms_min": best, "sample_indices_ms_median": ind_ms,
                        "gather_ms_median": gat_ms}
    return out


def _timed(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), ts


def bench_io(rows):
    rep = LAPReplayMemory(rows, "Humanoid-v4")
    rep.dev.fill_random(rows, 2)
    nbytes = rows * (2 * S + A + 3) * 4
    out = {"rows": rows, "bytes": nbytes}
    # the floor: one pinned copy of the same byte count, each direction
    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    pin = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    d2h, _ = _timed(lambda: pin.copy_(dev, non_blocking=True))
    h2d, _ = _timed(lambda: dev.copy_(pin, non_blocking=True))
    del dev, pin
    out["pinned_d2h_s"], out["pinned_h2d_s"] = d2h, h2d
    # export into fresh NumPy arrays (the state_dict path), then into arrays whose pages exist already
    exp, exp_all = _timed(lambda: rep.dev.export_rows(0, rows, priority=True))
    arrays = rep.dev.export_rows(0, rows, priority=True)
    s, a, r, s2, d, p = arrays
    lib = E.lib()
    warm, _ = _timed(lambda: E._check(lib.rle_replay_export(rep.dev.h, 0, rows, E._fp(s), E._fp(a), E._fp(r),
                                                             E._fp(s2), E._fp(d), E._fp(p))))
    out["export_s"], out["export_runs_s"], out["export_touched_arrays_s"] = exp, exp_all, warm
    # the host side alone: one pass over the bytes from one array into another
    src = np.ones(nbytes // 4, np.float32)
    dst = np.empty_like(src)
    t0 = time.perf_counter()
    dst[:] = src
    out["host_copy_fresh_pages_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    dst[:] = src
    out["host_copy_touched_pages_s"] = time.perf_counter() - t0
    del src, dst
    dst_rep = LAPReplayMemory(rows, "Humanoid-v4")
    imp, imp_all = _timed(lambda: dst_rep.dev.import_rows(0, *arrays))
    out["import_s"], out["import_runs_s"] = imp, imp_all
    ptr, size, maxp = rep.dev.state()
    t0 = time.perf_counter()
    dst_rep.dev.set_state(ptr, size, maxp)
    out["set_state_s"] = time.perf_counter() - t0
    back = dst_rep.dev.export_rows(0, rows, priority=True)
    out["roundtrip_bit_identical"] = all(np.array_equal(x, y) for x, y in zip(arrays, back))
    out["export_over_floor"] = exp / d2h
    out["export_touched_over_floor"] = warm / d2h
    out["import_over_floor"] = imp / h2d
    out["export_GBps"], out["import_GBps"] = nbytes / exp / 1e9, nbytes / imp / 1e9
    out["pinned_d2h_GBps"], out["pinned_h2d_GBps"] = nbytes / d2h / 1e9, nbytes / h2d / 1e9
    return out


def bench_copy(rows):
    rep = LAPReplayMemory(rows, "Humanoid-v4")
    rep.dev.fill_random(rows, 3)
    ring_bytes = rows * (2 * 384 + 32 + 3) * 4  # the padded ring, as rle_replay_copy moves it
    a = torch.empty(ring_bytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    d2d, _ = _timed(lambda: b.copy_(a))
    del a, b
    twin = LAPReplayMemory(rows, "Humanoid-v4")
    cp, _ = _timed(lambda: twin.dev.copy_from(rep.dev))
    del twin
    t0 = time.perf_counter()
    twin = copy.deepcopy(rep)
    dc = time.perf_counter() - t0
    same = all(np.array_equal(x, y) for x, y in zip(twin.dev.export_rows(0, 4096, priority=True),
                                                    rep.dev.export_rows(0, 4096, priority=True)))
    return {"rows": rows, "ring_bytes": ring_bytes, "d2d_memcpy_s": d2d, "copy_from_s": cp,
            "deepcopy_s_incl_new_ring": dc, "copy_over_d2d": cp / d2d, "copy_GBps": ring_bytes / cp / 1e9,
            "d2d_GBps": ring_bytes / d2d / 1e9, "first_rows_identical": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="sample,io,copy")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--parent", default=None, help="JSON of `--only sample` run on the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replay_io.json"))
    args = ap.parse_args()
    only = set(args.only.split(","))
    res = {"device": torch.cuda.get_device_name(0), "io_rows": getattr(E, "REPLAY_IO_ROWS", None)}
    if "sample" in only:
        res["sample"] = bench_sample()
    if "io" in only:
        res["io"] = bench_io(args.rows)
    if "copy" in only:
        res["copy"] = bench_copy(args.rows)
    if args.parent and "sample" in res:
        par = json.load(open(args.parent))["sample"]
        res["sample_parent"] = par
        res["sample_speedup"] = {k: par[k]["sample_ms_median"] / v["sample_ms_median"]
                                 for k, v in res["sample"].items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
