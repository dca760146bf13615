#!/usr/bin/env python
"""What the device state normalisation costs (DESIGN.md "Offline TD3"): adds the key "normalisation" to
profiles/offline_td3_bench.json.

A 1M-row Humanoid ring (S 376, rows padded to 384 floats).  Timed, each --rounds times after one warm-up call,
host wall time around the synchronous entry (median, min, max):

* rle_replay_state_stats: two passes over `state`, 4 * Sp * size bytes each (the issue counts 4 * S * size: the
  kernel reads the pad columns too, whole 64-byte-aligned rows);
* rle_replay_normalize_states (shift 0, scale 1, so the ring stays what it was between rounds): 2 * 4 * Sp * size
  bytes in and the same out;
* the host round trip they replace, alternating with them: rle_replay_export of state and next_state, the
  statistics and the transform in NumPy, rle_replay_import.

usage: python tools/replay_norm_bench.py [--rows 1000000] [--rounds 5] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sac-td3-td7_amd"))

S, A = 376, 17  # Humanoid-v4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "offline_td3_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from rl import _engine as E

    n, Sp = args.rows, (S + 15) // 16 * 16
    rep = E.Replay(n, S, A, False, device=0)
    rep.fill_random(n, seed=1)
    zero, one = np.zeros(S, np.float32), np.ones(S, np.float32)

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    def host_round_trip():
        s, a, r, s2, d = rep.export_rows(0, n)
        mean = s.mean(0, dtype=np.float64).astype(np.float32)
        scale = s.std(0, dtype=np.float64).astype(np.float32) + np.float32(1e-3)
        del mean, scale  # (the statistics are computed; the transform below keeps the ring what it was)
        s -= zero
        s /= one
        s2 -= zero
        s2 /= one
        rep.import_rows(0, s, a, r, s2, d)
        rep.set_state(0, n, 1.0)

    rep.state_stats()
    rep.normalize_states(zero, one)
    t = {"stats": [], "normalize": [], "host": []}
    for _ in range(args.rounds):
        t["stats"].append(timed(rep.state_stats))
        t["normalize"].append(timed(lambda: rep.normalize_states(zero, one)))
        t["host"].append(timed(host_round_trip))
    bytes_ = {"stats": 2 * 4 * Sp * n, "normalize": 2 * 2 * 4 * Sp * n}
    res = {"device": torch.cuda.get_device_name(0),
           "config": f"Humanoid ring S {S} (rows of {Sp} floats), {n} rows, {args.rounds} rounds, host wall time"}
    for k, v in t.items():
        med = statistics.median(v)
        res[k] = {"seconds": [round(x, 6) for x in v], "median_s": round(med, 6), "min_s": round(min(v), 6),
                  "max_s": round(max(v), 6)}
        if k in bytes_:
            res[k]["bytes"] = bytes_[k]
            res[k]["GB_per_s"] = round(bytes_[k] / med / 1e9, 1)
    res["host_over_device"] = round(res["host"]["median_s"] / (res["stats"]["median_s"] + res["normalize"]["median_s"]), 1)
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            out = json.load(fh)
    out["normalisation"] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
