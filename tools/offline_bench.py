#!/usr/bin/env python
"""What TD7's offline mode costs (DESIGN.md "Offline TD7"): writes profiles/offline_bench.json.

The flagship shape of bench.py -- TD7 on Humanoid-v4, hidden 256, batch 256, a 1M-row LAP replay -- as two
engines in one process on one replay each, one online (rle_config bc_lambda 0) and one offline (bc_lambda
0.1), with the same weights.  After a warm-up each runs --rounds bursts of rle_step_timed(--steps), the two
alternating (online, offline, online, ...), so clock and thermal drift fall on both alike.  Printed: every
burst's rate, the two medians, their ratio, the spread of the online bursts (what "within run-to-run spread"
is measured against), the levels per policy / plain step of both, and the offline policy step's levels
(rle_graph_describe) with the new op in place.

usage: python tools/offline_bench.py [--steps 2000] [--rounds 5] [--warmup 200] [--lmbda 0.1] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sac-td3-td7_amd"))

N_REPLAY = 1_000_000
S, A, H, B = 376, 17, 256, 256  # Humanoid-v4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--lmbda", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "offline_bench.json"))
    args = ap.parse_args()

    import torch
    from rl import _engine as E
    from rl.nn.layout import init_agent

    nets = init_agent("td7", S, A, H, 123)

    def engine(lmbda, seed):
        eng = E.Engine(E.make_config(E.RLE_TD7, S, A, H, B, use_lap=True, seed=111, bc_lambda=lmbda))
        for net, params in nets.items():
            for name, v in params.items():
                eng.set_param(net, name, v)
        rep = E.Replay(N_REPLAY, S, A, True, device=0)
        rep.fill_random(N_REPLAY, seed=seed)
        eng.bind(rep)
        return eng, rep

    engs = {"online": engine(0.0, 0), "offline": engine(args.lmbda, 0)}
    res = {"device": torch.cuda.get_device_name(0),
           "config": f"TD7 Humanoid-v4 hidden {H} batch {B} LAP {N_REPLAY} rows, rle_step_timed({args.steps}) "
                     f"x {args.rounds} per mode, alternating; offline bc_lambda {args.lmbda}",
           "levels_per_step": {}, "bursts_steps_per_s": {k: [] for k in engs}}
    for k, (eng, _) in engs.items():
        lp, lpl = eng.graph_stats()
        res["levels_per_step"][k] = {"policy": lp, "plain": lpl}
        eng.step_timed(args.warmup)
    for _ in range(args.rounds):
        for k, (eng, _) in engs.items():
            ms = eng.step_timed(args.steps)
            res["bursts_steps_per_s"][k].append(round(args.steps / (ms * 1e-3), 1))
    med = {k: statistics.median(v) for k, v in res["bursts_steps_per_s"].items()}
    on = res["bursts_steps_per_s"]["online"]
    res["median_steps_per_s"] = med
    res["offline_over_online"] = round(med["offline"] / med["online"], 4)
    res["online_spread"] = round((max(on) - min(on)) / med["online"], 4)
    res["offline_policy_step_levels"] = engs["offline"][0].describe(0).splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "offline_policy_step_levels"}))
    print("\n".join(res["offline_policy_step_levels"]))


if __name__ == "__main__":
    main()
