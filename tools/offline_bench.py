#!/usr/bin/env python
"""What the offline modes cost (DESIGN.md "Offline TD7", "Offline TD3", "Offline SAC"): writes
profiles/offline_bench.json (--algo td7, the default), profiles/offline_td3_bench.json (--algo td3) or
profiles/offline_sac_bench.json (--algo sac).

The flagship shape of bench.py -- TD7 on Humanoid-v4, hidden 256, batch 256, a 1M-row LAP replay -- as two
engines in one process on one replay each, one online (rle_config bc_lambda 0) and one offline (bc_lambda
0.1), with the same weights.  After a warm-up each runs --rounds bursts of rle_step_timed(--steps), the two
alternating (online, offline, online, ...), so clock and thermal drift fall on both alike.  Printed: every
burst's rate, the two medians, their ratio, the spread of the online bursts (what "within run-to-run spread"
is measured against), the levels per policy / plain step of both, and the offline policy step's levels
(rle_graph_describe) with the new op in place.

--algo td3: the same for TD3+BC on bench.py's TD3 shape -- HalfCheetah-v4, hidden 256, batch 256, a 1M-row
replay -- online (rle_create) against offline (rle_config_ext bc_alpha, --alpha, default 2.5).

--algo sac: the same for AWAC on bench.py's SAC shape -- Humanoid-v4, hidden 256, batch 256, a 1M-row replay --
online at a fixed temperature of 0 (rle_create, tmp 0) against offline (rle_config_ext awac_lambda, --awac,
default 1.0).

usage: python tools/offline_bench.py [--algo td7|td3|sac] [--steps 2000] [--rounds 5] [--warmup 200] [--lmbda 0.1]
                                     [--alpha 2.5] [--awac 1.0] [--out FILE]
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
S3, A3 = 17, 6                  # HalfCheetah-v4 (--algo td3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--lmbda", type=float, default=0.1)
    ap.add_argument("--algo", choices=("td7", "td3", "sac"), default="td7")
    ap.add_argument("--alpha", type=float, default=2.5)
    ap.add_argument("--awac", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    td3, sac = args.algo == "td3", args.algo == "sac"
    if args.out is None:
        name = "offline_td3_bench.json" if td3 else "offline_sac_bench.json" if sac else "offline_bench.json"
        args.out = os.path.join(REPO, "profiles", name)

    import torch
    from rl import _engine as E
    from rl.nn.layout import init_agent

    s_dim, a_dim = (S3, A3) if td3 else (S, A)
    nets = init_agent(args.algo, s_dim, a_dim, H, 123)

    def engine(weight, seed):
        if td3:  # (bench.py's TD3 run: no LAP; online through rle_create, offline through rle_create_ext)
            cfg = E.make_config(E.RLE_TD3, s_dim, a_dim, H, B, use_lap=False, seed=111)
            eng = E.Engine(cfg, ext=E.make_config_ext(bc_alpha=weight) if weight else None)
        elif sac:  # (online: the fixed-temperature program at tmp = 0, whose critic step the offline mode keeps)
            cfg = E.make_config(E.RLE_SAC, s_dim, a_dim, H, B, use_lap=False, seed=111, tmp=0.0)
            eng = E.Engine(cfg, ext=E.make_config_ext(awac_lambda=weight) if weight else None)
        else:
            eng = E.Engine(E.make_config(E.RLE_TD7, s_dim, a_dim, H, B, use_lap=True, seed=111, bc_lambda=weight))
        for net, params in nets.items():
            for name, v in params.items():
                eng.set_param(net, name, v)
        rep = E.Replay(N_REPLAY, s_dim, a_dim, not (td3 or sac), device=0)
        rep.fill_random(N_REPLAY, seed=seed)
        eng.bind(rep)
        return eng, rep

    engs = {"online": engine(0.0, 0), "offline": engine(args.alpha if td3 else args.awac if sac else args.lmbda, 0)}
    what = (f"TD3 HalfCheetah-v4 hidden {H} batch {B} {N_REPLAY} rows" if td3
            else f"SAC Humanoid-v4 tmp 0 hidden {H} batch {B} {N_REPLAY} rows" if sac
            else f"TD7 Humanoid-v4 hidden {H} batch {B} LAP {N_REPLAY} rows")
    res = {"device": torch.cuda.get_device_name(0),
           "config": f"{what}, rle_step_timed({args.steps}) x {args.rounds} per mode, alternating; offline "
                     + (f"bc_alpha {args.alpha}" if td3 else f"awac_lambda {args.awac}" if sac
                        else f"bc_lambda {args.lmbda}"),
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
    lv = res["levels_per_step"]  # (levels per step pair, policy_freq 2: what one extra level would explain)
    res["levels_online_over_offline"] = round((lv["online"]["policy"] + lv["online"]["plain"])
                                              / (lv["offline"]["policy"] + lv["offline"]["plain"]), 4)
    res["offline_policy_step_levels"] = engs["offline"][0].describe(0).splitlines()
    if td3 and os.path.exists(args.out):  # (tools/replay_norm_bench.py keeps its figures in the same file)
        with open(args.out) as fh:
            res.update({k: v for k, v in json.load(fh).items() if k == "normalisation"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "offline_policy_step_levels"}))
    print("\n".join(res["offline_policy_step_levels"]))


if __name__ == "__main__":
    main()
