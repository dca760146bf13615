#!/usr/bin/env python
"""What gradient-norm clipping costs (DESIGN.md "Gradient clipping"): writes profiles/grad_clip_bench.json.

bench.py's three shapes at batch 256 -- TD7 on Humanoid-v4 (LAP), TD3 on HalfCheetah-v4, SAC on Humanoid-v4, hidden
256, a 1M-row replay -- each as two engines in one process on one replay each, with the same weights: one
unclipped (rle_set_grad_clip never called: the program and kernel instance of every run so far) and one clipped
(rle_set_grad_clip(--max-norm)).  After a warm-up each runs --rounds bursts of rle_step_timed(--steps), the two
alternating (unclipped, clipped, unclipped, ...), so clock and thermal drift fall on both alike.  Recorded per
algorithm: every burst's rate, the two medians, their ratio, the spread of the unclipped bursts, the levels per
policy / plain step of both (rle_graph_stats), the clipped engine's last {total, coef} per optimizer, and the
clipped policy step's levels (rle_graph_describe) with the norm passes, OP_CLIP and the Adam passes in place.

The threshold only has to be a positive number: the clipped program does the same work whether a step's
coefficient comes out below 1 or at 1 (the gradient is multiplied either way).

usage: python tools/grad_clip_bench.py [--algos td7,td3,sac] [--steps 2000] [--rounds 5] [--warmup 200]
                                       [--max-norm 1.0] [--out FILE]
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
H, B = 256, 256
SHAPES = {"td7": ("Humanoid-v4", 376, 17), "td3": ("HalfCheetah-v4", 17, 6), "sac": ("Humanoid-v4", 376, 17)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algos", default="td7,td3,sac")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_clip_bench.json"))
    args = ap.parse_args()

    import torch
    from rl import _engine as E
    from rl.nn.layout import init_agent

    algo_id = {"td7": E.RLE_TD7, "td3": E.RLE_TD3, "sac": E.RLE_SAC}
    out = {"device": torch.cuda.get_device_name(0),
           "config": f"hidden {H} batch {B} {N_REPLAY} rows, rle_step_timed({args.steps}) x {args.rounds} per mode, "
                     f"alternating; clipped: rle_set_grad_clip({args.max_norm})"}
    for alg in args.algos.split(","):
        env, s_dim, a_dim = SHAPES[alg]
        nets = init_agent(alg, s_dim, a_dim, H, 123)
        lap = alg == "td7"

        def engine(clip):
            eng = E.Engine(E.make_config(algo_id[alg], s_dim, a_dim, H, B, use_lap=lap, seed=111))
            if clip:
                eng.set_grad_clip(args.max_norm)
            for net, params in nets.items():
                for name, v in params.items():
                    eng.set_param(net, name, v)
            rep = E.Replay(N_REPLAY, s_dim, a_dim, lap, device=0)
            rep.fill_random(N_REPLAY, seed=0)
            eng.bind(rep)
            return eng, rep

        engs = {"unclipped": engine(False), "clipped": engine(True)}
        res = {"shape": f"{alg.upper()} {env}", "levels_per_step": {}, "bursts_steps_per_s": {k: [] for k in engs}}
        for k, (eng, _) in engs.items():
            lp, lpl = eng.graph_stats()
            res["levels_per_step"][k] = {"policy": lp, "plain": lpl}
            eng.step_timed(args.warmup)
        for _ in range(args.rounds):
            for k, (eng, _) in engs.items():
                ms = eng.step_timed(args.steps)
                res["bursts_steps_per_s"][k].append(round(args.steps / (ms * 1e-3), 1))
        med = {k: statistics.median(v) for k, v in res["bursts_steps_per_s"].items()}
        un = res["bursts_steps_per_s"]["unclipped"]
        res["median_steps_per_s"] = med
        res["clipped_over_unclipped"] = round(med["clipped"] / med["unclipped"], 4)
        res["unclipped_spread"] = round((max(un) - min(un)) / med["unclipped"], 4)
        res["last_total_coef"] = {k: [round(x, 6) for x in v] for k, v in engs["clipped"][0].grad_clip_stats().items()}
        res["clipped_policy_step_levels"] = engs["clipped"][0].describe(0).splitlines()
        out[alg] = res
        print(json.dumps({k: v for k, v in res.items() if k != "clipped_policy_step_levels"}), flush=True)
        for eng, rep in engs.values():
            eng.close()
            rep.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
