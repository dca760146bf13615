#!/usr/bin/env python
"""What critic dropout costs on top of LayerNorm critics, and that the LayerNorm-only programs kept their rate
(DESIGN.md "Critic dropout": the check behind the decision to give the dropout path a kernel instance of its own,
drop_level.hip, and the re-check after it): writes profiles/critic_dropout_bench.json.

tools/layer_norm_bench.py's method: bench.py's synthetic workload -- TD3 on HalfCheetah-v4 and SAC on Humanoid-v4,
hidden 256, batch 256, a 1M-row replay, random weights -- on two libraries that alternate in one call, every run a
fresh child process with one engine in it.  The parent commit's library (--parent-lib) runs the LayerNorm + ReLU
programs; this tree's runs the same programs (p = 0) and the same with rle_set_critic_dropout(0.01).  In every pair
the parent's run of a shape comes first.  Per case and library: every run's steps/s, the median, the min-max range
and the levels per policy / plain step (rle_graph_stats).  This library's LayerNorm-only median is then placed against
the parent's own min-max range, and the dropout program against the parent's LayerNorm-only one.

usage: python tools/critic_dropout_bench.py --parent-lib PATH [--pairs 4] [--steps 4000] [--warmup 200] [--out FILE]
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sac-td3-td7_amd"))

N_REPLAY = 1_000_000
H, B = 256, 256
P_DROP = 0.01
SHAPES = {"td3": ("HalfCheetah-v4", 17, 6), "sac": ("Humanoid-v4", 376, 17)}
NEW = ("rle_set_critic_dropout", "rle_get_critic_dropout", "rle_dropout_mask")
# (name, dropout probability); the parent's library runs the first only
CASES = [("ln_relu", 0.0), ("ln_relu_drop", P_DROP)]


def child(args):
    """One library, one case (--only alg:case): a JSON line on stdout."""
    from rl import _engine as E
    from rl.nn.layout import init_agent

    has_drop = hasattr(ctypes.CDLL(E.LIB_PATH), NEW[0])
    if not has_drop:  # (a library from before the entry points: bind what it has)
        for name in NEW:
            E.SIGNATURES.pop(name, None)
    algo_id = {"td3": E.RLE_TD3, "sac": E.RLE_SAC}
    alg, case = args.only.split(":")
    env, s_dim, a_dim = SHAPES[alg]
    p = dict(CASES)[case]
    if p and not has_drop:
        raise SystemExit("this library has no rle_set_critic_dropout")
    eng = E.Engine(E.make_config(algo_id[alg], s_dim, a_dim, H, B, use_lap=False, seed=111))
    eng.set_layer_norm(True)
    if p:
        eng.set_critic_dropout(p)
    for net, params in init_agent(alg, s_dim, a_dim, H, 123).items():
        for pname, v in params.items():
            eng.set_param(net, pname, v)
    rep = E.Replay(N_REPLAY, s_dim, a_dim, False, device=0)
    rep.fill_random(N_REPLAY, seed=0)
    eng.bind(rep)
    eng.step_timed(args.warmup)
    ms = eng.step_timed(args.steps)
    lp, lpl = eng.graph_stats()
    print(json.dumps({"alg": alg, "env": env, "case": case, "steps_per_s": round(args.steps / (ms * 1e-3), 1),
                      "levels": {"policy": lp, "plain": lpl}}), flush=True)
    eng.close()
    rep.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=False, default=None, help="librle.so of the commit before critic dropout")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "critic_dropout_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    libs = ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else []) + [("this", None)]
    runs = {}  # (library, alg, case) -> {"steps_per_s": [...], "levels": ...}
    for pair in range(args.pairs):
        for alg in SHAPES:
            for lib, path in libs:
                for case, p in CASES:
                    if lib == "parent" and p:
                        continue
                    env = dict(os.environ)
                    env.pop("RLE_LIB", None)
                    if path:
                        env["RLE_LIB"] = path
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--only", f"{alg}:{case}", "--steps",
                           str(args.steps), "--warmup", str(args.warmup)]
                    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=300)
                    if r.returncode != 0:  # (nothing more on the GPU after a failed child)
                        raise SystemExit(f"child ({lib} {alg}:{case}) exited with {r.returncode}")
                    for line in r.stdout.splitlines():
                        d = json.loads(line)
                        slot = runs.setdefault((lib, d["alg"], d["case"]), {"steps_per_s": [], "levels": d["levels"]})
                        slot["steps_per_s"].append(d["steps_per_s"])
                        print(pair, lib, line, flush=True)

    import torch

    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "?",
           "config": f"hidden {H} batch {B} {N_REPLAY} rows, LayerNorm + ReLU critics, dropout p {P_DROP}, "
                     f"rle_step_timed({args.steps}) after {args.warmup} warm-up steps, one fresh process per run, "
                     f"{args.pairs} pairs, the parent's library first in each pair"}
    for alg, (env, _, _) in SHAPES.items():
        res = {"shape": f"{alg.upper()} {env}", "cases": {}}
        for (lib, a, case), slot in runs.items():
            if a != alg:
                continue
            v = slot["steps_per_s"]
            res["cases"][f"{lib}:{case}"] = {"runs_steps_per_s": v, "median": statistics.median(v), "min": min(v),
                                             "max": max(v), "levels_per_step": slot["levels"]}
        c = res["cases"]
        base = c.get("parent:ln_relu")
        if base:
            t = c["this:ln_relu"]
            res["ln_only_vs_parent"] = {"parent_range": [base["min"], base["max"]], "this_median": t["median"],
                                        "this_over_parent_median": round(t["median"] / base["median"], 4),
                                        "inside_parent_range": base["min"] <= t["median"] <= base["max"]}
        ref = base or c["this:ln_relu"]
        d = c["this:ln_relu_drop"]
        res["dropout_over_ln_only"] = {"baseline": "parent" if base else "this",
                                       "ratio": round(d["median"] / ref["median"], 4),
                                       "us_per_step_added": round(1e6 / d["median"] - 1e6 / ref["median"], 2),
                                       "levels_equal": d["levels_per_step"] == ref["levels_per_step"]}
        out[alg] = res
        print(json.dumps({k: v for k, v in res.items() if k != "cases"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
