#!/usr/bin/env python
"""What LayerNorm critics cost, and that the default programs kept their rate (DESIGN.md "LayerNorm critics"):
writes profiles/layer_norm_bench.json.

bench.py's synthetic workload -- TD3 on HalfCheetah-v4 and SAC on Humanoid-v4, hidden 256, batch 256, a 1M-row
replay, random weights -- on two libraries that alternate in one call: a build of the commit before LayerNorm
critics (--parent-lib) and this tree's.  Every run is a fresh child process with one engine in it (the library is
chosen when rl._engine loads; and engines that followed a closed one in the same process were seen to run some
bursts at a fraction of their rate, whatever their programs).  In every pair the parent's run of a shape comes
first, then this library's runs of it.  The parent's library runs the default programs; this one runs the default
programs, the ELU-critic programs, and the LayerNorm programs with ReLU and with ELU critics
(rle_set_layer_norm(1)).  Per case and library: every run's steps/s, the median, the min-max range, and the levels
per policy / plain step (rle_graph_stats).  The default cases of this library are then placed against the parent's
own run-to-run range, and each LayerNorm program against the program of the same activation without the norm.

usage: python tools/layer_norm_bench.py --parent-lib PATH [--pairs 3] [--steps 2000] [--warmup 200] [--out FILE]
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
SHAPES = {"td3": ("HalfCheetah-v4", 17, 6), "sac": ("Humanoid-v4", 376, 17)}
# (name, critic activation beyond the default, LayerNorm); the parent's library runs the first only
CASES = [("default", None, False), ("elu", "elu", False), ("ln_relu", None, True), ("ln_elu", "elu", True)]


def child(args):
    """One library, one case (--only alg:case): a JSON line on stdout."""
    from rl import _engine as E
    from rl.nn.layout import init_agent

    has_ln = hasattr(ctypes.CDLL(E.LIB_PATH), "rle_set_layer_norm")
    if not has_ln:  # (a library from before the entry points: bind what it has)
        for name in ("rle_set_layer_norm", "rle_get_layer_norm"):
            E.SIGNATURES.pop(name, None)
    algo_id = {"td3": E.RLE_TD3, "sac": E.RLE_SAC}
    only_alg, only_case = args.only.split(":")
    for alg, (env, s_dim, a_dim) in SHAPES.items():
        if alg != only_alg:
            continue
        nets = init_agent(alg, s_dim, a_dim, H, 123)
        for name, act, ln in CASES:
            if name != only_case:
                continue
            if ln and not has_ln:
                raise SystemExit("this library has no rle_set_layer_norm")
            acts = {"act_critic": act} if act else {}
            eng = E.Engine(E.make_config(algo_id[alg], s_dim, a_dim, H, B, use_lap=False, seed=111, **acts))
            if ln:
                eng.set_layer_norm(True)
            for net, params in nets.items():
                for pname, v in params.items():
                    eng.set_param(net, pname, v)
            rep = E.Replay(N_REPLAY, s_dim, a_dim, False, device=0)
            rep.fill_random(N_REPLAY, seed=0)
            eng.bind(rep)
            eng.step_timed(args.warmup)
            ms = eng.step_timed(args.steps)
            lp, lpl = eng.graph_stats()
            print(json.dumps({"alg": alg, "env": env, "case": name, "steps_per_s": round(args.steps / (ms * 1e-3), 1),
                              "levels": {"policy": lp, "plain": lpl}}), flush=True)
            eng.close()
            rep.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librle.so of the commit before LayerNorm critics")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "layer_norm_bench.json"))
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
                for case, _, _ in CASES:
                    if lib == "parent" and case != "default":
                        continue
                    env = dict(os.environ)
                    env.pop("RLE_LIB", None)
                    if path:
                        env["RLE_LIB"] = path
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--only", f"{alg}:{case}", "--steps",
                           str(args.steps), "--warmup", str(args.warmup)]
                    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=300)
                    if p.returncode != 0:  # (nothing more on the GPU after a failed child)
                        raise SystemExit(f"child ({lib} {alg}:{case}) exited with {p.returncode}")
                    for line in p.stdout.splitlines():
                        r = json.loads(line)
                        slot = runs.setdefault((lib, r["alg"], r["case"]), {"steps_per_s": [], "levels": r["levels"]})
                        slot["steps_per_s"].append(r["steps_per_s"])
                        print(pair, lib, line, flush=True)

    import torch

    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "?",
           "config": f"hidden {H} batch {B} {N_REPLAY} rows, rle_step_timed({args.steps}) after {args.warmup} warm-up "
                     f"steps, one fresh process per run, {args.pairs} pairs, the parent's library first in each pair"}
    for alg, (env, _, _) in SHAPES.items():
        res = {"shape": f"{alg.upper()} {env}", "cases": {}}
        for (lib, a, case), slot in runs.items():
            if a != alg:
                continue
            v = slot["steps_per_s"]
            res["cases"][f"{lib}:{case}"] = {"runs_steps_per_s": v, "median": statistics.median(v), "min": min(v),
                                             "max": max(v), "levels_per_step": slot["levels"]}
        c = res["cases"]
        if "parent:default" in c:
            p, t = c["parent:default"], c["this:default"]
            res["default_vs_parent"] = {"parent_range": [p["min"], p["max"]], "this_median": t["median"],
                                        "this_over_parent_median": round(t["median"] / p["median"], 4),
                                        "inside_parent_range": p["min"] <= t["median"] <= p["max"]}
        res["ln_over_same_activation"] = {
            "relu": round(c["this:ln_relu"]["median"] / c["this:default"]["median"], 4),
            "elu": round(c["this:ln_elu"]["median"] / c["this:elu"]["median"], 4)}
        out[alg] = res
        print(json.dumps({k: v for k, v in res.items() if k != "cases"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
