#!/usr/bin/env python
"""What n-step returns cost, and that the one-step programs kept their rate (DESIGN.md "n-step returns"): writes
profiles/n_step_bench.json.

tools/critic_dropout_bench.py's method: TD3 on HalfCheetah-v4 and SAC on Humanoid-v4, hidden 256, batch 256, random
weights, on two libraries that alternate in one call, every run a fresh child process with one engine in it.  The
parent commit's library (--parent-lib) runs the one-step programs; this tree's runs the same (n_step = 1) and
n_step = 3 and 8.  In every pair the parent's run of a shape comes first.  The replay is filled with EPISODIC rows
(state[i + 1] = next_state[i] inside an episode): rle_replay_fill_random's rows never chain, every walk would stop
after one hop and the multi-hop gather would measure nothing.  Episode lengths are uniform in 1 .. EP_MAX, every
second episode ends terminated (notdone 0), the others truncated (a fresh state, notdone 1); the ring is full with
its write pointer at slot 0.  Per case and library: every run's steps/s, the median, the min-max range, the levels
per policy / plain step (rle_graph_stats) and the mean of replay/hops over 64 further steps.  This library's
n_step = 1 median is then placed against the parent's own min-max range, and n_step = 3 / 8 against this library's
n_step = 1.

usage: python tools/n_step_bench.py --parent-lib PATH [--pairs 4] [--steps 4000] [--warmup 200] [--out FILE]
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

N_REPLAY = 131072
EP_MAX = 64
CHUNK = 16384
H, B = 256, 256
SHAPES = {"td3": ("HalfCheetah-v4", 17, 6, 3), "sac": ("Humanoid-v4", 376, 17, 6)}  # (.., the hops info column)
NEW = ("rle_set_n_step", "rle_get_n_step", "rle_replay_gather_nstep")
CASES = [("n1", 1), ("n3", 3), ("n8", 8)]  # the parent's library runs the first only


def fill_episodic(rep, s_dim, a_dim, seed=0):
    """N_REPLAY rows of episodes laid end to end, appended in chunks (the ring ends full, ptr 0)."""
    import numpy as np

    rng = np.random.Generator(np.random.PCG64(seed))
    starts = np.zeros(N_REPLAY, bool)
    notdone = np.ones(N_REPLAY, np.float32)
    i = k = 0
    while i < N_REPLAY:
        starts[i] = True
        last = min(i + int(rng.integers(1, EP_MAX + 1)), N_REPLAY) - 1
        if k % 2 == 0:
            notdone[last] = 0.0
        i, k = last + 1, k + 1
    carry = None
    for row0 in range(0, N_REPLAY, CHUNK):
        n = min(CHUNK, N_REPLAY - row0)
        nxt = rng.standard_normal((n, s_dim), dtype=np.float32)
        st = np.empty_like(nxt)
        st[1:] = nxt[:-1]
        st[0] = carry if carry is not None else 0.0
        first = np.flatnonzero(starts[row0:row0 + n])
        st[first] = rng.standard_normal((first.size, s_dim), dtype=np.float32)  # (an episode's first row: a fresh state)
        carry = nxt[-1]
        rep.append(st, rng.uniform(-1, 1, (n, a_dim)).astype(np.float32), rng.standard_normal(n, dtype=np.float32),
                   nxt, notdone[row0:row0 + n])


def child(args):
    """One library, one case (--only alg:case): a JSON line on stdout."""
    import numpy as np

    from rl import _engine as E
    from rl.nn.layout import init_agent

    has_n = hasattr(ctypes.CDLL(E.LIB_PATH), NEW[0])
    if not has_n:  # (a library from before the entry points: bind what it has)
        for name in NEW:
            E.SIGNATURES.pop(name, None)
    algo_id = {"td3": E.RLE_TD3, "sac": E.RLE_SAC}
    alg, case = args.only.split(":")
    env, s_dim, a_dim, hops_col = SHAPES[alg]
    n_step = dict(CASES)[case]
    if n_step > 1 and not has_n:
        raise SystemExit("this library has no rle_set_n_step")
    eng = E.Engine(E.make_config(algo_id[alg], s_dim, a_dim, H, B, use_lap=False, seed=111))
    if n_step > 1:
        eng.set_n_step(n_step)
    for net, params in init_agent(alg, s_dim, a_dim, H, 123).items():
        for pname, v in params.items():
            eng.set_param(net, pname, v)
    rep = E.Replay(N_REPLAY, s_dim, a_dim, False, device=0)
    fill_episodic(rep, s_dim, a_dim)
    assert rep.state()[:2] == (0, N_REPLAY)
    eng.bind(rep)
    eng.step_timed(args.warmup)
    ms = eng.step_timed(args.steps)
    lp, lpl = eng.graph_stats()
    hops = float(np.mean(eng.step(64)[:, hops_col])) if n_step > 1 else 1.0
    print(json.dumps({"alg": alg, "env": env, "case": case, "steps_per_s": round(args.steps / (ms * 1e-3), 1),
                      "levels": {"policy": lp, "plain": lpl}, "hops": round(hops, 4)}), flush=True)
    eng.close()
    rep.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librle.so of the commit before n-step returns (required)")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "n_step_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        ap.error("--parent-lib: the parent commit's librle.so (the one-step programs are placed against its range)")

    libs = [("parent", os.path.abspath(args.parent_lib)), ("this", None)]
    runs = {}  # (library, alg, case) -> {"steps_per_s": [...], "levels": ..., "hops": [...]}
    for pair in range(args.pairs):
        for alg in SHAPES:
            for lib, path in libs:
                for case, n_step in CASES:
                    if lib == "parent" and n_step > 1:
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
                        slot = runs.setdefault((lib, d["alg"], d["case"]),
                                               {"steps_per_s": [], "levels": d["levels"], "hops": []})
                        slot["steps_per_s"].append(d["steps_per_s"])
                        slot["hops"].append(d["hops"])
                        print(pair, lib, line, flush=True)

    import torch

    out = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "?",
           "config": f"hidden {H} batch {B}, rle_step_timed({args.steps}) after {args.warmup} warm-up steps, one fresh "
                     f"process per run, {args.pairs} pairs, the parent's library first in each pair",
           "replay": {"rows": N_REPLAY, "full": True, "ptr": 0,
                      "episode_lengths": f"uniform in 1 .. {EP_MAX}, laid end to end",
                      "episode_ends": "alternately terminated (notdone 0) and truncated (fresh state, notdone 1)"}}
    for alg, (env, *_rest) in SHAPES.items():
        res = {"shape": f"{alg.upper()} {env}", "cases": {}}
        for (lib, a, case), slot in runs.items():
            if a != alg:
                continue
            v = slot["steps_per_s"]
            res["cases"][f"{lib}:{case}"] = {"runs_steps_per_s": v, "median": statistics.median(v), "min": min(v),
                                             "max": max(v), "levels_per_step": slot["levels"],
                                             "replay_hops": statistics.median(slot["hops"])}
        c = res["cases"]
        base = c.get("parent:n1")
        t = c["this:n1"]
        if base:
            res["n1_vs_parent"] = {"parent_range": [base["min"], base["max"]], "this_median": t["median"],
                                   "this_over_parent_median": round(t["median"] / base["median"], 4),
                                   "inside_parent_range": base["min"] <= t["median"] <= base["max"]}
        for case in ("n3", "n8"):
            d = c[f"this:{case}"]
            res[f"{case}_over_n1"] = {"ratio": round(d["median"] / t["median"], 4), "range": [d["min"], d["max"]],
                                      "us_per_step_added": round(1e6 / d["median"] - 1e6 / t["median"], 2),
                                      "replay_hops": d["replay_hops"],
                                      "levels_equal": d["levels_per_step"] == t["levels_per_step"]}
        out[alg] = res
        print(json.dumps({k: v for k, v in res.items() if k != "cases"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
