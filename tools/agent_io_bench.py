#!/usr/bin/env python
"""Agent save / restore measurements (DESIGN.md "Agent save / restore"): writes profiles/agent_io.json.

TD7 on Humanoid-v4 (hidden 256, batch 256, LAP) after a few gradient steps, so the Adam moments are not zero.
Each operation is the median of --runs calls (default 25) after 3 warm-ups, host wall time:

  dumps            pickle.dumps(agent)
  loads            pickle.loads(blob)              (a new engine and the import)
  deepcopy         copy.deepcopy(agent)
  load_state_dict  b.load_state_dict(a)
  rebuild          the batch-size change 256 -> 128 through train_n (no step; the way back is not timed)

and, as the floor of export and import, one pinned hipMemcpy of the payload's byte count in each direction
(beside it one single-threaded host copy of the same bytes, what a pass into or out of a staging array costs).
Only the agents' public interface is used, so the same file measures any commit: run it on the parent with
`--pkg <parent>/sac-td3-td7_amd --out parent.json`, then here with `--parent parent.json`.  Where the engine
has the one-pass export, its stages are timed too (pack + copy alone, the dict slicing, the import alone).

usage: python tools/agent_io_bench.py [--runs 25] [--pkg DIR] [--parent FILE] [--out FILE]
"""

from __future__ import annotations

import argparse
import copy
import json
import os
import pickle
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median_ms(fn, runs, warmup=3, before=None):
    ts = []
    for i in range(warmup + runs):
        if before is not None:
            before()
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            ts.append(dt)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "runs": runs}


def _payload_bytes(st):
    n = sum(v.nbytes for d in st["params"].values() for v in d.values())
    n += sum(m.nbytes + v.nbytes for d in st["adam"].values() for m, v in d.values())
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--pkg", default=os.path.join(REPO, "sac-td3-td7_amd"), help="the package to measure")
    ap.add_argument("--parent", default=None, help="JSON this tool wrote on the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "agent_io.json"))
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs: at least 20")
    sys.path.insert(0, os.path.abspath(args.pkg))

    import torch
    from rl.agent import TD7
    from rl.replay_memory import LAPReplayMemory

    def agent(seed, batch=256):
        return TD7("Humanoid-v4", use_lap=True, hidden=256, batch_size=batch, seed=seed)

    rep = LAPReplayMemory(65536, "Humanoid-v4")
    rep.dev.fill_random(65536, 1)
    a = agent(1)
    a.train_n(rep, 256, 8)
    b = agent(2)
    st = a.__getstate__()["_engine_state"]
    nbytes = _payload_bytes(st)
    res = {"device": torch.cuda.get_device_name(0), "agent": "TD7 Humanoid-v4 hidden 256 batch 256 LAP",
           "payload_bytes": nbytes, "tensors": sum(len(d) for d in st["params"].values())
           + 2 * sum(len(d) for d in st["adam"].values())}
    ops = res["ops"] = {}
    ops["dumps"] = _median_ms(lambda: pickle.dumps(a), args.runs)
    blob = pickle.dumps(a)
    res["pickle_bytes"] = len(blob)
    ops["loads"] = _median_ms(lambda: pickle.loads(blob), args.runs)
    ops["deepcopy"] = _median_ms(lambda: copy.deepcopy(a), args.runs)
    ops["load_state_dict"] = _median_ms(lambda: b.load_state_dict(a), args.runs)
    ops["rebuild"] = _median_ms(lambda: a.train_n(rep, 128, 0), args.runs, before=lambda: a.train_n(rep, 256, 0))
    a.train_n(rep, 256, 0)
    # what a new engine alone costs (part of loads, deepcopy and rebuild on any commit)
    ops["new_engine"] = _median_ms(lambda: a._new_engine(256).close(), args.runs)

    # the floor: one pinned copy of the payload's bytes, each direction
    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    pin = torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    def d2h():
        pin.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()

    def h2d():
        dev.copy_(pin, non_blocking=True)
        torch.cuda.synchronize()

    res["floor"] = {"pinned_d2h": _median_ms(d2h, args.runs), "pinned_h2d": _median_ms(h2d, args.runs)}
    del dev, pin
    # the host side alone: one single-threaded pass over the payload from one touched array into another
    # (what leaving or entering the pinned image costs on top of the device copy)
    src, dst = np.ones(nbytes // 4, np.float32), np.zeros(nbytes // 4, np.float32)
    res["host_copy"] = _median_ms(lambda: np.copyto(dst, src), args.runs)
    del src, dst

    # export / import and their stages, where the engine has the one-pass entries
    ops["export_dict"] = _median_ms(lambda: a._export(), args.runs)
    full = a._export()
    ops["import_dict"] = _median_ms(lambda: b._import(full), args.runs)
    eng = a.engine
    if hasattr(eng, "state_export"):
        from rl.agent.state_blob import blob_to_dict, dict_to_blob

        what = 7
        toc = eng.state_toc(what)
        packed = eng.state_export(what)
        stages = res["stages"] = {}
        stages["export_pack_and_copy"] = _median_ms(lambda: eng.state_export(what), args.runs)
        stages["export_slicing"] = _median_ms(lambda: blob_to_dict(toc, packed), args.runs)
        stages["import_assemble"] = _median_ms(lambda: dict_to_blob(toc, full), args.runs)
        stages["import_copy_and_unpack"] = _median_ms(lambda: b.engine.state_import(packed, what), args.runs)
        res["packed_bytes"] = int(packed.nbytes)
    res["export_over_floor"] = ops["export_dict"]["median_ms"] / res["floor"]["pinned_d2h"]["median_ms"]
    res["import_over_floor"] = ops["import_dict"]["median_ms"] / res["floor"]["pinned_h2d"]["median_ms"]

    # the round trip is exact
    c = pickle.loads(blob)
    sa, sc = a.state_dict(), c.state_dict()
    res["roundtrip_bit_identical"] = all(np.array_equal(sa[n][k], sc[n][k]) for n in sa for k in sa[n])

    if args.parent:
        par = json.load(open(args.parent))
        res["parent"] = {k: par[k] for k in ("ops", "floor", "export_over_floor", "import_over_floor") if k in par}
        res["speedup_over_parent"] = {k: par["ops"][k]["median_ms"] / v["median_ms"]
                                      for k, v in ops.items() if k in par["ops"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
