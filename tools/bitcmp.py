"""Bitwise comparison of two engine builds on a golden trajectory (GPU box, diagnostics).

    RLE_LIB=lib_a.so python tools/bitcmp.py dump NAME STEPS out_a.npz
    RLE_LIB=lib_b.so python tools/bitcmp.py dump NAME STEPS out_b.npz
    python tools/bitcmp.py cmp out_a.npz out_b.npz [out_a_again.npz]

NAME: a golden of tests/golden, edge:<case> for a case of tests/edge_cases.py (built under edge_env,
as tests/test_shape_edges_gpu.py builds it), or offline3:<shape> for an offline TD3 (TD3+BC) engine over a shape
of tests/test_offline_td3_gpu.py's SHAPES (its _env, offline_engine, ALPHA and tapes: OP_BC modes 2 and 3 and the
kDwGs weight gradients, which no golden or edge case builds), or awac:<case> for an offline SAC (AWAC) engine over a
case of tests/offline_sac_cases.py (test_offline_sac_gpu.offline_engine, the cases' own tapes: OP_AWAC).  Per step: every parameter, the priorities and the
info row after a single-step replay, and the engine's launch count (launches_<t>: how many rle_level dispatches
the programs replayed so far took).  The dump also holds the programs' descriptions (rle_graph_describe 0, 1, 3
and the hard-update program; empty where the engine has none) -- with RLE_DESC_WG=1 in the environment
they carry every op's workgroup count, so a changed tile plan shows even where the floats agree.  After the last
burst: act_sample on 1 and on 5 seeded observations, mode 0 and mode 2 with a seeded eps (act_<n>_<mode>), eval_q of
q1 on 5 seeded rows (TD7: the embeddings of fixed_encoder), and the packed state (state_export), so the act, eval and
state code is compared bit for bit as well.

Environment (dump): BITCMP_BURST steps per rle_step call (6: the multi-step and remainder programs);
BITCMP_NETS nets to dump; BITCMP_FUSE_OFF the plan's fuse_off, names of rl._engine.FUSE joined by "+" or
"all" (every fusion that is on by default); BITCMP_WIDE the plan's wide; BITCMP_CLIP a max_norm for
set_grad_clip; BITCMP_LN=1 for set_layer_norm (TD3 / SAC names only).  The last two apply before the first step.

cmp exits 1 when any array or description differs.  With a third dump (a second run of the first build),
arrays that differ between the first build's own two runs are reported and left out of the verdict.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "sac-td3-td7_amd"), os.path.join(REPO, "tests")]

OPT_IN = ("priosample",)  # include/rle.h RLE_FUSE_OPT_IN: off unless asked for, so not part of "all"
DESCRIBE = {"desc_policy": 0, "desc_plain": 1, "desc_multi": 3, "desc_hard": 2}
OFFLINE3_STEPS = 6  # steps of an offline3: trajectory (policy steps 1, 3, 5, as the offline TD3 tests run)
AWAC_STEPS = 12  # steps of an awac: trajectory (SAC's 8-step program, then its 4-step remainder at a burst of 12)


def plan_from_env():
    from rl import _engine as E

    off, wide = os.environ.get("BITCMP_FUSE_OFF"), os.environ.get("BITCMP_WIDE")
    if not off and not wide:
        return None
    names = [n for n in E.FUSE if n not in OPT_IN] if off == "all" else [n for n in (off or "").split("+") if n]
    return E.make_plan(fuse_off=names, **({"wide": int(wide)} if wide else {}))


def build(name, plan):
    """(golden, engine, replay, state dim, action dim) of a golden's name or of edge:<case>."""
    from harness import engine_from_golden
    from oracle import spec

    if name.startswith("offline3:"):
        import test_offline_td3_gpu as T

        shape = name[9:]
        g = {k: v for k, v in T.SHAPES[shape]().items() if not k.startswith("tape_")}
        with T._env(shape):
            S, A = spec.TASKS[str(g["meta_env"])][:2]
            eng, rep = T.offline_engine(g, T.ALPHA, plan)
        # (the tests' own tapes, for every shape as they run it: the synthetic shapes have none)
        g["meta"] = np.array(g["meta"])
        g["meta"][4] = OFFLINE3_STEPS
        tapes = T._tapes(OFFLINE3_STEPS, int(g["meta"][1]), A, int(g["meta"][6]))
        g.update({"tape_" + k: v for k, v in tapes.items()})
        return g, eng, rep, S, A
    if name.startswith("awac:"):
        import offline_sac_cases as C
        from test_offline_sac_gpu import offline_engine

        case = name[5:]
        c = C.CASES[case]
        eng, rep = offline_engine(case, plan=plan)
        g = {"meta_alg": "sac", "meta_env": C.ENV, "meta_extra_keys": np.array([], str), "meta_extra_vals": np.array([]),
             "meta": np.array([c.H, c.B, C.NCAP, C.NCAP, AWAC_STEPS, 0, c.seed]),
             "_shapes": {net: {k: np.shape(v) for k, v in p.items()} for net, p in C.nets(case).items()}}
        g.update({"tape_" + k: v for k, v in C.tapes(case, AWAC_STEPS).items()})
        return g, eng, rep, c.S, c.A
    if not name.startswith("edge:"):
        from conftest import load_golden

        g = load_golden(name)
        return (g,) + engine_from_golden(g, plan=plan)[:2] + spec.TASKS[str(g["meta_env"])][:2]
    import edge_cases

    c = edge_cases.CASES[name[5:]]
    g = edge_cases.golden(name[5:])
    with edge_cases.edge_env(name[5:]):
        if c.bc_lambda:
            from test_offline_gpu import offline_engine

            return (g,) + offline_engine(g, c.bc_lambda, plan) + (c.S, c.A)
        return (g,) + engine_from_golden(g, plan=plan)[:2] + (c.S, c.A)


def dump(name, steps, out):
    from harness import parse, shape_of
    from oracle import spec

    g, eng, rep, S, A = build(name, plan_from_env())
    alg, env, H, B, Ncap, n_fill, n_steps, use_lap, seed, extra = parse(g)
    steps = min(steps, n_steps)  # (the golden's tapes cover n_steps)
    tp = {k[5:]: v for k, v in g.items() if k.startswith("tape_")}
    shapes = g.pop("_shapes", None) or {net: {k: np.shape(v) for k, v in p.items()}
                                        for net, p in spec.agent_params(alg, S, A, H, seed, **shape_of(g)).items()}
    keep = os.environ.get("BITCMP_NETS")  # comma-separated nets to dump (default: all)
    if keep:
        shapes = {n: v for n, v in shapes.items() if n in keep.split(",")}
    if os.environ.get("BITCMP_CLIP"):
        eng.set_grad_clip(float(os.environ["BITCMP_CLIP"]))
    if os.environ.get("BITCMP_LN") == "1":
        eng.set_layer_norm(True)
    res = {k: np.array(eng.describe(which)) for k, which in DESCRIBE.items()}
    eng.set_tapes(u=tp["u"][:steps], eps=tp["eps"][:steps], eps_pi=tp.get("eps_pi"))
    burst = int(os.environ.get("BITCMP_BURST", "1"))  # steps per rle_step call (6: TD7's multi-step graphs)
    for t in range(0, steps, burst):
        res[f"info_{t}"] = np.asarray(eng.step(min(burst, steps - t)))
        res[f"launches_{t}"] = np.array(eng.launch_count(), np.int64)
        if use_lap:
            res[f"prio_{t}"] = rep.get_priority(Ncap)
        for net, ps in shapes.items():
            for p, shape in ps.items():
                res[f"{t}/{net}/{p}"] = np.asarray(eng.get_param(net, p)).reshape(shape)
    rng = np.random.default_rng(20240521)
    obs, act = rng.standard_normal((5, S)).astype(np.float32), rng.uniform(-1, 1, (5, A)).astype(np.float32)
    eps = rng.standard_normal((5, A)).astype(np.float32)
    for n in (1, 5):
        res[f"act_{n}_0"] = eng.act_sample(obs[:n], 0).copy()
        res[f"act_{n}_2"] = eng.act_sample(obs[:n], 2, eps[:n]).copy()
    res["eval_q1"] = eng.eval_q("q1", obs, act, enc="fixed_encoder")
    res["state_export"] = np.array(eng.state_export())
    np.savez(out, **res)


def differing(A, B, report):
    """Keys of A whose arrays are not bit-for-bit those of B (NaN payloads included: the info row's NaN
    on plain steps is equal to itself)."""
    bad = []
    for k in A.files:
        x, y = A[k], B[k]
        if x.dtype.kind == "U":  # a program description
            if str(x) != str(y):
                bad.append(k)
                report(f"{k:50s} differ (program description)")
            continue
        xb = x.view(np.uint32) if x.dtype == np.float32 else x
        yb = y.view(np.uint32) if y.dtype == np.float32 else y
        n = int((xb != yb).sum()) if x.shape == y.shape else x.size
        if n:
            bad.append(k)
            d = np.abs(x.astype(np.float64) - y.astype(np.float64)) if x.shape == y.shape else np.array([np.inf])
            report(f"{k:50s} differ {n:7d}/{x.size:7d} max {d.max():.3e}")
            if x.ndim == 2 and x.shape == y.shape:
                r, c = np.nonzero(xb != yb)
                report(f"    rows {sorted(set((r // 16).tolist()))} (16-blocks), cols {sorted(set((c // 16).tolist()))} (16-blocks)")
    return bad


def cmp(a, b, again=None):
    A, B = np.load(a), np.load(b)
    unstable = []
    if again:
        unstable = differing(A, np.load(again), lambda line: print("unstable (first build, run to run):", line))
    missing = sorted(set(A.files) ^ set(B.files))
    if missing:
        print("arrays in one dump only:", missing)
    bad = [k for k in differing(A, B, print) if k not in unstable] if not missing else missing
    print("compared", len(A.files), "arrays:", len(bad), "differ", f"({len(unstable)} unstable, left out)" if again else "")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        sys.exit(cmp(*sys.argv[2:5]))
