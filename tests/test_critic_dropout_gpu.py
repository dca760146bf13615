"""Critic dropout in the device step (rle_set_critic_dropout) against the CPU oracle with the ``dropln_<act>``
composite of tests/critic_dropout.py, whose masks are rebuilt on the host from the device's Philox stream.

The seven cases run through the shape-edge sweep's own body (tests/test_shape_edges_gpu.py
check_trains_like_the_oracle) with its criteria unchanged: step-1 Adam first moments within max(1e-5, 4 d32) of
the float64 oracle, info rows rel 1e-3, end parameters within 2 lr n + 1e-4 with 0.99 of each tensor within 1e-5,
indices and priorities as there.  The compositions use their existing oracles' own checks.  Every test calls an
entry that exists only with the feature.
"""

import copy
import functools
import pickle
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
import critic_dropout as CD  # noqa: E402
import edge_cases as EC  # noqa: E402
import layer_norm as LN  # noqa: E402
import test_shape_edges_gpu as sweep  # noqa: E402
from harness import ALGO, LOSS_RTOL, engine_from_golden  # noqa: E402
from oracle import agents  # noqa: E402
from test_engine_gpu import assert_params_close  # noqa: E402


def case_engine(case, p="case", plan=None):
    """(engine, replay) of a DROP case with LayerNorm on and dropout p ("case": the table's; None: never set)."""
    with CD.registered(case, engine=True, engine_p=p):
        return sweep._engine(case, plan)


def _count(desc, name):
    return len(re.findall(r"(?:^|[ :])\*?%s(?= |$)" % re.escape(name), desc, re.M))


def _ops(desc):
    """The kinds of the ops a description names, whatever their level (critical-chain marks and GEMM shapes dropped)."""
    body = " ".join(line.split(": ", 1)[1] for line in desc.splitlines() if ": " in line)
    return sorted(tok.lstrip("*") for tok in re.sub(r"\[[^\]]*\]", "", body).split())


def _levels(desc):
    return len(re.findall(r"(?m)^L\d+ ", desc))


# ---- 1. the mask stream --------------------------------------------------------------------------------------

HI_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15


@pytest.mark.parametrize("p", [0.01, 0.25, 0.5])
def test_dropout_mask_equals_the_host_law_bit_for_bit(p):
    """rle_dropout_mask -- the row ops' own mask function as a stand-alone kernel -- against critic_dropout.mask:
    one float4, widths that are no multiple of 16, the second Philox block of a row (width > 256), the widest
    layer at 1,024 rows; the first two sites and the largest; across the step counter's carry at 2^32; a seed with
    a non-zero high word."""
    eng = E.Engine(E.make_config(ALGO["td3"], 11, 3, 32, 32, seed=HI_SEED))
    eng.set_layer_norm(True)
    eng.set_critic_dropout(p)
    s = CD.scale(p)
    for rows, width in ((1, 4), (17, 20), (33, 260), (1024, 512)):
        for site in (0, 1, CD.MAX_SITE):
            for step in (0, 2**32 - 1, 2**32):
                got = eng.dropout_mask(step, site, rows, width)
                want = CD.mask(HI_SEED, p, step, site, rows, width)
                assert got.dtype == np.float32 and got.shape == (rows, width)
                assert got.tobytes() == want.tobytes(), (p, rows, width, site, step, float((got != want).mean()))
                assert set(np.unique(got)) <= {np.float32(0), s}
    big = eng.dropout_mask(5, 9, 1024, 512)
    q = float(np.float32(p))
    assert abs((big != 0).mean() - (1 - q)) <= 5 * np.sqrt(q * (1 - q) / big.size)
    other = E.Engine(E.make_config(ALGO["td3"], 11, 3, 32, 32, seed=HI_SEED ^ (1 << 32)))  # (another high word alone)
    other.set_layer_norm(True)
    other.set_critic_dropout(0.5)
    assert other.dropout_mask(0, 0, 33, 260).tobytes() == CD.mask(HI_SEED ^ (1 << 32), 0.5, 0, 0, 33, 260).tobytes()
    lib = E.lib()
    out = np.zeros(16, np.float32)
    for args in ((0, 64, 1, 4), (0, -1, 1, 4), (0, 0, 0, 4), (0, 0, 1, 6), (0, 0, 1, 516), (0, 0, (1 << 20) + 1, 4)):
        assert lib.rle_dropout_mask(eng.h, *args, out.ctypes.data_as(E._f32p)) == -1, args  # RLE_EINVAL


# ---- 2. the sweep --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CD.DROP_CASES))
def test_drop_case_trains_like_the_oracle(case):
    """Step 1 alone, then the rest as one burst, with the sweep's body and criteria: step-1 Adam first moments,
    info rows, end parameters, indices and priorities.  The draws u / eps come from the case's tapes; the masks
    come from the device's own stream and, for the oracle, from the host law."""
    with CD.registered(case, engine=True):
        worst = sweep.check_trains_like_the_oracle(case)
    print("DROP", case, worst)


# ---- 3. negative control -------------------------------------------------------------------------------------

def test_an_engine_without_dropout_misses_the_dropout_oracle():
    """drop-td3-k49 -- the case with the largest host margin (its float32 oracle's worst step-1 moment distance
    from float64, 3.4e-7, is the smallest of the seven) -- with the engine's p left at 0 (LayerNorm on): the sweep's
    criteria must fail against the dropout oracle."""
    case = "drop-td3-k49"
    with CD.registered(case, engine=True, engine_p=None):
        eng, _ = sweep._engine(case)
        assert eng.layer_norm() and eng.critic_dropout() == 0.0
        with pytest.raises(AssertionError):
            sweep.check_trains_like_the_oracle(case)


# ---- 4. program shape and the off state ----------------------------------------------------------------------

@pytest.mark.parametrize("case", ["drop-td3-k49", "drop-td3-deep6", "drop-sac-h260"])
def test_descriptions_levels_and_the_off_state(case):
    """A policy step names 6 D ``ln+drop`` and 4 D ``ln-bwd+drop`` (a plain TD3 step 4 D and 2 D) and no bare ``ln``
    / ``ln-bwd``; rle_graph_stats and every program's level count equal the LayerNorm-only engine's; with p = 0 the
    descriptions and the parameters after 4 steps equal the LayerNorm-only engine's bit for bit."""
    D = CD.depth(case)
    eng, _ = case_engine(case)
    ln, _ = case_engine(case, p=None)
    off, _ = case_engine(case, p=0.25)
    off.set_critic_dropout(0.0)
    assert eng.critic_dropout() > 0 and ln.critic_dropout() == 0.0 and off.critic_dropout() == 0.0
    pol = eng.describe(0)
    assert (_count(pol, "ln+drop"), _count(pol, "ln-bwd+drop")) == (6 * D, 4 * D), pol
    assert (_count(pol, "ln"), _count(pol, "ln-bwd")) == (0, 0), pol
    if case.startswith("drop-td3"):
        pln = eng.describe(1)
        assert (_count(pln, "ln+drop"), _count(pln, "ln-bwd+drop")) == (4 * D, 2 * D), pln
    assert (_count(ln.describe(0), "ln"), _count(ln.describe(0), "ln-bwd")) == (6 * D, 4 * D)
    assert eng.graph_stats() == ln.graph_stats() == off.graph_stats()
    for w in (0, 1, 3):
        assert _levels(eng.describe(w)) == _levels(ln.describe(w)) > 0, w
        assert _ops(eng.describe(w).replace("+drop", "")) == _ops(ln.describe(w)), w  # (the same ops, ...)
        if w != 3:  # (... in the single-step programs on the same levels; the multi-step program orders the row ops
            # of step t + 1 behind step t's counter bump, which moves off-chain ops between levels, not their count)
            assert eng.describe(w).replace("+drop", "") == ln.describe(w), w
        assert off.describe(w) == ln.describe(w), w
    a, b = off.step(4), ln.step(4)
    assert a.tobytes() == b.tobytes()
    assert off.state_export(E.STATE_ALL).tobytes() == ln.state_export(E.STATE_ALL).tobytes()
    eng.step(4)
    assert eng.state_export(E.STATE_ALL).tobytes() != ln.state_export(E.STATE_ALL).tobytes()


# ---- 5. bursts and repeatability -----------------------------------------------------------------------------

def _same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("case,calls", [("drop-td3-k49", (16 + 4,)), ("drop-sac-a25", (8 + 4 + 2,))])
def test_burst_equals_single_steps_bitwise(case, calls):
    """One rle_step call -- the multi-step program (16 / 8 steps) and its remainder programs, the step word read on
    the device -- against the same steps run one at a time, and a second engine from the same seed against the
    first: parameters, moments and info rows bit for bit.  (Every draw is the engine's own Philox stream.)"""
    total = sum(calls)
    out = []
    for cs in ((1,) * total, calls, calls):
        eng, rep = case_engine(case)
        infos = []
        for k in cs:
            infos += [r.copy() for r in eng.step(k)]
        out.append({"info": np.asarray(infos, np.float32), "state": eng.state_export(E.STATE_ALL).copy(),
                    "ind": eng.last_indices().copy()})
        assert eng.plan()["steps_per_graph"] == (16 if case.startswith("drop-td3") else 8)
        assert eng.counters()[4] == total
    _same(out[0], out[1], (case, "burst vs single"))
    _same(out[1], out[2], (case, "two engines"))
    assert np.isfinite(out[1]["info"][:, 0]).all()


def test_engine_fed_by_copy_state_from_another_p_steps_like_its_own_oracle():
    """drop-sac-a25 (uniform replay): an engine with p = 0.5 runs the first 2 steps, an engine with the case's
    p = 0.25 takes its state by rle_copy_state (parameters, moments, the step counter; p is not part of the state)
    and runs the other 2; the oracle does the same with its composite's p switched after step 2.  End parameters
    and the last info rows at the sweep's tolerances."""
    from test_oracle import build_from_golden

    case, k, p_a = "drop-sac-a25", 2, 0.5
    with CD.registered(case, engine=True) as comp:
        c = EC.CASES[case]
        g = EC.golden(case)
        with EC.edge_env(case):
            _, orc, orep, tp, n, B = build_from_golden(g)
        torch.set_num_threads(1)
        p_b, comp.p = comp.p, p_a
        info = []
        for t in range(n):
            if t == k:
                comp.p = p_b
            i1, _ = agents.run_steps(orc, c.alg, orep, {key: v[t:t + 1] for key, v in tp.items()}, 1, B)
            info += i1
        comp.p = p_b
        keys = EC.info_keys(case)
        table = np.array([[np.nan if i[q] is None else i[q] for q in keys] for i in info], np.float64)
        with EC.edge_env(case):
            first, _ = CD.drop_engine(g, p_a)
            second, _ = CD.drop_engine(g, p_b)
        first.set_tapes(u=tp["u"][:k], eps=tp["eps"][:k], eps_pi=tp["eps_pi"][:k])
        first.step(k)
        first.set_tapes()
        second.copy_state_from(first)
        assert second.critic_dropout() == 0.25 and first.critic_dropout() == 0.5 and second.counters()[4] == k
        second.set_tapes(u=tp["u"][k:], eps=tp["eps"][k:], eps_pi=tp["eps_pi"][k:])
        rows = np.asarray(second.step(n - k), np.float64)[:, :len(keys)]
        second.set_tapes()
        np.testing.assert_allclose(rows, table[k:], rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
        tol = 2 * 3e-4 * n + 1e-4
        for net, d in orc.nets().items():
            for name, v in d.items():
                v = v.detach().numpy()
                assert_params_close(second.get_param(net, name, v.shape), v, tol, (net, name), bulk=0.99)


# ---- 6. diagnostics ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["drop-td3-k49", "drop-td3-deep6", "drop-sac-h260"])
def test_drop_programs_pass_audit_and_hazard_checks(case, monkeypatch):
    """RLE_AUDIT + RLE_HAZARD while every step program of the case is built (no step runs): the row ops' images,
    rstd vectors and the step counter they now read lie inside live allocations, and no level holds an op that
    reads the counter beside the step end that bumps it."""
    monkeypatch.setenv("RLE_AUDIT", "1")
    monkeypatch.setenv("RLE_HAZARD", "1")
    eng, rep = case_engine(case)
    assert eng.describe(0) and eng.describe(1)
    assert _count(eng.describe(0), "ln+drop") == 6 * CD.depth(case)


# ---- 7. compositions -----------------------------------------------------------------------------------------

def test_td3bc_with_dropout_matches_its_oracle(monkeypatch):
    """Offline TD3 (bc_alpha 2.5) on a DroQ critic at the odd shape of tests/test_offline_td3_gpu.py, against that
    file's oracle run and checks with the composite registered."""
    import test_offline_td3_gpu as T

    name, n, p = "drop_edge_odd", 5, 0.25
    S, A, H, B, lap, seed = T.EDGES["edge_odd"]
    monkeypatch.setitem(T.EDGES, name, (S, A, H, B, lap, seed))

    def golden():
        g = T._synthetic(name, H, B, 256, 200, lap, seed)
        g["meta_acts"] = LN.meta_acts(CD.PREFIX + "relu")
        return g

    monkeypatch.setitem(T.SHAPES, name, golden)
    with CD.composite("relu", seed, p, 2):
        ref = T._reference(name, T.ALPHA, n)
    with T._env(name):
        eng, rep = CD.drop_engine(ref["g"], p, build=lambda g, plan=None: T.offline_engine(g, T.ALPHA, plan))
    eng.set_tapes(u=ref["tp"]["u"], eps=ref["tp"]["eps"])
    infos = []
    for t in range(n):
        infos.append(eng.step(1)[0])
        T._check_state(eng, rep, ref, t)
        if t == ref["m_step"]:
            T._check_moments(eng, ref)
    eng.set_tapes()
    T._check_end(eng, ref, infos, n)
    desc = eng.describe(0)
    assert _count(desc, "ln+drop") == 12 and _count(desc, "bc") == 2, desc


def test_awac_with_dropout_matches_its_oracle(monkeypatch):
    """Offline SAC (AWAC) on a DroQ critic at case b17 of tests/offline_sac_cases.py: the two forward-only passes of
    the policy phase drop too -- Q(s, a) at pass 3, which exists only here, and Q(s, a_pi) at pass 2."""
    import offline_sac_cases as C
    import offline_sac_oracle as O
    from test_offline_sac_gpu import _tape, offline_engine

    case, n, p = "b17", C.N_STEPS, 0.25
    c = C.CASES[case]
    L = len(c.hidden_sizes) if c.hidden_sizes else 2
    with CD.composite("relu", c.seed, p, L, awac=True) as comp:
        monkeypatch.setattr(O, "AWACOracle", functools.partial(O.AWACOracle, acts={"critic": CD.PREFIX + "relu"}))
        torch.set_num_threads(1)
        f32 = C._run(case, n, C.LMBDA)
        sites = {site for _, site in comp.seen}
    assert sites == {CD.site_of(ps, tw, l) for ps in range(4) for tw in range(2) for l in range(L)}
    eng, rep = offline_engine(case)
    eng.set_layer_norm(True)
    eng.set_critic_dropout(p)
    _tape(eng, C.tapes(case, n))
    infos = [eng.step(1)[0]]
    np.testing.assert_array_equal(eng.last_indices(), f32["ind"][0])

    def adam(key):
        net, pname = key[:-2].split(".", 1)
        return eng.get_adam(net, pname, 0 if key.endswith(":m") else 1)

    bad = C.moment_shortfalls(adam, f32["m"])
    infos += list(eng.step(n - 1))
    np.testing.assert_array_equal(eng.last_indices(), f32["ind"][n - 1])
    eng.set_tapes()
    bad += C.end_shortfalls(np.asarray(infos, np.float64)[:, :5], eng.get_param, f32, n)
    assert not bad, bad
    desc = eng.describe(0)
    assert _count(desc, "awac") == 1 and _count(desc, "ln+drop") == 8 * L and _count(desc, "ln-bwd+drop") == 2 * L, desc


def test_clipping_with_dropout_matches_the_clipped_oracle():
    """clip_grad_norm on drop-td3-k49 through tests/grad_clip_oracle.py.  The threshold is half the smallest total
    gradient norm of the critics in the unclipped oracle run, so the critics clip at every step -- asserted from the
    clipped oracle's log before the engine runs."""
    import grad_clip_cases as C
    import grad_clip_oracle as GO
    from test_oracle import build_from_golden

    case = "drop-td3-k49"
    with CD.registered(case, engine=True):
        c = EC.CASES[case]
        g = EC.reference(case)["g"]

        def run(max_norm):
            with EC.edge_env(case):
                _, orc, rep, tp, n, B = build_from_golden(g)
            log = GO.clip(orc, max_norm)
            out = {"info": [], "ind": [], "m": None}
            for t in range(n):
                i1, n1 = agents.run_steps(orc, c.alg, rep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
                out["info"] += i1
                out["ind"] += n1
                if t == 0:
                    out["m"] = dict(agents.moments(orc))
            out["log"] = list(log)
            out["params"] = {(net, k): v.detach().numpy().copy() for net, d in orc.nets().items() for k, v in d.items()}
            keys = EC.info_keys(case)
            out["table"] = np.array([[np.nan if i[k] is None else i[k] for k in keys] for i in out["info"]], np.float64)
            return out, tp, n

        torch.set_num_threads(1)
        plain, tp, n = run(float("inf"))
        totals = [t for name, t, _ in plain["log"] if name == "critics"]
        assert len(totals) == n
        max_norm = 0.5 * min(totals)
        ref, _, _ = run(max_norm)
        coefs = [c_ for name, _, c_ in ref["log"] if name == "critics"]
        assert len(coefs) == n and all(c_ < 1.0 for c_ in coefs), coefs
        eng, rep = sweep._engine(case)
        eng.set_grad_clip(max_norm)
        eng.set_tapes(u=tp["u"], eps=tp["eps"], eps_pi=tp.get("eps_pi"))
        infos = [eng.step(1)[0].copy()]
        np.testing.assert_array_equal(eng.last_indices(), ref["ind"][0])

        def adam(key):
            name, which = key.rsplit(":", 1)
            net, pname = name.split(".", 1)
            return eng.get_adam(net, pname, 0 if which == "m" else 1, ref["m"][key].shape)

        assert C.moment_shortfalls(adam, ref["m"]) == []
        st = eng.grad_clip_stats()["critics"]
        first = next(e for e in ref["log"] if e[0] == "critics")
        np.testing.assert_allclose(st, first[1:], rtol=LOSS_RTOL, atol=1e-4)
        infos += [r.copy() for r in eng.step(n - 1)]
        eng.set_tapes()
        np.testing.assert_array_equal(eng.last_indices(), ref["ind"][n - 1])
        k = ref["table"].shape[1]
        np.testing.assert_allclose(np.asarray(infos, np.float64)[:, :k], ref["table"], rtol=LOSS_RTOL, atol=1e-4,
                                   equal_nan=True)
        tol = 2 * 3e-4 * n + 1e-4
        for (net, pname), v in ref["params"].items():
            assert_params_close(eng.get_param(net, pname, v.shape), v, tol, (net, pname), bulk=0.99)
        desc = eng.describe(0)
        assert "clip" in desc and "gsq" in desc and _count(desc, "ln+drop") == 12


# ---- 8. rle_eval ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["drop-td3-k49", "drop-sac-h260"])
def test_eval_q_runs_without_dropout(case):
    """rle_eval(RLE_EVAL_Q) is inference: q1 and target_q2 at 1, 17 and 1,024 rows equal a LayerNorm-only engine's
    with the same parameters bit for bit, before and after gradient steps (the LayerNorm-only engine then takes
    the trained parameters by rle_copy_state)."""
    c = EC.CASES[CD.DROP_CASES[case][0]]
    rng = np.random.default_rng(CD.DROP_CASES[case][3])
    s = rng.standard_normal((1024, c.S)).astype(np.float32)
    a = rng.uniform(-1, 1, (1024, c.A)).astype(np.float32)
    eng, _ = case_engine(case)
    ln, _ = case_engine(case, p=None)
    for trained in (False, True):
        if trained:
            eng.step(3)
            ln.copy_state_from(eng)
        for net in ("q1", "target_q2"):
            for n in (1, 17, 1024):
                got, want = eng.eval_q(net, s[:n], a[:n]), ln.eval_q(net, s[:n], a[:n])
                assert got.tobytes() == want.tobytes() and np.isfinite(got).all(), (case, net, n, trained)
    assert eng.critic_dropout() > 0 and ln.critic_dropout() == 0.0


# ---- 9. setter errors, isolation, the mirror -----------------------------------------------------------------

def test_setter_errors():
    """Every refusal rle.h lists: p outside [0, 1) or NaN, LayerNorm off at the call, LayerNorm switched off while
    p > 0, TD7, and RLE_ESTATE after the first step."""
    lib = E.lib()
    eng, _ = case_engine("drop-td3-k49", p=None)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert lib.rle_set_critic_dropout(eng.h, bad) == -1 and b"[0, 1)" in lib.rle_last_error(), bad
    eng.set_layer_norm(False)
    assert lib.rle_set_critic_dropout(eng.h, 0.25) == -1
    assert b"dropout without LayerNorm is not run" in lib.rle_last_error()
    assert lib.rle_set_critic_dropout(eng.h, 0.0) == 0  # (off: nothing to refuse)
    eng.set_layer_norm(True)
    eng.set_critic_dropout(0.25)
    assert eng.critic_dropout() == 0.25
    assert lib.rle_set_layer_norm(eng.h, 0) == -1 and b"dropout without LayerNorm is not run" in lib.rle_last_error()
    assert eng.layer_norm()
    eng.set_critic_dropout(0.0)
    eng.set_layer_norm(False)
    eng.set_layer_norm(True)
    eng.set_critic_dropout(0.5)
    eng.step(1)
    rc = lib.rle_set_critic_dropout(eng.h, 0.25)
    assert rc not in (0, -1) and b"first step" in lib.rle_last_error(), rc  # RLE_ESTATE
    assert eng.critic_dropout() == 0.5
    td7, _ = sweep._engine("td7-b1")
    assert lib.rle_set_critic_dropout(td7.h, 0.25) == -1 and b"TD3 / SAC only" in lib.rle_last_error()
    assert lib.rle_set_critic_dropout(td7.h, 0.0) == 0 and td7.critic_dropout() == 0.0


@pytest.mark.parametrize("name", ["td3_tiny", "sac_tiny"])
def test_goldens_still_match_after_a_dropout_engine_ran(name):
    """The default programs and their kernel instance are untouched by a dropout engine in the same process."""
    from test_engine_gpu import _trajectory

    eng, rep = case_engine("drop-td3-min" if name == "td3_tiny" else "drop-sac-min")
    eng.step(2)
    _trajectory(name, burst=False)
    eng.step(1)
    _trajectory(name, burst=True)
    assert eng.critic_dropout() == 0.5


def _dataset(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 11)).astype(np.float32), rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32),
            (3 * rng.standard_normal(n)).astype(np.float32), rng.standard_normal((n, 11)).astype(np.float32),
            (rng.random(n) > 0.1).astype(np.float32))


def _replay():
    from rl.replay_memory import SimpleReplayMemory

    rep = SimpleReplayMemory(512, "Tiny-v0")
    rep.append_batch(*_dataset(300, 11))
    return rep


def test_mirror_keyword_survives_copies_and_trains_on_identically():
    """TD3("Tiny-v0", critic_layer_norm=True, critic_dropout=0.25): the engine carries p; a pickle, a deepcopy and a
    batch-size rebuild (17 and back to 16) train on bit-identically to the original; to() keeps it; the host q1
    carries the dropout and, in eval(), agrees with rle_eval; SAC takes the keyword, TD7 refuses it."""
    from rl.agent import SAC, TD3, TD7
    from rl.nn.modules import NormAct
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    kw = dict(hidden=32, batch_size=16, seed=5)
    ag = TD3("Tiny-v0", critic_layer_norm=True, critic_dropout=0.25, **kw)
    assert ag.critic_dropout == 0.25 and ag.engine.critic_dropout() == 0.25 and ag.engine.layer_norm()
    ln = TD3("Tiny-v0", critic_layer_norm=True, **kw)
    assert ln.engine.critic_dropout() == 0.0 and "critic_dropout" not in ln.__dict__
    assert list(ag.state_dict()["q1"]) == list(ln.state_dict()["q1"])
    ag.train_n(_replay(), 16, 4)
    ln.train_n(_replay(), 16, 4)
    assert _count(ag.engine.describe(0), "ln+drop") == 12 and _count(ln.engine.describe(0), "ln+drop") == 0
    assert ag.engine.state_export(E.STATE_ALL).tobytes() != ln.engine.state_export(E.STATE_ALL).tobytes()
    copies = [pickle.loads(pickle.dumps(ag)), copy.deepcopy(ag)]
    rebuilt = copy.deepcopy(ag)
    rebuilt._rebuild(17)
    rebuilt._rebuild(16)
    for other in copies + [rebuilt]:
        assert other.critic_dropout == 0.25 and other.engine.critic_dropout() == 0.25
    want = ag.train_n(_replay(), 16, 3)
    state = ag.engine.state_export(E.STATE_ALL)
    for other in copies + [rebuilt]:
        got = other.train_n(_replay(), 16, 3)
        assert got == want
        assert other.engine.state_export(E.STATE_ALL).tobytes() == state.tobytes()
    ag.to("cuda:0")
    assert ag.engine.critic_dropout() == 0.25
    s, a = _dataset(33, 3)[:2]
    q1 = ag.q1
    assert isinstance(q1.mlp[1], NormAct) and q1.layer_norm and q1.dropout == 0.25 and q1.mlp[1].p == 0.25
    with torch.no_grad():
        host = q1.eval().estimate_q_value(torch.from_numpy(s), torch.from_numpy(a))[:, 0].numpy()
    sweep._close(ag.engine.eval_q("q1", s, a), host, 1e-5, "host q1.eval() vs rle_eval")
    sac = SAC("Tiny-v0", critic_layer_norm=True, critic_dropout=0.01, clip_grad_norm=0.5, **kw)
    assert sac.engine.critic_dropout() == float(np.float32(0.01)) and sac.engine.layer_norm()
    rows = sac.train_n(_replay(), 16, 3)
    assert all(np.isfinite(r["train/q_fn"]) for r in rows)
    assert _count(sac.engine.describe(0), "ln+drop") == 12 and "clip" in sac.engine.describe(0)
    with pytest.raises(TypeError, match="critic_dropout"):
        TD7("Tiny-v0", critic_dropout=0.25, **kw)
