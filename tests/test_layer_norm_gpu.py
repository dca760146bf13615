"""LayerNorm critics in the device step (rle_set_layer_norm) against the CPU oracle with the ``ln_<act>``
composite of tests/layer_norm.py, through the C ABI and the Python mirror.

The seven cases run through the shape-edge sweep's own body (tests/test_shape_edges_gpu.py
check_trains_like_the_oracle) with its criteria unchanged: step-1 Adam first moments within max(1e-5, 4 d32) of
the float64 oracle, info rows rel 1e-3, end parameters within 2 lr n + 1e-4 with 0.99 of each tensor within 1e-5,
indices and priorities as there.  The compositions use their existing oracles' own checks.
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
import edge_cases as EC  # noqa: E402
import layer_norm as LN  # noqa: E402
import test_shape_edges_gpu as sweep  # noqa: E402
from harness import LOSS_RTOL  # noqa: E402
from oracle import agents, spec  # noqa: E402
from oracle import nets as N  # noqa: E402
from test_engine_gpu import assert_params_close  # noqa: E402


def ln_case_engine(case, plan=None, on=True):
    """(engine, replay) of an LN case; on=False: the same engine without the call (its plain activation)."""
    with LN.registered(case, engine=True):
        if on:
            return sweep._engine(case, plan)
        g = EC.reference(case)["g"]
        with EC.edge_env(case):
            from harness import engine_from_golden

            eng, rep, _ = engine_from_golden(LN.strip(g), plan=plan)
        return eng, rep


def depth(case):
    c = EC.CASES[LN.LN_CASES[case][0]]
    return len(c.hidden_sizes) if c.hidden_sizes else 2


# ---- the sweep ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(LN.LN_CASES))
def test_ln_case_trains_like_the_oracle(case):
    """Step 1 alone, then the rest as one burst, with the sweep's body and criteria."""
    with LN.registered(case, engine=True):
        sweep.check_trains_like_the_oracle(case)


def _engine_without_the_norm(case, plan=None, g=None):
    from harness import engine_from_golden

    with EC.edge_env(case):
        eng, rep, _ = engine_from_golden(LN.strip(EC.reference(case)["g"]), plan=plan)
    assert not eng.layer_norm()
    return eng, rep


def test_an_engine_without_the_setting_misses_the_ln_oracle(monkeypatch):
    """The same case with the norm left off: the sweep's criteria must fail (the oracle carries the norm)."""
    case = "ln-td3-k49"
    with LN.registered(case):
        monkeypatch.setattr(sweep, "_engine", _engine_without_the_norm)
        with pytest.raises(AssertionError):
            sweep.check_trains_like_the_oracle(case)


@pytest.mark.parametrize("case", ["ln-td3-k49", "ln-td3-deep6", "ln-sac-h260"])
def test_ln_programs_pass_audit_and_hazard_checks(case, monkeypatch):
    """RLE_AUDIT + RLE_HAZARD while every step program of the case is built (no step runs): the row ops' images
    and rstd vectors lie inside live allocations, and no level holds two ops touching one byte."""
    monkeypatch.setenv("RLE_AUDIT", "1")
    monkeypatch.setenv("RLE_HAZARD", "1")
    eng, rep = ln_case_engine(case)
    assert eng.describe(0) and eng.describe(1)


# ---- rle_graph_describe --------------------------------------------------------------------------------------

def _count(desc, name):
    return len(re.findall(r"(?:^|[ :])\*?%s(?= |$)" % re.escape(name), desc, re.M))


@pytest.mark.parametrize("case", ["ln-td3-k49", "ln-td3-deep6", "ln-sac-h260"])
def test_descriptions_name_the_row_ops(case):
    """A policy step holds the target, online and policy passes of two critics: 6 D forward and 4 D backward
    row ops for D hidden layers (a plain TD3 step: 4 D and 2 D); the heads run stand-alone, no q-dot partials,
    no layer recomputed in a critic's tile.  With the setting off the descriptions are those of an engine that
    was never asked."""
    D = depth(case)
    eng, rep = ln_case_engine(case)
    pol = eng.describe(0)
    assert (_count(pol, "ln"), _count(pol, "ln-bwd")) == (6 * D, 4 * D), pol
    if case.startswith("ln-td3"):
        pln = eng.describe(1)
        assert (_count(pln, "ln"), _count(pln, "ln-bwd")) == (4 * D, 2 * D), pln
    for text in (pol, eng.describe(1), eng.describe(3)):
        assert "head+dx" not in text and "qdot" not in text and "+pl" not in text and "sacpre" not in text, text
    assert _count(pol, "head") == 2  # (the loss head and the policy objective's head)
    never, _ = ln_case_engine(case, on=False)
    off, _ = ln_case_engine(case, on=False)
    off.set_layer_norm(False)
    assert not off.layer_norm() and not never.layer_norm()
    for w in (0, 1, 3):
        assert never.describe(w) == off.describe(w)
        assert _count(never.describe(w), "ln") == 0 and _count(never.describe(w), "ln-bwd") == 0


# ---- rle_eval ------------------------------------------------------------------------------------------------

_FWD = {}


def _fwd_reference(case):
    """oracle.nets.mlp_critic with the composite (float32) on the case's start weights and 1,024 seeded rows."""
    if case not in _FWD:
        src, critic, _, seed = LN.LN_CASES[case]
        c = EC.CASES[src]
        rng = np.random.default_rng(seed)
        s = rng.standard_normal((1024, c.S)).astype(np.float32)
        a = rng.uniform(-1, 1, (1024, c.A)).astype(np.float32)
        shape = {"hidden_sizes": c.hidden_sizes} if c.hidden_sizes else {}
        P = {net: {k: torch.from_numpy(v) for k, v in d.items()}
             for net, d in spec.agent_params(c.alg, c.S, c.A, c.H, seed, **shape).items()}
        torch.set_num_threads(1)
        with torch.no_grad():
            q = {net: N.mlp_critic(P[net], torch.from_numpy(s), torch.from_numpy(a), N.ACTS[critic])[:, 0].numpy()
                 for net in ("q1", "target_q2")}
            plain = N.mlp_critic(P["q1"], torch.from_numpy(s), torch.from_numpy(a))[:, 0].numpy()
        _FWD[case] = (s, a, q, plain)
    return _FWD[case]


@pytest.mark.parametrize("n", [1, 17, 1024])
@pytest.mark.parametrize("case", ["ln-td3-k49", "ln-sac-h260"])
def test_eval_q_at_row_count_edges(case, n):
    """rle_eval(RLE_EVAL_Q) of q1 and target_q2 on n rows against the oracle forward, within 1e-5 + 1e-5 |ref|
    (test_forward_entry_points_at_row_count_edges' tolerance)."""
    s, a, q, _ = _fwd_reference(case)
    eng, rep = ln_case_engine(case)
    for net, ref in q.items():
        sweep._close(eng.eval_q(net, s[:n], a[:n]), ref[:n], 1e-5, (case, net, n))


def test_setter_errors_and_rebuilds_forward_programs():
    """RLE_EINVAL on a TD7 engine and for a value other than 0 / 1; calling it after an rle_eval drops the captured
    forward program, so the next rle_eval computes with the norm; RLE_ESTATE after the first step."""
    case = "ln-td3-k49"
    s, a, q, plain = _fwd_reference(case)
    eng, rep = ln_case_engine(case, on=False)
    lib = E.lib()
    assert lib.rle_set_layer_norm(eng.h, 2) == -1 and b"0 (off) or 1 (on)" in lib.rle_last_error()
    sweep._close(eng.eval_q("q1", s[:17], a[:17]), plain[:17], 1e-5, "before")
    eng.set_layer_norm(True)
    assert eng.layer_norm()
    got = eng.eval_q("q1", s[:17], a[:17])
    sweep._close(got, q["q1"][:17], 1e-5, "after")
    assert np.abs(got - plain[:17]).max() > 1e-3
    eng.set_layer_norm(False)
    sweep._close(eng.eval_q("q1", s[:17], a[:17]), plain[:17], 1e-5, "off again")
    eng.set_layer_norm(True)
    eng.step(1)
    rc = lib.rle_set_layer_norm(eng.h, 0)
    assert rc not in (0, -1) and b"first step" in lib.rle_last_error(), rc  # RLE_ESTATE
    assert eng.layer_norm()
    td7, _ = sweep._engine("td7-b1")
    assert lib.rle_set_layer_norm(td7.h, 1) == -1 and b"TD3 / SAC only" in lib.rle_last_error()  # RLE_EINVAL
    assert lib.rle_set_layer_norm(td7.h, 0) == 0 and not td7.layer_norm()


# ---- bitwise -------------------------------------------------------------------------------------------------

def _same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("case,calls", [("ln-td3-k49", (16 + 4,)), ("ln-sac-a25", (8 + 4 + 2,))])
def test_burst_equals_single_steps_bitwise(case, calls):
    """One rle_step call -- the multi-step program (16 / 8 steps) and its remainder programs -- against the same
    steps run one at a time, and a second engine from the same seed against the first: parameters, moments and
    info rows bit for bit.  (The draws are the engine's own Philox streams.)"""
    total = sum(calls)
    out = []
    for cs in ((1,) * total, calls, calls):
        eng, rep = ln_case_engine(case)
        infos = []
        for k in cs:
            infos += [r.copy() for r in eng.step(k)]
        out.append({"info": np.asarray(infos, np.float32), "state": eng.state_export(E.STATE_ALL).copy(),
                    "ind": eng.last_indices().copy()})
        assert eng.plan()["steps_per_graph"] == (16 if case.startswith("ln-td3") else 8)
    _same(out[0], out[1], (case, "burst vs single"))
    _same(out[1], out[2], (case, "two engines"))
    assert np.isfinite(out[1]["info"][:, 0]).all()


# ---- compositions --------------------------------------------------------------------------------------------

def test_td3bc_with_layer_norm_matches_its_oracle(monkeypatch):
    """Offline TD3 (bc_alpha 2.5) on a LayerNorm critic at the odd shape of tests/test_offline_td3_gpu.py, against
    that file's oracle run and checks with the composite registered."""
    import test_offline_td3_gpu as T

    name, n = "ln_edge_odd", 5
    S, A, H, B, lap, seed = T.EDGES["edge_odd"]
    monkeypatch.setitem(T.EDGES, name, (S, A, H, B, lap, seed))

    def golden():
        g = T._synthetic(name, H, B, 256, 200, lap, seed)
        g["meta_acts"] = LN.meta_acts("ln_relu")
        return g

    monkeypatch.setitem(T.SHAPES, name, golden)
    ref = T._reference(name, T.ALPHA, n)
    with T._env(name):
        eng, rep = LN.ln_engine(ref["g"], build=lambda g, plan=None: T.offline_engine(g, T.ALPHA, plan))
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
    assert _count(desc, "ln") == 12 and _count(desc, "bc") == 2, desc


def test_awac_with_layer_norm_matches_its_oracle(monkeypatch):
    """Offline SAC (AWAC) on a LayerNorm critic at case b17 of tests/offline_sac_cases.py: the two forward-only
    passes of the policy phase carry the norm too."""
    import offline_sac_cases as C
    import offline_sac_oracle as O
    from test_offline_sac_gpu import _tape, offline_engine

    case, n = "b17", C.N_STEPS
    monkeypatch.setattr(O, "AWACOracle", functools.partial(O.AWACOracle, acts={"critic": "ln_relu"}))
    torch.set_num_threads(1)
    f32 = C._run(case, n, C.LMBDA)
    eng, rep = offline_engine(case)
    eng.set_layer_norm(True)
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
    # (target and online passes, then AWAC's two forward-only passes of each critic: 2 x 2 x (1 + 1 + 2) row ops)
    assert _count(desc, "awac") == 1 and _count(desc, "ln") == 16 and _count(desc, "ln-bwd") == 4, desc


def test_clipping_with_layer_norm_matches_the_clipped_oracle():
    """clip_grad_norm on ln-td3-k49 through tests/grad_clip_oracle.py.  The threshold is half the smallest total
    gradient norm of the critics in the unclipped oracle run, so the critics clip at every step -- asserted from the
    clipped oracle's log before the engine runs."""
    import grad_clip_cases as C
    import grad_clip_oracle as GO
    from test_oracle import build_from_golden

    case = "ln-td3-k49"
    with LN.registered(case, engine=True):
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
        assert "clip" in desc and "gsq" in desc and _count(desc, "ln") == 12


# ---- the goldens after an LN engine ran ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["td3_tiny", "sac_tiny"])
def test_goldens_still_match_after_an_ln_engine_ran(name):
    """The default programs and their kernel instance are untouched by an engine of the other instance in the same
    process: the reference goldens hold, step by step."""
    from test_engine_gpu import _trajectory

    eng, rep = ln_case_engine("ln-td3-min" if name == "td3_tiny" else "ln-sac-min")
    eng.step(2)
    _trajectory(name, burst=False)
    eng.step(1)
    _trajectory(name, burst=True)


# ---- the Python mirror ---------------------------------------------------------------------------------------

def _dataset(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 11)).astype(np.float32), rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32),
            (3 * rng.standard_normal(n)).astype(np.float32), rng.standard_normal((n, 11)).astype(np.float32),
            (rng.random(n) > 0.1).astype(np.float32))


def _replay(lap):
    from rl.replay_memory import LAPReplayMemory, SimpleReplayMemory

    rep = (LAPReplayMemory if lap else SimpleReplayMemory)(512, "Tiny-v0")
    rep.append_batch(*_dataset(300, 11))
    return rep


def test_mirror_keyword_survives_copies_and_trains_on_identically():
    """TD3("Tiny-v0", critic_layer_norm=True): the engine carries the norm; a pickle, a deepcopy and a batch-size
    rebuild (17 and back to 16) train on bit-identically to the original; the host q1 agrees with rle_eval."""
    from rl.agent import TD3
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    kw = dict(hidden=32, batch_size=16, seed=5)
    ag = TD3("Tiny-v0", critic_layer_norm=True, **kw)
    assert ag.critic_layer_norm is True and ag.engine.layer_norm()
    plain = TD3("Tiny-v0", **kw)
    assert not plain.engine.layer_norm() and "critic_layer_norm" not in plain.__dict__
    assert list(ag.state_dict()["q1"]) == list(plain.state_dict()["q1"])
    rep = _replay(False)
    ag.train_n(rep, 16, 4)
    plain.train_n(_replay(False), 16, 2)
    assert _count(ag.engine.describe(0), "ln") == 12 and _count(plain.engine.describe(0), "ln") == 0
    copies = [pickle.loads(pickle.dumps(ag)), copy.deepcopy(ag)]
    for other in copies:
        assert other.critic_layer_norm is True and other.engine.layer_norm()
    rebuilt = copy.deepcopy(ag)
    rebuilt._rebuild(17)
    rebuilt._rebuild(16)
    assert rebuilt.engine.layer_norm() and rebuilt.batch_size == 16
    # (each on a replay of its own with the same rows: the same Philox draws, the same batches)
    want = ag.train_n(_replay(False), 16, 3)
    state = ag.engine.state_export(E.STATE_ALL)
    for other in copies + [rebuilt]:
        got = other.train_n(_replay(False), 16, 3)
        assert got == want
        assert other.engine.state_export(E.STATE_ALL).tobytes() == state.tobytes()
    ag.to("cuda:0")
    assert ag.engine.layer_norm()
    # the host-side critic carries the norm and agrees with the device
    from rl.nn.modules import NormAct

    s, a = _dataset(33, 3)[:2]
    q1 = ag.q1
    assert isinstance(q1.mlp[1], NormAct) and q1.layer_norm
    with torch.no_grad():
        host = q1.estimate_q_value(torch.from_numpy(s), torch.from_numpy(a))[:, 0].numpy()
        host_plain = plain.q1.estimate_q_value(torch.from_numpy(s), torch.from_numpy(a))[:, 0].numpy()
    sweep._close(ag.engine.eval_q("q1", s, a), host, 1e-5, "host q1 vs rle_eval")
    sweep._close(plain.engine.eval_q("q1", s, a), host_plain, 1e-5, "plain host q1 vs rle_eval")
    # an agent pickled without the attribute has no norm
    old = pickle.loads(pickle.dumps(plain))
    assert old.critic_layer_norm is False and not old.engine.layer_norm()


def test_sac_mirror_keyword_reaches_the_engine():
    from rl.agent import SAC, TD7
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    kw = dict(hidden=32, batch_size=16, seed=5)
    ag = SAC("Tiny-v0", critic_layer_norm=True, clip_grad_norm=0.5, **kw)
    assert ag.engine.layer_norm() and ag.engine.grad_clip() == np.float32(0.5)
    rows = ag.train_n(_replay(False), 16, 3)
    assert all(np.isfinite(r["train/q_fn"]) for r in rows)
    assert _count(ag.engine.describe(0), "ln") == 12 and "clip" in ag.engine.describe(0)
    with pytest.raises(TypeError, match="critic_layer_norm"):
        TD7("Tiny-v0", critic_layer_norm=True, **kw)
