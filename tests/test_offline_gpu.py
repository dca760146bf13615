"""TD7 offline mode on the GPU: the engine's policy step with the behaviour-cloning term (rle_config
bc_lambda) against tests/offline_oracle.py's TD7BCOracle, step by step on seeded tapes.

Tolerances are those tests/test_engine_gpu.py holds the same quantities to against the oracle: info columns
rel 1e-3 (harness.LOSS_RTOL, atol 1e-4); priorities rtol 1e-4 / atol 1e-5; value bounds 1e-4; indices exact;
parameters after k steps every element within 2 lr k + 1e-4 and the bulk (99% of an H = 32 tensor, 99.9% at
full width) within 1e-5.  The Adam first moments after the first policy step are held to
tests/test_parity_gpu.py's criterion for the moments of steps 1 and 2, |d| <= 1e-4 |m| + 1e-4 max|m|
(test_engine_gpu.py's 1e-5 max|m| is for step 1 alone, and the first policy step is step 2 or 3).
Every test here passes bc_lambda or offline and so fails on an engine without the field.
"""

import copy
import pickle

import numpy as np
import pytest
import torch

from conftest import acts_of, load_golden, shape_of

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
from harness import LOSS_RTOL, fill_replay, parse  # noqa: E402
from offline_oracle import INFO_KEYS, build_offline  # noqa: E402
from oracle import agents, spec  # noqa: E402

LMBDAS = [0.1, 5.0]


def _synthetic(env, H, B, ncap, n_fill, use_lap, seed, **extra):
    return {"meta_alg": np.array("td7"), "meta_env": np.array(env),
            "meta": np.array([H, B, ncap, n_fill, 0, int(use_lap), seed]),
            "meta_extra_keys": np.array(list(extra), dtype="<U32"),
            "meta_extra_vals": np.array(list(extra.values()), np.float64)}


# the Tiny shape of the issue (S 11, A 3, H 32, B 16, 64 rows, LAP, hard update every 4 steps) is td7_tiny's
SHAPES = {
    "tiny": lambda: load_golden("td7_tiny"),
    "b100": lambda: load_golden("td7_tiny_b100"),     # B = 100 in a 256-row replay: 12 padded rows
    "zs": lambda: load_golden("td7_tiny_zs"),         # zs_dim != hidden: no RLE_FUSE_FOLD
    "act": lambda: load_golden("td7_tiny_act"),       # non-default activations: the extended kernel instance
    "act_id": lambda: load_golden("td7_tiny_act_id"),  # identity critics: the q partials' extended-only variant
    "hp": lambda: load_golden("td7_tiny_hp"),         # policy_freq 3 (and the other hyper-parameters)
    "nolap": lambda: load_golden("td7_tiny_nolap"),   # use_lap=False
    "ant": lambda: _synthetic("Ant-v4", 256, 256, 2048, 2048, True, 42),
    "tiny250": lambda: _synthetic("Tiny-v0", 32, 16, 64, 50, True, 5),  # no hard update: multi-step programs
}


def _tapes(n, B, A, seed):
    rng = np.random.default_rng(7000 + seed)
    return {"u": rng.random((n, B), dtype=np.float32), "eps": rng.standard_normal((n, B, A), dtype=np.float32)}


def offline_engine(g, lmbda, plan=None):
    """harness.engine_from_golden with rle_config.bc_lambda: make_config, spec.agent_params,
    spec.replay_data and spec.init_priorities."""
    alg, env, H, B, Ncap, n_fill, _, use_lap, seed, extra = parse(g)
    S, A, hi = spec.TASKS[env]
    kw = {}
    for k, v in extra.items():
        if k in ("target_update_rate", "policy_freq"):
            kw[k] = int(v)
        elif k == "discount_factor":
            kw["discount"] = float(v)
        else:
            kw[k] = float(v)
    shape = shape_of(g)
    acts = {f"act_{k}": v for k, v in acts_of(g).items()}
    cfg = E.make_config(E.RLE_TD7, S, A, H, B, use_lap=use_lap, seed=seed, bc_lambda=lmbda, **kw, **shape, **acts)
    eng = E.Engine(cfg, plan)
    for net, params in spec.agent_params(alg, S, A, H, seed, **shape).items():
        for name, v in params.items():
            eng.set_param(net, name, v)
    rep = E.Replay(Ncap, S, A, use_lap, 0)
    fill_replay(rep, S, A, hi, n_fill, seed)
    if use_lap:
        p0 = spec.init_priorities(Ncap, seed + 2)
        p0[n_fill:] = 0.0
        rep.set_priority(p0, float(p0.max()))
    eng.bind(rep)
    return eng, rep


_REF = {}


def _reference(shape, lmbda, n):
    """The oracle's n-step trajectory of a shape, computed once and shared: per step info, indices,
    priorities, value bounds, the Adam moments after the first policy step, and the end parameters."""
    key = (shape, lmbda, n)
    if key in _REF:
        return _REF[key]
    torch.set_num_threads(4)
    g = SHAPES[shape]()
    orc, orep, _, _, B = build_offline(g, lmbda)
    A = spec.TASKS[str(g["meta_env"])][1]
    tp = _tapes(n, B, A, int(g["meta"][6]))
    ref = {"g": g, "tp": tp, "info": [], "ind": [], "prio": [], "vb": [], "m": None, "m_step": None}
    for t in range(n):
        i1, n1 = agents.run_steps(orc, "td7", orep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
        ref["info"] += i1
        ref["ind"] += n1
        ref["prio"].append(orep.priority.copy() if orc.lap else None)
        ref["vb"].append(np.array([orc.value_max, orc.value_min, orc.vt_max, orc.vt_min], np.float32))
        if ref["m"] is None and i1[0]["train/policy"] is not None:
            ref["m"] = {k: v for k, v in agents.moments(orc).items() if k.endswith(":m")}
            ref["m_step"] = t
    ref["params"] = {(net, k): v.detach().numpy().copy() for net, d in orc.nets().items() for k, v in d.items()}
    ref["table"] = np.array([[np.nan if i[k] is None else i[k] for k in INFO_KEYS] for i in ref["info"]], np.float64)
    _REF[key] = ref
    return ref


def _check_state(eng, rep, ref, t):
    Ncap = int(ref["g"]["meta"][2])
    np.testing.assert_array_equal(eng.last_indices(), ref["ind"][t])
    if ref["prio"][t] is not None:
        np.testing.assert_allclose(rep.get_priority(Ncap), ref["prio"][t], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(eng.value_bounds(), ref["vb"][t], rtol=1e-4, atol=1e-4)


def _check_moments(eng, ref):
    """tests/test_parity_gpu.py assert_moments' criterion (moments after steps 1 and 2): the first policy step
    is the critics' and the encoder's second Adam step or later."""
    for key, m in ref["m"].items():
        net, pname = key[:-2].split(".", 1)
        got = np.asarray(eng.get_adam(net, pname, 0, m.shape), np.float64)
        r = np.asarray(m, np.float64)
        d = np.abs(got - r)
        lim = 1e-4 * np.abs(r) + 1e-4 * max(np.abs(r).max(), 1e-30)
        assert (d <= lim).all(), (key, float(d.max()), float((d / lim).max()))


def _check_end(eng, ref, infos, n, bulk):
    infos = np.asarray(infos, np.float64)[:, :5]
    for t in range(n):
        print("info", t, infos[t].tolist(), ref["table"][t].tolist())
    np.testing.assert_array_equal(np.isnan(infos), np.isnan(ref["table"]))
    np.testing.assert_allclose(infos, ref["table"], rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    tol = 2 * 3e-4 * n + 1e-4
    for (net, name), v in ref["params"].items():
        d = np.abs(eng.get_param(net, name, v.shape).astype(np.float64) - v)
        assert d.max() <= tol, (net, name, float(d.max()))
        assert (d <= 1e-5).mean() >= bulk, (net, name, float((d <= 1e-5).mean()))


def _per_step(shape, lmbda, n, plan=None, bulk=0.99):
    ref = _reference(shape, lmbda, n)
    eng, rep = offline_engine(ref["g"], lmbda, plan)
    eng.set_tapes(u=ref["tp"]["u"], eps=ref["tp"]["eps"])
    infos = []
    for t in range(n):
        infos.append(eng.step(1)[0])
        _check_state(eng, rep, ref, t)
        if t == ref["m_step"]:
            _check_moments(eng, ref)
    eng.set_tapes()
    _check_end(eng, ref, infos, n, bulk)
    return eng


@pytest.mark.parametrize("lmbda", LMBDAS)
@pytest.mark.parametrize("shape,n", [("tiny", 8), ("b100", 8), ("zs", 8), ("act", 8), ("act_id", 6), ("hp", 9),
                                     ("nolap", 6)])
def test_offline_steps_match_oracle(shape, n, lmbda):
    """Single-step programs, step by step: policy steps on either side of a hard update (tiny: steps 2, 4 |
    6, 8), a batch of 100 padded to 112 (the padded rows add nothing to q_abs or bc and get no gradient),
    zs_dim != hidden (no folded zsa3), the extended kernel instance (ELU actor, ReLU critics; identity
    critics), policy_freq 3, and no LAP."""
    _per_step(shape, lmbda, n, bulk=0.999 if shape == "zs" else 0.99)


@pytest.mark.parametrize("lmbda", LMBDAS)
def test_offline_full_width_matches_oracle(lmbda):
    """The Ant shape (S 27, A 8, H 256, B 256, 2,048 rows), 4 steps: the q row partials span many column
    tiles and OP_BC's threads each own one batch row."""
    eng = _per_step("ant", lmbda, 4, bulk=0.999)
    assert " bc" in eng.describe(0) and " bc" not in eng.describe(1)


def _burst(shape, lmbda, calls, plan=None):
    n = sum(calls)
    ref = _reference(shape, lmbda, n)
    eng, rep = offline_engine(ref["g"], lmbda, plan)
    eng.set_tapes(u=ref["tp"]["u"], eps=ref["tp"]["eps"])
    infos, t = [], 0
    for c in calls:
        infos += list(eng.step(c))
        t += c
        _check_state(eng, rep, ref, t - 1)
    eng.set_tapes()
    return eng, ref, np.array(infos), n


PLANS = {"default": {}, "dispatch0": dict(dispatch=0), "no_pre": dict(fuse_off=["pre"]),
         "no_qdot": dict(fuse_off=["qdot"])}


@pytest.mark.parametrize("lmbda", LMBDAS)
@pytest.mark.parametrize("plan", list(PLANS))
def test_offline_program_kinds_match_oracle(plan, lmbda):
    """Every program kind that holds a policy step, Tiny shape without a hard update in the way: rle_step(11)
    runs 1 + 6 + 4 steps and rle_step(8) from the odd step count 6 + 2 (engine.cpp kRemK), under direct AQL
    dispatch and hipGraph replays, and without RLE_FUSE_PRE (the action gradient read from memory instead of
    recomputed in-tile) and RLE_FUSE_QDOT."""
    eng, ref, infos, n = _burst("tiny250", lmbda, (11, 8), E.make_plan(**PLANS[plan]))
    _check_end(eng, ref, infos, n, 0.99)


@pytest.mark.parametrize("field", ["dispatch", "dpf", "xcd", "lpt"])
def test_offline_launch_choices_are_bitwise_neutral(field):
    """q_abs, bc and the gradient operand are summed by row and by tile, in an order B and A alone fix: turning
    off the direct dispatch, the descriptor prefetch, the XCD tile order or the longest-first op order changes
    no bit of the info rows or of any parameter."""
    lmbda = 5.0
    e0, ref, i0, n = _burst("tiny250", lmbda, (11, 8))
    e1, _, i1, _ = _burst("tiny250", lmbda, (11, 8), E.make_plan(**{field: 0}))
    np.testing.assert_array_equal(i0, i1)
    for (net, name) in ref["params"]:
        np.testing.assert_array_equal(e0.get_param(net, name), e1.get_param(net, name), err_msg=f"{net}.{name}")


def test_online_config_through_the_offline_path_reproduces_the_golden():
    """bc_lambda = 0 builds the online programs: the td7_tiny golden's info rows, indices and value bounds through
    this file's construction path, three info columns and no new op."""
    g = load_golden("td7_tiny")
    eng, rep = offline_engine(g, 0.0)
    n = int(g["meta"][4])
    eng.set_tapes(u=g["tape_u"][:n], eps=g["tape_eps"][:n])
    infos = []
    for t in range(n):
        infos.append(eng.step(1)[0])
        np.testing.assert_array_equal(eng.last_indices(), g["ind"][t])
        if f"vbounds_{t}" in g:
            np.testing.assert_allclose(eng.value_bounds(), g[f"vbounds_{t}"].astype(np.float32), rtol=1e-4, atol=1e-4)
    eng.set_tapes()
    infos = np.array(infos)
    np.testing.assert_allclose(infos[:, :3], g["info"], rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    assert " bc" not in eng.describe(0)
    on, _ = offline_engine(g, 0.0)
    off, _ = offline_engine(g, 0.1)
    off.step(1), on.step(1)
    assert off.graph_stats()[0] == on.graph_stats()[0], "the offline policy step keeps the online level count"
    assert off.graph_stats()[1] == on.graph_stats()[1]


@pytest.mark.parametrize("check", ["RLE_AUDIT", "RLE_HAZARD"])
@pytest.mark.parametrize("shape", ["tiny250", "act_id", "ant"])
def test_offline_programs_pass_audit_and_hazard_checks(shape, check, monkeypatch):
    """The address replay of every GEMM (the identity segment of the action gradient and of its in-tile
    recomputation included) and the byte-level race check of every level, OP_BC's buffers among them, over an
    offline engine's single-step, multi-step and hard-update programs; then two steps run."""
    monkeypatch.setenv(check, "1")
    ref_g = SHAPES[shape]()
    eng, rep = offline_engine(ref_g, 0.1)
    eng.step(2)


def test_state_moves_between_online_and_offline_engines():
    """rle_copy_state, rle_copy_nets and the packed state work between engines whose bc_lambda differ."""
    g = load_golden("td7_tiny")
    on, _ = offline_engine(g, 0.0)
    off, _ = offline_engine(g, 0.1)
    off.step(4)
    on.copy_state_from(off)
    for net, d in spec.agent_params("td7", 11, 3, 32, 5).items():
        for name in d:
            np.testing.assert_array_equal(on.get_param(net, name), off.get_param(net, name))
    on2, _ = offline_engine(g, 0.0)
    on2.copy_nets_from(off)
    np.testing.assert_array_equal(on2.get_param("policy", "l3.weight"), off.get_param("policy", "l3.weight"))
    blob = off.state_export(E.STATE_ALL)
    on2.state_import(blob, E.STATE_ALL)
    np.testing.assert_array_equal(on2.get_adam("policy", "l0.weight", 0), off.get_adam("policy", "l0.weight", 0))


# ---- the Python mirror -------------------------------------------------------------------------------------

def _mirror():
    from rl.agent import TD7
    from rl.replay_memory import LAPReplayMemory
    from rl.runner.run import run_train_ops
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    return TD7, LAPReplayMemory, run_train_ops


def _dataset(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 11)).astype(np.float32), rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 11)).astype(np.float32),
            (rng.random(n) > 0.1).astype(np.float32))


def test_offline_agent_trains_from_a_fixed_dataset_and_survives_copies(tmp_path):
    TD7, LAPReplayMemory, run_train_ops = _mirror()
    B = 32
    ag = TD7("Tiny-v0", use_lap=True, hidden=32, batch_size=B, seed=9, offline=True, lmbda=0.5)
    assert ag.__getstate__()["_cfg"]["bc_lambda"] == 0.5 and ag.offline
    rep = LAPReplayMemory(512, "Tiny-v0")
    rep.append_batch(*_dataset(300, 3))
    infos = run_train_ops(type("R", (), {"replay_buffer": rep})(), ag, B, n_ops=4)
    keys = ["train/encoder", "train/q_fn", "train/policy", "train/bc", "train/q_abs"]
    assert [list(i) for i in infos] == [keys] * 4
    assert infos[0]["train/policy"] is None and infos[0]["train/bc"] is None and infos[0]["train/q_abs"] is None
    assert infos[1]["train/bc"] > 0 and infos[1]["train/q_abs"] > 0
    online = TD7("Tiny-v0", use_lap=True, hidden=32, batch_size=B, seed=9, lmbda=0.5)
    assert "bc_lambda" not in online._cfg and len(online._info_keys()) == 3
    path = tmp_path / "agent.pkl"
    ag.save(path)
    ag2 = TD7.load(path)
    ag3 = copy.deepcopy(ag)
    ag4 = pickle.loads(pickle.dumps(ag))
    for a in (ag2, ag3, ag4):
        assert a.offline and a.lmbda == 0.5 and a.engine.cfg.bc_lambda == 0.5
    # a 5th step (no policy update) and a 6th (with one) on the same explicit batches: identical info
    p0, m0 = rep.priority.numpy().copy(), rep.max_priority
    torch.manual_seed(7)
    batches = [rep.sample(B), rep.sample(B)]
    outs = []
    for a in (ag, ag2, ag3, ag4):
        rep.dev.set_priority(p0, m0)
        outs.append([a.train_ops(b, rep) for b in batches])
    assert outs[0][1]["train/bc"] is not None
    assert outs[0] == outs[1] == outs[2] == outs[3]
    ag.train_ops(rep.sample(48), rep)  # another batch size: the rebuilt engine is offline too
    assert ag.engine.cfg.bc_lambda == 0.5


def test_offline_train_ops_on_a_host_batch_equals_the_device_batch():
    """The host BATCH dict's action is the BC target: the rows go into the B-row ring the path builds."""
    TD7, LAPReplayMemory, _ = _mirror()
    B = 32
    kw = dict(use_lap=True, target_policy_noise=0.0, hidden=32, batch_size=B, seed=21, offline=True, lmbda=5.0)
    dev, host = TD7("Tiny-v0", **kw), TD7("Tiny-v0", **kw)
    rep = LAPReplayMemory(512, "Tiny-v0")
    hrep = LAPReplayMemory(512, "Tiny-v0")
    data = _dataset(300, 11)
    rep.append_batch(*data)
    hrep.append_batch(*data)
    for t in range(4):
        torch.manual_seed(500 + t)
        batch = rep.sample(B)
        ind = np.asarray(batch.ind)
        s, a, r, s2, d = rep.dev.gather(ind)
        hrep.ind = batch.ind
        hb = {"state": s, "action": a, "reward": r, "next_state": s2, "done": d}
        i_dev = dev.train_ops(batch, rep)
        i_host = host.train_ops(hb, hrep)
        assert list(i_dev) == list(i_host) and len(i_dev) == 5
        for k in i_dev:
            if i_dev[k] is None:
                assert i_host[k] is None
            else:
                assert abs(i_host[k] - i_dev[k]) <= 1e-6 * (1 + abs(i_dev[k])), (k, i_host[k], i_dev[k])
    for net, d in dev.state_dict().items():
        for name, v in d.items():
            np.testing.assert_array_equal(host.state_dict()[net][name], v)
