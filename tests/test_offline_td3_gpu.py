"""Offline TD3 on the GPU: the engine's policy step with the TD3+BC objective (rle_config_ext bc_alpha) against
tests/offline_td3_oracle.py's TD3BCOracle, step by step on seeded tapes.

Tolerances are those tests/test_engine_gpu.py and tests/test_offline_gpu.py hold the same quantities to against
the oracle, none new: info columns rel 1e-3 (harness.LOSS_RTOL, atol 1e-4); priorities rtol 1e-4 / atol 1e-5;
indices exact; parameters after k steps every element within 2 * 3e-4 * k + 1e-4 and 99% of each (H = 32)
tensor within 1e-5; the Adam moments (m and v) after the first policy step |d| <= 1e-4 |m| + 1e-4 max|m|
(tests/test_parity_gpu.py's criterion).  tests/test_offline_td3.py shows on the CPU that at alpha = 2.5 both the
Q part and the cloning part of the action gradient are >= 10% of it on every golden used here, so these cases
fail with either term missing.  Every test here goes through rle_create_ext or TD3(offline=) and so fails on an
engine without them.
"""

import contextlib
import copy
import pickle

import numpy as np
import pytest
import torch

from conftest import acts_of, load_golden, shape_of

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
from harness import LOSS_RTOL, fill_replay, parse  # noqa: E402
from offline_td3_oracle import INFO_KEYS, build_offline_td3  # noqa: E402
from oracle import agents, spec  # noqa: E402

ALPHA = 2.5
ALL_FUSIONS = [k for k in E.FUSE if k != "priosample"]  # (priosample is opt-in: off unless switched on)


def _synthetic(env, H, B, ncap, n_fill, use_lap, seed):
    return {"meta_alg": np.array("td3"), "meta_env": np.array(env),
            "meta": np.array([H, B, ncap, n_fill, 0, int(use_lap), seed]),
            "meta_extra_keys": np.array([], dtype="<U32"), "meta_extra_vals": np.array([], np.float64)}


# Action-width and batch edges (oracle against engine, no golden file), as tests/edge_cases.py builds its cases:
# name -> (S, A, H, B, use_lap, seed).  A = 1; A = 17 pads to 32 columns; A = 33 is one past the A <= 32 in-tile
# actor path (engine.cpp actor_pre); odd S and H % 16 != 0 with B = 31 (one masked row in a padded batch of 32).
EDGES = {"edge_a1": (11, 1, 32, 16, True, 301), "edge_a17": (11, 17, 32, 16, True, 302),
         "edge_a33": (11, 33, 32, 16, False, 303), "edge_odd": (33, 5, 36, 31, True, 304)}

SHAPES = {name: (lambda name=name: load_golden(name))
          for name in ("td3_tiny", "td3_tiny_lap", "td3_tiny_b100", "td3_tiny_deep", "td3_tiny_act", "td3_tiny_hp")}
for _name, (_S, _A, _H, _B, _lap, _seed) in EDGES.items():
    SHAPES[_name] = (lambda n=_name, H=_H, B=_B, lap=_lap, seed=_seed: _synthetic(n, H, B, 256, 200, lap, seed))


@contextlib.contextmanager
def _env(shape):
    """oracle.spec.TASKS[shape] = the edge case's (S, A, action bound 1) while the block runs."""
    if shape not in EDGES:
        yield
        return
    S, A = EDGES[shape][:2]
    spec.TASKS[shape] = (S, A, 1.0)
    try:
        yield
    finally:
        del spec.TASKS[shape]


def _tapes(n, B, A, seed):
    rng = np.random.default_rng(9000 + seed)
    return {"u": rng.random((n, B), dtype=np.float32), "eps": rng.standard_normal((n, B, A), dtype=np.float32)}


def offline_engine(g, alpha, plan=None, ext=True):
    """harness.engine_from_golden through rle_create_ext (ext=False: through rle_create)."""
    alg, env, H, B, Ncap, n_fill, _, use_lap, seed, extra = parse(g)
    S, A, hi = spec.TASKS[env]
    kw = {}
    for k, v in extra.items():
        if k == "policy_freq":
            kw[k] = int(v)
        elif k == "discount_factor":
            kw["discount"] = float(v)
        else:
            kw[k] = float(v)
    shape = shape_of(g)
    acts = {f"act_{k}": v for k, v in acts_of(g).items()}
    cfg = E.make_config(E.RLE_TD3, S, A, H, B, use_lap=use_lap, seed=seed, **kw, **shape, **acts)
    eng = E.Engine(cfg, plan, ext=E.make_config_ext(bc_alpha=alpha) if ext else None)
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


def _reference(shape, alpha, n):
    """The oracle's n-step trajectory of a shape, computed once and shared (read-only): per step info, indices
    and priorities, the Adam moments (m and v) after the first policy step, and the end parameters."""
    key = (shape, alpha, n)
    if key in _REF:
        return _REF[key]
    torch.set_num_threads(1)  # (as tests/edge_cases.py: the CPU oracle tests that follow in a whole-suite run expect it)
    g = SHAPES[shape]()
    with _env(shape):
        orc, orep, _, _, B = build_offline_td3(g, alpha)
        A = spec.TASKS[str(g["meta_env"])][1]
    tp = _tapes(n, B, A, int(g["meta"][6]))
    ref = {"g": g, "tp": tp, "info": [], "ind": [], "prio": [], "maxp": [], "m": None, "m_step": None}
    for t in range(n):
        i1, n1 = agents.run_steps(orc, "td3", orep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
        ref["info"] += i1
        ref["ind"] += n1
        ref["prio"].append(orep.priority.copy() if orc.lap else None)
        ref["maxp"].append(float(orep.max_priority) if orc.lap else None)
        if ref["m"] is None and i1[0]["train/policy"] is not None:
            ref["m"] = dict(agents.moments(orc))  # (first and second moments, ":m" / ":v")
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
        assert rep.state()[2] == pytest.approx(ref["maxp"][t], rel=1e-4)


def _check_moments(eng, ref):
    for key, m in ref["m"].items():
        net, pname = key[:-2].split(".", 1)
        got = np.asarray(eng.get_adam(net, pname, 0 if key.endswith(":m") else 1, m.shape), np.float64)
        r = np.asarray(m, np.float64)
        d = np.abs(got - r)
        lim = 1e-4 * np.abs(r) + 1e-4 * max(np.abs(r).max(), 1e-30)
        assert (d <= lim).all(), (key, float(d.max()), float((d / lim).max()))


def _check_end(eng, ref, infos, n, bulk=0.99):
    infos = np.asarray(infos, np.float64)[:, :5]
    for t in range(n):
        print("info", t, infos[t].tolist(), ref["table"][t].tolist())
    np.testing.assert_array_equal(np.isnan(infos), np.isnan(ref["table"]))
    np.testing.assert_allclose(infos, ref["table"], rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    tol = 2 * 3e-4 * n + 1e-4
    worst_bulk, far = 1.0, 0.0
    for (net, name), v in ref["params"].items():
        d = np.abs(eng.get_param(net, name, v.shape).astype(np.float64) - v)
        worst_bulk, far = min(worst_bulk, float((d <= 1e-5).mean())), max(far, float(d.max()))
    print(f"parameters after {n} steps: worst bulk {worst_bulk:.4f}, worst |d| {far:.2e}")
    for (net, name), v in ref["params"].items():
        d = np.abs(eng.get_param(net, name, v.shape).astype(np.float64) - v)
        assert d.max() <= tol, (net, name, float(d.max()))
        assert (d <= 1e-5).mean() >= bulk, (net, name, float((d <= 1e-5).mean()))


def _per_step(shape, alpha, n, plan=None):
    ref = _reference(shape, alpha, n)
    with _env(shape):
        eng, rep = offline_engine(ref["g"], alpha, plan)
    eng.set_tapes(u=ref["tp"]["u"], eps=ref["tp"]["eps"])
    infos = []
    for t in range(n):
        infos.append(eng.step(1)[0])
        _check_state(eng, rep, ref, t)
        if t == ref["m_step"]:
            _check_moments(eng, ref)
    eng.set_tapes()
    _check_end(eng, ref, infos, n)
    return eng


@pytest.mark.parametrize("shape,alpha", [("td3_tiny", 2.5), ("td3_tiny_lap", 2.5), ("td3_tiny_b100", 2.5),
                                         ("td3_tiny_deep", 2.5), ("td3_tiny_act", 2.5), ("td3_tiny_hp", 2.5),
                                         ("td3_tiny", 0.25)])
def test_offline_td3_steps_match_oracle(shape, alpha):
    """Single-step programs, 6 steps (policy steps 1, 3, 5; hp: 1, 4): the nets and replay of the goldens, with
    priorities and the max priority (lap), a batch of 100 padded to 112 (the masked rows count in no mean),
    deeper nets, the extended kernel instance (act), other hyper-parameters (hp), and the BC-dominated second
    point alpha = 0.25."""
    eng = _per_step(shape, alpha, 6)
    assert " bc" in eng.describe(0) and " bc" not in eng.describe(1)


@pytest.mark.parametrize("shape", ["td3_tiny_b100", "edge_odd"])
def test_offline_td3_unfused_steps_match_oracle(shape):
    """Every fusion off: the standalone head and OP_BC mode 2 (q_abs from the head's |min| partials) with masked
    rows -- B = 100 padded to 112, B = 31 padded to 32 -- step by step against the oracle."""
    _per_step(shape, ALPHA, 6 if shape == "td3_tiny_b100" else 5, E.make_plan(fuse_off=ALL_FUSIONS))


@pytest.mark.parametrize("shape", list(EDGES))
def test_offline_td3_action_width_edges_match_oracle(shape):
    """A = 1, A = 17 (pads to 32), A = 33 (past the in-tile actor path), and odd S with B = 31."""
    _per_step(shape, ALPHA, 5)


def _burst(shape, alpha, calls, plan=None):
    n = sum(calls)
    ref = _reference(shape, alpha, n)
    with _env(shape):
        eng, rep = offline_engine(ref["g"], alpha, plan)
    eng.set_tapes(u=ref["tp"]["u"], eps=ref["tp"]["eps"])
    infos, t = [], 0
    for c in calls:
        infos += list(eng.step(c))
        t += c
        _check_state(eng, rep, ref, t - 1)
    eng.set_tapes()
    return eng, ref, np.array(infos), n


def test_offline_td3_burst_equals_single_steps_bitwise_and_the_unfused_plan_matches():
    """Default plan: rle_step(20) (1 + a 16-step graph + 3) equals 20 single steps bit for bit -- info rows and
    every parameter -- and matches the oracle; the same burst with every fusion switched off (the standalone
    head, the action gradient read from memory, the standalone Polyak) matches the oracle at the same
    tolerances (its reductions are split differently, so it is not held to the fused run bit for bit)."""
    n = 20
    e_b, ref, i_b, _ = _burst("td3_tiny_lap", ALPHA, (n,))
    e_s, _, i_s, _ = _burst("td3_tiny_lap", ALPHA, (1,) * n)
    np.testing.assert_array_equal(i_b, i_s)
    for (net, name) in ref["params"]:
        np.testing.assert_array_equal(e_b.get_param(net, name), e_s.get_param(net, name), err_msg=f"{net}.{name}")
    _check_end(e_b, ref, i_b, n)
    e_u, _, i_u, _ = _burst("td3_tiny_lap", ALPHA, (n,), E.make_plan(fuse_off=ALL_FUSIONS))
    _check_end(e_u, ref, i_u, n)
    # the unfused burst against unfused single steps: bit for bit as well
    e_us, _, i_us, _ = _burst("td3_tiny_lap", ALPHA, (1,) * n, E.make_plan(fuse_off=ALL_FUSIONS))
    np.testing.assert_array_equal(i_u, i_us)
    for (net, name) in ref["params"]:
        np.testing.assert_array_equal(e_u.get_param(net, name), e_us.get_param(net, name), err_msg=f"{net}.{name}")


def test_alpha_zero_is_the_online_program():
    """rle_create_ext(bc_alpha = 0) and rle_create: identical rle_graph_describe text for every graph kind and
    bitwise-identical 6-step results (info rows, parameters, Adam moments), three info columns, no new op."""
    g = load_golden("td3_tiny_lap")
    on, _ = offline_engine(g, 0.0, ext=False)
    z, _ = offline_engine(g, 0.0, ext=True)
    tp = _tapes(6, 16, 3, 1)
    infos = []
    for e in (on, z):
        e.set_tapes(u=tp["u"], eps=tp["eps"])
        infos.append(np.array([e.step(1)[0] for _ in range(3)] + list(e.step(3))))
        e.set_tapes()
    np.testing.assert_array_equal(infos[0][:, :3], infos[1][:, :3])
    for which in (0, 1, 2):
        texts = []
        for e in (on, z):
            try:
                texts.append(e.describe(which))
            except RuntimeError as err:  # (a graph kind this algorithm does not have)
                texts.append(str(err))
        assert texts[0] == texts[1], which
    assert " bc" not in z.describe(0)
    for net, d in spec.agent_params("td3", 11, 3, 32, 8).items():
        for name in d:
            np.testing.assert_array_equal(on.get_param(net, name), z.get_param(net, name))
            if net in ("policy", "q1", "q2"):
                for w in (0, 1):
                    np.testing.assert_array_equal(on.get_adam(net, name, w), z.get_adam(net, name, w))


@pytest.mark.parametrize("shape", ["td3_tiny", "td3_tiny_b100"])
def test_offline_level_counts(shape):
    """Plain steps keep their level count; a policy step gains at most one level, under the default plan (the
    fused head: q_abs comes from the row partials beside it) and with every fusion off (the standalone head:
    q_abs comes from its |min| partials a level later)."""
    g = load_golden(shape)
    for plan in (None, E.make_plan(fuse_off=ALL_FUSIONS)):
        on, _ = offline_engine(g, 0.0, plan, ext=False)
        off, _ = offline_engine(g, ALPHA, plan)
        on.step(1), off.step(1)
        (pol_on, plain_on), (pol_off, plain_off) = on.graph_stats(), off.graph_stats()
        print(shape, "levels policy / plain: online", pol_on, plain_on, "offline", pol_off, plain_off)
        assert plain_off == plain_on
        assert pol_on <= pol_off <= pol_on + 1


@pytest.mark.parametrize("check", ["RLE_AUDIT", "RLE_HAZARD"])
@pytest.mark.parametrize("shape", ["td3_tiny_lap", "td3_tiny_b100", "edge_a33"])
def test_offline_td3_programs_pass_audit_and_hazard_checks(shape, check, monkeypatch):
    """The address replay of every GEMM (the identity segment of the action gradient and of its in-tile
    recomputation included) and the byte-level race check of every level, OP_BC's buffers and the Adam
    epilogues' lmbda among them, over an offline engine's single-step and multi-step programs; then steps run."""
    monkeypatch.setenv(check, "1")
    with _env(shape):
        eng, rep = offline_engine(SHAPES[shape](), ALPHA)
    eng.step(3)


def test_state_moves_between_online_and_offline_td3_engines():
    """rle_copy_state, rle_copy_nets and the packed state work between engines whose bc_alpha differ."""
    g = load_golden("td3_tiny")
    on, _ = offline_engine(g, 0.0, ext=False)
    off, _ = offline_engine(g, ALPHA)
    off.step(4)
    on.copy_state_from(off)
    names = [(net, name) for net, d in spec.agent_params("td3", 11, 3, 32, 7).items() for name in d]
    for net, name in names:
        np.testing.assert_array_equal(on.get_param(net, name), off.get_param(net, name))
    np.testing.assert_array_equal(on.counters(), off.counters())
    on2, _ = offline_engine(g, 0.0, ext=False)
    on2.copy_nets_from(off)
    np.testing.assert_array_equal(on2.get_param("policy", "mlp.0.weight"), off.get_param("policy", "mlp.0.weight"))
    blob = off.state_export(E.STATE_ALL)
    on2.state_import(blob, E.STATE_ALL)
    np.testing.assert_array_equal(on2.get_adam("policy", "mlp.0.weight", 0), off.get_adam("policy", "mlp.0.weight", 0))
    off2, _ = offline_engine(g, 0.25)
    off2.state_import(on2.state_export(E.STATE_ALL), E.STATE_ALL)
    np.testing.assert_array_equal(off2.get_adam("q1", "mlp.0.weight", 1), off.get_adam("q1", "mlp.0.weight", 1))


# ---- the Python mirror -------------------------------------------------------------------------------------

def _mirror():
    from rl.agent import TD3
    from rl.replay_memory import LAPReplayMemory
    from rl.runner.run import run_train_ops
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    return TD3, LAPReplayMemory, run_train_ops


def _dataset(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 11)).astype(np.float32), rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 11)).astype(np.float32),
            (rng.random(n) > 0.1).astype(np.float32))


def test_offline_td3_agent_trains_from_a_fixed_dataset_and_survives_copies(tmp_path):
    TD3, LAPReplayMemory, run_train_ops = _mirror()
    B = 32
    ag = TD3("Tiny-v0", use_lap=True, hidden=32, batch_size=B, seed=9, offline=True, alpha=1.5)
    assert ag.__getstate__()["_ext"] == {"bc_alpha": 1.5} and ag.offline
    rep = LAPReplayMemory(512, "Tiny-v0")
    rep.append_batch(*_dataset(300, 3))
    infos = run_train_ops(type("R", (), {"replay_buffer": rep})(), ag, B, n_ops=4)
    keys = ["train/q_fn", "train/policy", "norm/policy", "train/bc", "train/lmbda"]
    assert [list(i) for i in infos] == [keys] * 4
    assert all(infos[1][k] is None for k in keys[1:])
    assert infos[0]["train/bc"] > 0 and infos[0]["train/lmbda"] > 0 and infos[0]["norm/policy"] > 0
    online = TD3("Tiny-v0", use_lap=True, hidden=32, batch_size=B, seed=9, alpha=1.5)
    assert not online.offline and "_ext" not in online.__dict__ and online.engine.ext is None
    assert list(online.train_ops(rep.sample(B), rep)) == keys[:3]
    path = tmp_path / "agent.pkl"
    ag.save(path)
    ag2 = TD3.load(path)
    ag3 = copy.deepcopy(ag)
    ag4 = pickle.loads(pickle.dumps(ag))
    for a in (ag2, ag3, ag4):
        assert a.offline and a.alpha == 1.5 and a.engine.ext.bc_alpha == 1.5
    # a 5th step (with a policy update) and a 6th (without) on the same explicit batches: identical info
    p0, m0 = rep.priority.numpy().copy(), rep.max_priority
    torch.manual_seed(7)
    batches = [rep.sample(B), rep.sample(B)]
    outs = []
    for a in (ag, ag2, ag3, ag4):
        rep.dev.set_priority(p0, m0)
        outs.append([a.train_ops(b, rep) for b in batches])
    assert outs[0][0]["train/bc"] is not None and outs[0][1]["train/bc"] is None
    assert outs[0] == outs[1] == outs[2] == outs[3]
    ag.train_ops(rep.sample(48), rep)  # another batch size: the rebuilt engine is offline too
    assert ag.engine.ext.bc_alpha == 1.5 and ag.batch_size == 48
    # an agent pickled before the offline mode existed (no such attributes) loads as online
    st = online.__getstate__()
    for k in ("offline", "alpha"):
        st.pop(k)
    old = TD3.__new__(TD3)
    old.__setstate__(copy.deepcopy(st))
    assert not old.offline and old.engine.ext is None and len(old._info_keys()) == 3


def test_offline_td3_train_ops_on_a_host_batch_equals_the_device_batch():
    """The host BATCH dict's action is the cloning target: the rows go into the B-row ring the path builds."""
    TD3, LAPReplayMemory, _ = _mirror()
    B = 32
    kw = dict(use_lap=True, target_policy_noise=0.0, hidden=32, batch_size=B, seed=21, offline=True, alpha=2.5)
    dev, host = TD3("Tiny-v0", **kw), TD3("Tiny-v0", **kw)
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


def test_set_obs_norm_feeds_the_normalised_observation_to_the_act_path():
    """sample(deterministic=True) after set_obs_norm(mean, scale) is the oracle forward of (obs - mean) / scale
    (tests/test_mirror_gpu.py's tolerance for the deterministic action); it is pickled with the agent, available
    to every agent class, and None clears it."""
    from oracle import nets as N
    from rl.agent import SAC, TD7

    TD3, _, _ = _mirror()
    rng = np.random.default_rng(4)
    obs = rng.standard_normal(11).astype(np.float32)
    mean = rng.standard_normal(11).astype(np.float32)
    scale = (0.5 + rng.random(11)).astype(np.float32)
    ag = TD3("Tiny-v0", hidden=32, batch_size=32, seed=2, offline=True)
    plain = ag.sample(obs, deterministic=True)
    ag.set_obs_norm(mean, scale)
    sd = {n: torch.from_numpy(v) for n, v in ag.state_dict()["policy"].items()}
    x = torch.from_numpy((obs - mean) / scale)[None]
    with torch.no_grad():
        ref = torch.tanh(N.mlp(sd, x)).numpy()[0] * 0.5
    got = ag.sample(obs, deterministic=True)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    assert not np.array_equal(got, plain)
    ag2 = pickle.loads(pickle.dumps(ag))
    np.testing.assert_array_equal(ag2.sample(obs, deterministic=True), got)
    np.testing.assert_array_equal(copy.deepcopy(ag).sample(obs, deterministic=True), got)
    ag.set_obs_norm(None)
    np.testing.assert_array_equal(ag.sample(obs, deterministic=True), plain)
    with pytest.raises(ValueError):
        ag.set_obs_norm(mean, np.zeros(11, np.float32))
    for cls in (TD7, SAC):
        other = cls("Tiny-v0", hidden=32, batch_size=32, seed=2)
        a0 = other.sample(obs, deterministic=True)
        a1 = other.sample(((obs - mean) / scale).astype(np.float32), deterministic=True)
        other.set_obs_norm(mean, scale)
        np.testing.assert_array_equal(other.sample(obs, deterministic=True), a1)
        other.set_obs_norm(None)
        np.testing.assert_array_equal(other.sample(obs, deterministic=True), a0)
