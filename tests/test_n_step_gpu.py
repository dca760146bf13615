"""n-step returns on the device (rle_set_n_step, rle_replay_gather_nstep) against tests/n_step_ref.py and the
unmodified CPU oracle.

The gather is compared bit for bit: every product and sum of the law is one float32 operation on both sides.
The step parity cases step the oracle on a ring whose rows were replaced on the host by the reference's n-step
rows, on the same indices; tolerances are the ones tests/test_shape_edges_gpu.py and tests/test_offline_td3_gpu.py
hold the same quantities to, none new: info columns rel 1e-3 (harness.LOSS_RTOL, atol 1e-4), priorities rtol 1e-4 /
atol 1e-5, end parameters within 2 * 3e-4 * k + 1e-4 with 99% of each tensor within 1e-5
(test_engine_gpu.assert_params_close).  replay/hops is a sum of small integers times 1 / B: rel 1e-6.
"""

import copy
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
import layer_norm  # noqa: E402,F401  (registers the oracle's ln_<act> composites)
import n_step_cases as C  # noqa: E402
import n_step_ref as R  # noqa: E402
from harness import ALGO, LOSS_RTOL  # noqa: E402
from offline_td3_oracle import TD3BCOracle  # noqa: E402
from oracle import agents, spec  # noqa: E402
from oracle.replay import Replay as OracleReplay  # noqa: E402
from test_engine_gpu import assert_params_close  # noqa: E402

A = 3


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8])


def _loaded(kind, S):
    r = C.ring(kind, S, A)
    rep = E.Replay(C.CAP, S, A, False)
    C.load(rep, r)
    return rep, r


def _check_gather(rep, r, ind, n, what):
    s, a, rw, s2, nd, hops = rep.gather_nstep(ind, n, C.GAMMA)
    Rn, ns, ndn, h = R.n_step(r, ind, n, C.GAMMA)
    _same(s, r["state"][ind], what + " state")
    _same(a, r["action"][ind], what + " action")
    _same(rw, Rn, what + " reward")
    _same(s2, ns, what + " next_state")
    _same(nd, ndn, what + " notdone")
    _same(hops, h, what + " hops")
    return hops


# ---- the gather, bit for bit ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("S", [5, 130, 520])
def test_gather_equals_the_reference_bitwise(S, kind):
    """S 5: per-wave stores; S 130: the quad LDS path (a multiple of four queries) and its fallback; S 520: the
    tail loop past 512 columns."""
    rep, r = _loaded(kind, S)
    size = r["size"]
    lists = [np.arange(size, dtype=np.int64)]
    if S == 130:
        lists = [np.resize(lists[0], (size + 3) // 4 * 4), lists[0][: size - 2 if size % 4 == 0 else size]]
        assert len(lists[0]) % 4 == 0 and len(lists[1]) % 4 != 0 and set(lists[0].tolist()) == set(range(size))
        if size == C.CAP:
            assert (len(lists[0]), len(lists[1])) == (64, 62)
    for n in C.N_TESTED:
        for ind in lists:
            hops = _check_gather(rep, r, ind, n, f"{kind} S{S} n{n} q{len(ind)}")
            if len(ind) >= size:
                assert set(hops.tolist()) == set(range(1, n + 1))
    for ind in lists:  # n_step = 1 is rle_replay_gather
        for got, want, name in zip(rep.gather_nstep(ind, 1, C.GAMMA)[:5], rep.gather(ind), "sarSd"):
            _same(got, want, f"n1 {name}")
    for bad in (0, 9):
        with pytest.raises(RuntimeError, match="rle error -1"):
            rep.gather_nstep(lists[0], bad, C.GAMMA)
    if size < C.CAP:
        with pytest.raises(RuntimeError, match="rle error -1"):
            rep.gather_nstep(np.array([size]), 2, C.GAMMA)
    rep.close()


def _exported(rep, ptr, size):
    s, a, rw, s2, d = rep.export_rows(0, C.CAP)
    return dict(state=s, action=a, reward=rw, next_state=s2, notdone=d, ptr=ptr, size=size)


@pytest.mark.parametrize("kind", ["part", "wrap"])
def test_hops_survive_normalize_states(kind):
    rep, r = _loaded(kind, 11)
    ind = np.arange(r["size"], dtype=np.int64)
    before = rep.gather_nstep(ind, 5, C.GAMMA)[5]
    mean, std = rep.state_stats()
    rep.normalize_states(mean, std + np.float32(1e-3))
    now = _exported(rep, r["ptr"], r["size"])
    assert not np.array_equal(now["state"][: r["size"]], r["state"][: r["size"]])
    hops = _check_gather(rep, now, ind, 5, f"normalized {kind}")
    _same(hops, before, "hops after normalize_states")
    rep.close()


def test_appends_move_the_device_write_pointer():
    """A full ring with ptr 33: three appended rows that continue slot 32's episode.  Slot 32 now walks into them,
    and the row before the new ptr stops at one hop although the old row after it continues it in the data."""
    rep, r = _loaded("mid", 11)
    rng = np.random.default_rng(3)
    nxt = rng.standard_normal((3, 11)).astype(np.float32)
    nxt[2] = r["state"][36]  # (the appended episode's last next_state is the old slot 36's state: only ptr stops)
    st = np.stack([r["next_state"][32], nxt[0], nxt[1]])
    act = rng.uniform(-1, 1, (3, A)).astype(np.float32)
    rw = rng.standard_normal(3).astype(np.float32)
    rep.append(st, act, rw, nxt, np.ones(3, np.float32))
    assert rep.state()[:2] == (36, C.CAP)
    now = _exported(rep, 36, C.CAP)
    _same(now["state"][33:36], st, "appended rows")
    ind = np.arange(C.CAP, dtype=np.int64)
    hops = _check_gather(rep, now, ind, 3, "after append")
    assert hops[35] == 1 and hops[34] == 2 and hops[32] == 3
    assert R.n_step_one(dict(now, ptr=0), 35, 3, C.GAMMA)[3] == 3  # (the data alone would go on)
    # set_state and rle_replay_copy carry the pointer too
    rep.set_state(35, C.CAP, 1.0)
    assert rep.gather_nstep(ind, 3, C.GAMMA)[5][34] == 1
    other = E.Replay(C.CAP, 11, A, False)
    other.copy_from(rep)
    _check_gather(other, dict(now, ptr=35), ind, 3, "copied ring")
    other.close()
    rep.close()


# ---- the step against the oracle ------------------------------------------------------------------------------

S_T, A_T, _ = spec.TASKS["Tiny-v0"]
H, N_STEPS, GAMMA = 64, 3, 0.99
KEYS = {
    "td3": ("train/q_fn", "train/policy", "norm/policy"),
    "td3bc": ("train/q_fn", "train/policy", "norm/policy", "train/bc", "train/lmbda"),
    "sac": ("train/q_fn", "tmp", "norm/tmp", "train/policy", "train/tmp", "entropy"),
}
# name -> (oracle kind, B, use_lap, LayerNorm critics, seed)
STEP_CASES = {
    "td3-b16": ("td3", 16, False, False, 31),
    "td3-lap-b20": ("td3", 20, True, False, 32),
    "sac-auto-b18": ("sac", 18, False, False, 33),
    "td3bc-ln-b16": ("td3bc", 16, False, True, 34),
}
BC_ALPHA = 2.5


def _case_inputs(case):
    kind, B, lap, ln, seed = STEP_CASES[case]
    alg = "sac" if kind == "sac" else "td3"
    r = C.ring("wrap", S_T, A_T, seed)
    tp = spec.tapes(alg, B, A_T, N_STEPS, seed + 3)
    ind = np.random.default_rng(seed + 4).integers(0, r["size"], (N_STEPS, B)).astype(np.int64)
    p0 = spec.init_priorities(C.CAP, seed + 2) if lap else None
    return kind, alg, B, lap, ln, seed, r, tp, ind, p0


def _engine(case, n_step):
    kind, alg, B, lap, ln, seed, r, tp, ind, p0 = _case_inputs(case)
    cfg = E.make_config(ALGO[alg], S_T, A_T, H, B, use_lap=lap, seed=seed, discount=GAMMA)
    eng = E.Engine(cfg, None, ext=E.make_config_ext(bc_alpha=BC_ALPHA) if kind == "td3bc" else None)
    for net, params in spec.agent_params(alg, S_T, A_T, H, seed).items():
        for name, v in params.items():
            eng.set_param(net, name, v)
    if ln:
        eng.set_layer_norm(True)
    if n_step > 1:
        eng.set_n_step(n_step)
    assert eng.n_step() == n_step
    rep = E.Replay(C.CAP, S_T, A_T, lap)
    C.load(rep, r)
    if lap:
        rep.set_priority(p0, float(p0.max()))
    eng.bind(rep)
    return eng, rep


def _run_engine(case, n_step):
    _, alg, *_, tp, ind, _ = _case_inputs(case)
    eng, rep = _engine(case, n_step)
    eng.set_tapes(ind=ind, eps=tp["eps"], eps_pi=tp.get("eps_pi"))
    rows = np.array([eng.step(1)[0] for _ in range(N_STEPS)])
    eng.set_tapes()
    return eng, rep, rows


def _run_oracle(case, n_step):
    kind, alg, B, lap, ln, seed, r, tp, ind, p0 = _case_inputs(case)
    torch.set_num_threads(1)
    size = r["size"]
    Rn, ns, ndn, hops = R.n_step(r, np.arange(size), n_step, GAMMA)
    orep = OracleReplay(C.CAP, S_T, A_T, 1.0, 0.0, lap)
    orep.state[:size], orep.action[:size] = r["state"][:size], r["action"][:size]
    orep.reward[:size, 0], orep.next_state[:size], orep.done[:size, 0] = Rn, ns, ndn
    orep.ptr, orep.size = r["ptr"], size
    if lap:
        orep.priority[:] = p0
        orep.max_priority = float(p0.max())
    nets = spec.agent_params(alg, S_T, A_T, H, seed)
    acts = {"critic": "ln_relu"} if ln else None
    if kind == "td3bc":
        orc = TD3BCOracle(nets, alpha=BC_ALPHA, discount=GAMMA, use_lap=lap, acts=acts)
    else:
        orc = agents.make_oracle(alg, nets, A_T, lap, acts=acts, discount=GAMMA)
    table = np.full((N_STEPS, len(KEYS[kind])), np.nan)
    for t in range(N_STEPS):
        batch = orep.gather(ind[t])
        args = (tp["eps"][t], tp["eps_pi"][t]) if alg == "sac" else (tp["eps"][t],)
        info = orc.step(batch, orep, *args)
        table[t] = [np.nan if info.get(k) is None else info[k] for k in KEYS[kind]]
    mean_hops = np.array([hops[ind[t]].astype(np.float64).mean() for t in range(N_STEPS)])
    return orc, orep, table, mean_hops


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_matches_the_oracle_on_n_step_rows(case):
    kind = STEP_CASES[case][0]
    k = len(KEYS[kind])
    orc, orep, table, mean_hops = _run_oracle(case, 3)
    eng, rep, rows = _run_engine(case, 3)
    for t in range(N_STEPS):
        print("NSTEP", case, t, rows[t].tolist(), table[t].tolist(), mean_hops[t])
    np.testing.assert_array_equal(np.isnan(rows[:, :k]), np.isnan(table))
    np.testing.assert_allclose(rows[:, :k], table, rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    np.testing.assert_allclose(rows[:, k], mean_hops, rtol=1e-6, atol=0)
    assert 1.0 < mean_hops.min() and mean_hops.max() < 3.0  # (the batches mix hop counts)
    if STEP_CASES[case][2]:
        np.testing.assert_allclose(rep.get_priority(C.CAP), orep.priority, rtol=1e-4, atol=1e-5)
    tol = 2 * 3e-4 * N_STEPS + 1e-4
    for net, params in orc.nets().items():
        for name, v in params.items():
            assert_params_close(np.ravel(eng.get_param(net, name)), v.detach().numpy().ravel(), tol, (case, net, name))
    # the cross-check that must differ: the same case with one-step targets
    eng1, rep1, rows1 = _run_engine(case, 1)
    assert np.isfinite(rows1[:, 0]).all()
    assert not np.allclose(rows1[:, 0], rows[:, 0], rtol=10 * LOSS_RTOL, atol=1e-4), (rows1[:, 0], rows[:, 0])
    # ... and one-step targets match the oracle on the ring as it is
    _, _, table1, _ = _run_oracle(case, 1)
    np.testing.assert_allclose(rows1[:, :k], table1, rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    for h in (eng, eng1, rep, rep1):
        h.close()


# ---- settings and lifecycle -----------------------------------------------------------------------------------

def test_setter_errors_and_level_counts():
    eng, rep = _engine("td3-b16", 1)
    assert eng.n_step() == 1
    for bad in (0, 9, -3):
        with pytest.raises(RuntimeError, match="rle error -1"):
            eng.set_n_step(bad)
    eng.set_n_step(8)
    eng.set_n_step(1)
    assert eng.n_step() == 1
    eng.step(2)
    with pytest.raises(RuntimeError, match="rle error -3"):
        eng.set_n_step(3)
    with pytest.raises(RuntimeError, match="rle error -3"):
        eng.set_n_step(1)
    plain_stats = eng.graph_stats()
    eng3, rep3 = _engine("td3-b16", 3)
    eng3.step(2)
    assert eng3.graph_stats() == plain_stats
    # the same with every earlier link of the instance chain switched on: LayerNorm, dropout and clipping
    pair = []
    for n in (1, 3):
        e, r = _engine("td3bc-ln-b16", n)
        e.set_critic_dropout(0.01)
        e.set_grad_clip(0.5)
        e.step(2)
        pair.append((e, r, e.graph_stats()))
    assert pair[0][2] == pair[1][2]
    td7 = E.Engine(E.make_config(E.RLE_TD7, S_T, A_T, 32, 16, seed=1))
    with pytest.raises(RuntimeError, match="rle error -1"):
        td7.set_n_step(2)
    td7.set_n_step(1)
    assert td7.n_step() == 1
    # not part of the state: a copy between engines whose n differ
    eng3.copy_state_from(eng)
    assert eng3.n_step() == 3
    for h in (eng, rep, eng3, rep3, td7, *[x for p in pair for x in p[:2]]):
        h.close()


# ---- the Python mirror ----------------------------------------------------------------------------------------

def _mirror_replay():
    from rl.replay_memory import SimpleReplayMemory

    r = C.ring("mid", 11, 3)
    rep = SimpleReplayMemory(C.CAP, "Tiny-v0")
    rep.append_batch(r["state"], r["action"] * np.float32(0.5), r["reward"], r["next_state"], r["notdone"])
    return rep, dict(r, ptr=0, size=C.CAP)


def test_mirror_keyword_survives_copies_and_both_training_paths_agree():
    from rl.agent import SAC, TD3, TD7
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    kw = dict(hidden=32, batch_size=16, seed=5)
    ag = TD3("Tiny-v0", n_step=3, **kw)
    assert ag.n_step == 3 and ag.engine.n_step() == 3 and ag._info_keys()[-1] == "replay/hops"
    copies = [pickle.loads(pickle.dumps(ag)), copy.deepcopy(ag)]
    for other in copies:
        assert other.n_step == 3 and other.engine.n_step() == 3
    ag.to("cuda:0")
    assert ag.engine.n_step() == 3
    rep, ring = _mirror_replay()
    # train_n draws its own indices; sample + train_ops on those indices gives the same info row
    want = ag.train_n(rep, 16, 1)[0]
    ind = np.array(rep.ind)
    assert 1.0 < want["replay/hops"] <= 3.0
    np.testing.assert_allclose(want["replay/hops"], R.n_step(ring, ind, 3, 0.99)[3].mean(), rtol=1e-6)
    rep2, _ = _mirror_replay()
    batch = rep2.sample(16, n_step=3, discount=0.99)
    Rn, ns, ndn, hops = R.n_step(ring, batch.ind, 3, 0.99)
    _same(batch["reward"].numpy()[:, 0], Rn, "sample reward")
    _same(batch["next_state"].numpy(), ns, "sample next_state")
    _same(batch["done"].numpy()[:, 0], ndn, "sample done")
    _same(batch.hops, hops, "sample hops")
    batch.ind = ind
    got = copies[1].train_ops(batch, rep2)
    assert got == want, (got, want)
    with pytest.raises(ValueError, match="no episode order"):
        copies[0].train_ops({k: v for k, v in batch.items()}, None)
    plain = TD3("Tiny-v0", **kw)
    assert plain.engine.n_step() == 1 and "replay/hops" not in plain.train_n(_mirror_replay()[0], 16, 1)[0]
    sac = SAC("Tiny-v0", n_step=2, **kw)
    row = sac.train_n(_mirror_replay()[0], 16, 1)[0]
    assert sac.engine.n_step() == 2 and 1.0 <= row["replay/hops"] <= 2.0 and np.isfinite(row["train/q_fn"])
    with pytest.raises(ValueError, match="one-step model"):
        TD7("Tiny-v0", n_step=2, **kw)
