"""Offline SAC on the GPU: the engine's AWAC policy step (rle_config_ext awac_lambda) against
tests/offline_sac_oracle.py's AWACOracle, with identical u / eps / eps_pi tapes.

Criteria: those tests/test_offline_td3_gpu.py and tests/harness.py apply, none new (tests/offline_sac_cases.py
restates them once for the host and the device tests): indices exact; info columns rel 1e-3 (harness.LOSS_RTOL,
atol 1e-4); the Adam moments (m and v) after step 1 |d| <= 1e-4 |m| + 1e-4 max|m|; end parameters every element
within 2 * 3e-4 * n + 1e-4 and 99% of each tensor within 1e-5.  Cases, datasets (exact +1 / -1 / 0 action entries,
log_std columns past both clamps) and seeds: tests/offline_sac_cases.py, whose float32 oracle
tests/test_offline_sac.py holds to the same criteria against float64 on the CPU.  Every case runs four steps:
step 1 alone (the single-step program), then a burst of 3 (a multi-step remainder program).  Every test here goes
through awac_lambda or SAC(offline=) and so fails on an engine without them.
"""

import copy
import pickle
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
import offline_sac_cases as C  # noqa: E402
from harness import LOSS_RTOL  # noqa: E402

assert LOSS_RTOL == C.LOSS_RTOL
ALL_FUSIONS = [k for k in E.FUSE if k != "priosample"]  # (priosample is opt-in: off unless switched on)


def offline_engine(case, lmbda=C.LMBDA, plan=None, ext=True):
    """An engine of the case's shape, nets and dataset through rle_create_ext (ext=False: through rle_create)."""
    c = C.CASES[case]
    cfg = E.make_config(E.RLE_SAC, c.S, c.A, c.H, c.B, seed=c.seed, tmp=0.0, min_log_std=C.MIN_LOG_STD,
                        max_log_std=C.MAX_LOG_STD, **C.shape_kw(case))
    eng = E.Engine(cfg, plan, ext=E.make_config_ext(awac_lambda=lmbda) if ext else None)
    for net, params in C.nets(case).items():
        for name, v in params.items():
            eng.set_param(net, name, v)
    rep = E.Replay(C.NCAP, c.S, c.A, False, 0)
    rep.append(*C.dataset(case))
    eng.bind(rep)
    return eng, rep


def _tape(eng, tp):
    eng.set_tapes(u=tp["u"], eps=tp["eps"], eps_pi=tp["eps_pi"])


def _against_oracle(case, plan=None):
    ref = C.reference(case)
    f32 = ref["f32"]
    n = C.N_STEPS
    eng, rep = offline_engine(case, plan=plan)
    _tape(eng, ref["tp"])
    infos = [eng.step(1)[0]]
    np.testing.assert_array_equal(eng.last_indices(), f32["ind"][0])

    def adam(key):
        net, pname = key[:-2].split(".", 1)
        return eng.get_adam(net, pname, 0 if key.endswith(":m") else 1)

    bad = C.moment_shortfalls(adam, f32["m"])
    infos += list(eng.step(n - 1))
    np.testing.assert_array_equal(eng.last_indices(), f32["ind"][n - 1])
    eng.set_tapes()
    infos = np.asarray(infos, np.float64)[:, :5]
    for t in range(n):
        print("AWAC", case, "info", t, infos[t].tolist(), f32["table"][t].tolist())
    bad += C.end_shortfalls(infos, eng.get_param, f32, n)
    assert not bad, bad
    return eng


@pytest.mark.parametrize("case", list(C.CASES))
def test_offline_sac_steps_match_oracle(case):
    """(11, 3) H 32 B 16; B 17 (a second row block with one valid row) and B 1; A 24 and A 25 (both sides of the
    fused raw head's 2A = 48); hidden [260, 260] with S 16, A 24, B 15 (width % 16 != 0, H > 256)."""
    eng = _against_oracle(case)
    desc = eng.describe(0)
    assert re.search(r"(?m)[: ]\*?awac( |$)", desc), desc
    assert bool(re.search(r"sacfwd\]", desc)) == (case not in ("a25", "h260")), desc  # the path the case is for


def test_offline_sac_unfused_steps_match_oracle():
    """Every fusion off on the baseline: the standalone rsample, no pre-layers, the unsplit step end."""
    eng = _against_oracle("base", E.make_plan(fuse_off=ALL_FUSIONS))
    assert re.search(r"(?m)[: ]\*?sacfwd( |$)", eng.describe(0))


def _run(eng, tp, calls):
    _tape(eng, tp)
    infos = []
    for c in calls:
        infos += list(eng.step(c))
    eng.set_tapes()
    return np.array(infos)


def _names(case):
    return [(net, name) for net, d in C.nets(case).items() for name in d]


def test_awac_lambda_zero_is_the_online_program():
    """rle_create_ext(awac_lambda = 0) and rle_create: identical rle_graph_describe text for every graph kind
    and bitwise-identical 4-step results (info rows, parameters, Adam moments); three info columns, no new op."""
    on, _ = offline_engine("base", 0.0, ext=False)
    z, _ = offline_engine("base", 0.0, ext=True)
    tp = C.tapes("base")
    i_on, i_z = _run(on, tp, (1, 3)), _run(z, tp, (1, 3))
    np.testing.assert_array_equal(i_on, i_z)
    for which in (0, 1, 2):
        texts = []
        for e in (on, z):
            try:
                texts.append(e.describe(which))
            except RuntimeError as err:  # (a graph kind this algorithm does not have)
                texts.append(str(err))
        assert texts[0] == texts[1], which
    assert "awac" not in z.describe(0) and "sacbwd" in z.describe(0)
    for net, name in _names("base"):
        np.testing.assert_array_equal(on.get_param(net, name), z.get_param(net, name))
        if net in ("policy", "q1", "q2"):
            for w in (0, 1):
                np.testing.assert_array_equal(on.get_adam(net, name, w), z.get_adam(net, name, w))


def test_burst_equals_single_steps_bitwise():
    """Default plan: rle_step(20) (SAC's 8-step graph twice, then its 4-step remainder) equals 20 single steps
    bit for bit -- info rows and every parameter."""
    n = 20
    tp = C.tapes("b17", n)
    e_b, _ = offline_engine("b17")
    e_s, _ = offline_engine("b17")
    i_b, i_s = _run(e_b, tp, (n,)), _run(e_s, tp, (1,) * n)
    np.testing.assert_array_equal(i_b, i_s)
    assert np.isfinite(i_b[:, :5]).all()
    for net, name in _names("b17"):
        np.testing.assert_array_equal(e_b.get_param(net, name), e_s.get_param(net, name), err_msg=f"{net}.{name}")


@pytest.mark.parametrize("plan", [None, "unfused"])
def test_offline_policy_step_description_and_level_count(plan):
    """The offline policy step names the new op and holds no critic input gradient and no squashed-Gaussian
    backward (neither the op nor the epilogue) and no loss head in policy mode; rle_graph_stats reports no more
    levels per step than online SAC at the same shape."""
    p = E.make_plan(fuse_off=ALL_FUSIONS) if plan else None
    c = C.CASES["base"]
    on, _ = offline_engine("base", 0.0, p, ext=False)
    off, _ = offline_engine("base", C.LMBDA, p)
    on.step(1), off.step(1)
    d_on, d_off = on.describe(0), off.describe(0)
    print(d_off)
    assert "awac" in d_off and "awac" not in d_on
    assert "sacbwd" not in d_off and "sacbwd" in d_on
    # critic input gradients: a DX whose reduction runs over a critic's hidden width and whose output is the
    # critic's input (S + A padded) or, fused, the head + dx ops.  Online has 2 critic-loss head+dx ops and 2 more
    # in the policy pass; offline keeps the critic loss's two only.
    n_head = lambda d: len(re.findall(r"head\+dx|[: ]\*?head( |$)", d, re.M))  # noqa: E731
    assert n_head(d_off) < n_head(d_on)
    gemms = lambda d: len(re.findall(r"gemm\[", d))  # noqa: E731
    print("GEMMs per step: online", gemms(d_on), "offline", gemms(d_off))
    (pol_on, plain_on), (pol_off, plain_off) = on.graph_stats(), off.graph_stats()
    print("levels per step: online", pol_on, plain_on, "offline", pol_off, plain_off)
    assert pol_off <= pol_on and plain_off <= plain_on
    assert c.B == 16


@pytest.mark.parametrize("case", ["b17", "a25", "h260"])
def test_offline_sac_programs_pass_audit_and_hazard_checks(case, monkeypatch):
    """The address replay of every GEMM and the byte-level race check of every level, OP_AWAC's buffers among
    them, over an offline engine's single-step and multi-step programs; then steps run."""
    monkeypatch.setenv("RLE_AUDIT", "1")
    monkeypatch.setenv("RLE_HAZARD", "1")
    eng, rep = offline_engine(case)
    eng.step(3)


def test_state_moves_between_online_and_offline_sac_engines():
    """rle_copy_state, rle_copy_nets and the packed state work between an online fixed-tmp = 0 engine and an
    offline one."""
    on, _ = offline_engine("base", 0.0, ext=False)
    off, _ = offline_engine("base")
    off.step(4)
    on.copy_state_from(off)
    for net, name in _names("base"):
        np.testing.assert_array_equal(on.get_param(net, name), off.get_param(net, name))
    np.testing.assert_array_equal(on.counters(), off.counters())
    on2, _ = offline_engine("base", 0.0, ext=False)
    on2.copy_nets_from(off)
    np.testing.assert_array_equal(on2.get_param("policy", "mlp.0.weight"), off.get_param("policy", "mlp.0.weight"))
    blob = off.state_export(E.STATE_ALL)
    assert blob.size == on2.state_size(E.STATE_ALL)
    on2.state_import(blob, E.STATE_ALL)
    np.testing.assert_array_equal(on2.get_adam("policy", "mlp.0.weight", 0), off.get_adam("policy", "mlp.0.weight", 0))
    off2, _ = offline_engine("base", 1.0)
    off2.state_import(on2.state_export(E.STATE_ALL), E.STATE_ALL)
    np.testing.assert_array_equal(off2.get_adam("q1", "mlp.0.weight", 1), off.get_adam("q1", "mlp.0.weight", 1))
    # the copies train on: an online engine that took an offline engine's state, and the reverse
    on.step(2), off2.step(2)


# ---- the Python mirror -------------------------------------------------------------------------------------

def _mirror():
    from rl.agent import SAC
    from rl.replay_memory import SimpleReplayMemory
    from rl.runner.run import run_train_ops
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    return SAC, SimpleReplayMemory, run_train_ops


def _dataset(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    a[::5, 0], a[1::5, 1], a[2::5, 2] = 0.5, -0.5, 0.0  # (stored as a / 0.5: exact +1, -1 and 0)
    return (rng.standard_normal((n, 11)).astype(np.float32), a, rng.standard_normal(n).astype(np.float32),
            rng.standard_normal((n, 11)).astype(np.float32), (rng.random(n) > 0.1).astype(np.float32))


KEYS = ["train/q_fn", "train/policy", "entropy", "train/adv", "train/weight"]


def test_offline_sac_agent_trains_from_a_fixed_dataset_and_survives_copies(tmp_path):
    SAC, SimpleReplayMemory, run_train_ops = _mirror()
    B = 32
    ag = SAC("Tiny-v0", hidden=32, batch_size=B, seed=9, offline=True, lmbda=0.5)
    assert ag.__getstate__()["_ext"] == {"awac_lambda": 0.5} and ag.offline and not ag.auto_tmp_mode and ag.tmp == 0.0
    rep = SimpleReplayMemory(512, "Tiny-v0")
    rep.append_batch(*_dataset(300, 3))
    infos = run_train_ops(type("R", (), {"replay_buffer": rep})(), ag, B, n_ops=4)
    assert [list(i) for i in infos] == [KEYS] * 4
    assert all(np.isfinite(list(i.values())).all() for i in infos)
    assert all(0 < i["train/weight"] <= 100 for i in infos)
    online = SAC("Tiny-v0", tmp=0.0, hidden=32, batch_size=B, seed=9, lmbda=0.5)
    assert not online.offline and "_ext" not in online.__dict__ and online.engine.ext is None
    assert list(online.train_ops(rep.sample(B), rep)) == KEYS[:3]
    path = tmp_path / "agent.pkl"
    ag.save(path)
    ag2 = SAC.load(path)
    ag3 = copy.deepcopy(ag)
    ag4 = pickle.loads(pickle.dumps(ag))
    for a in (ag2, ag3, ag4):
        assert a.offline and a.lmbda == 0.5 and a.engine.ext.awac_lambda == 0.5 and a.engine.cfg.tmp == 0.0
    # two more steps on the same explicit batches: the agent and its three copies were left at the same Philox
    # position, so the info rows are identical
    torch.manual_seed(7)
    batches = [rep.sample(B), rep.sample(B)]
    outs = [[a.train_ops(b, rep) for b in batches] for a in (ag, ag2, ag3, ag4)]
    assert list(outs[0][0]) == KEYS
    assert outs[0] == outs[1] == outs[2] == outs[3]
    ag.train_ops(rep.sample(48), rep)  # another batch size: the rebuilt engine is offline too
    assert ag.engine.ext.awac_lambda == 0.5 and ag.batch_size == 48 and list(ag.train_ops(rep.sample(48), rep)) == KEYS


def test_offline_sac_train_ops_on_a_host_batch_equals_the_device_batch():
    """The host BATCH dict's action is the dataset action: the rows go into the B-row ring the path builds."""
    SAC, SimpleReplayMemory, _ = _mirror()
    B = 32
    kw = dict(hidden=32, batch_size=B, seed=21, offline=True, lmbda=0.5)
    dev, host = SAC("Tiny-v0", **kw), SAC("Tiny-v0", **kw)
    rep = SimpleReplayMemory(512, "Tiny-v0")
    rep.append_batch(*_dataset(300, 11))
    for t in range(3):
        torch.manual_seed(500 + t)
        batch = rep.sample(B)
        s, a, r, s2, d = rep.dev.gather(np.asarray(batch.ind))
        assert (a == 1.0).any() and (a == -1.0).any() and (a == 0.0).any()
        i_dev = dev.train_ops(batch, rep)
        i_host = host.train_ops({"state": s, "action": a, "reward": r, "next_state": s2, "done": d}, None)
        assert list(i_dev) == list(i_host) == KEYS
        for k in i_dev:
            assert abs(i_host[k] - i_dev[k]) <= 1e-6 * (1 + abs(i_dev[k])), (k, i_host[k], i_dev[k])
    for net, d in dev.state_dict().items():
        for name, v in d.items():
            np.testing.assert_array_equal(host.state_dict()[net][name], v)
