"""Dataset state normalisation on the device (rle_replay_state_stats, rle_replay_normalize_states,
replay.normalize_states) against NumPy.

Bounds, from the number formats alone: the statistics are accumulated in fp64 on both sides in different orders
and then rounded to fp32, so the cast can land on the neighbouring float: 1 fp32 ulp.  The transform is one
correctly rounded subtraction and one correctly rounded division per element, which NumPy's float32 arithmetic
reproduces exactly; 2 ulp only guards against a compiler default (a reciprocal multiply).
"""

import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
from harness import LOSS_RTOL  # noqa: E402
from oracle import agents, replay as oreplay, spec  # noqa: E402

A = 3


def _rows(n, S, seed):
    """n transitions whose state features differ in offset and spread (so mean and std are not 0 and 1)."""
    rng = np.random.default_rng(seed)
    off = rng.uniform(-5, 5, S).astype(np.float32)
    spread = rng.uniform(0.1, 4, S).astype(np.float32)
    s = (off + spread * rng.standard_normal((n, S))).astype(np.float32)
    s2 = (off + spread * rng.standard_normal((n, S))).astype(np.float32)
    a = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    r = rng.standard_normal(n).astype(np.float32)
    d = (rng.random(n) > 0.1).astype(np.float32)
    return s, a, r, s2, d


def _ulps(got, ref):
    """|got - ref| in units of ref's fp32 spacing."""
    ref = np.asarray(ref, np.float32)
    return np.abs(np.asarray(got, np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("size", [1, 7, 4097])
@pytest.mark.parametrize("S", [1, 16, 17, 376])
def test_stats_and_transform_match_numpy(S, size):
    """A LAP ring of capacity size + 9 with every slot holding data and size rows valid: mean and std within
    1 ulp of NumPy's float64 statistics of the float32 rows cast to fp32; after the transform rows [0, size) of
    state and next_state within 2 ulp of NumPy's fp32 (x - m) / s, rows at or past size, actions, rewards, masks
    and priorities bit for bit what they were, and the LAP sampler draws the same indices."""
    cap = size + 9
    rep = E.Replay(cap, S, A, True, 0)
    s, a, r, s2, d = _rows(cap, S, 100 * S + size)
    prio = np.random.default_rng(5).uniform(1.0, 3.0, cap).astype(np.float32)
    rep.import_rows(0, s, a, r, s2, d, prio)
    rep.set_state(size % cap, size, float(prio.max()))
    u = np.random.default_rng(6).random(64, dtype=np.float32)
    ind0 = rep.sample_indices(u)
    p0 = rep.get_priority(cap)
    mean, std = rep.state_stats()
    ref_m = s[:size].astype(np.float64).mean(0).astype(np.float32)
    ref_s = s[:size].astype(np.float64).std(0).astype(np.float32)
    print("mean ulps", float(_ulps(mean, ref_m).max()), "std ulps", float(_ulps(std, ref_s).max()))
    assert _ulps(mean, ref_m).max() <= 1.0
    assert _ulps(std, ref_s).max() <= 1.0
    scale = std + np.float32(1e-3)
    rep.normalize_states(mean, scale)
    gs, ga, gr, gs2, gd, gp = rep.export_rows(0, cap, priority=True)
    for got, x in ((gs, s), (gs2, s2)):
        want = (x[:size] - mean) / scale
        assert want.dtype == np.float32
        ul = _ulps(got[:size], want)
        print("transform ulps", float(ul.max()))
        assert ul.max() <= 2.0
        np.testing.assert_array_equal(got[size:], x[size:])
    np.testing.assert_array_equal(ga, a)
    np.testing.assert_array_equal(gr, r)
    np.testing.assert_array_equal(gd, d)
    np.testing.assert_array_equal(gp, prio)
    np.testing.assert_array_equal(rep.get_priority(cap), p0)
    np.testing.assert_array_equal(rep.sample_indices(u), ind0)
    assert rep.state() == (size % cap, size, pytest.approx(float(prio.max())))


def test_bad_arguments_and_the_empty_replay():
    """scale == 0 or non-finite, a non-finite shift, a NULL pointer: RLE_EINVAL; an empty replay: RLE_ESTATE."""
    lib = E.lib()
    rep = E.Replay(64, 5, A, False, 0)
    f32p = ctypes.POINTER(ctypes.c_float)
    ok = np.ones(5, np.float32)

    def ptr(v):
        return v.ctypes.data_as(f32p)

    assert lib.rle_replay_state_stats(rep.h, ptr(ok), ptr(ok)) == -3  # RLE_ESTATE
    assert lib.rle_replay_normalize_states(rep.h, ptr(ok), ptr(ok)) == -3
    rep.append(*_rows(10, 5, 1))
    assert lib.rle_replay_state_stats(rep.h, None, ptr(ok)) == -1  # RLE_EINVAL
    assert lib.rle_replay_state_stats(rep.h, ptr(ok), None) == -1
    assert lib.rle_replay_normalize_states(rep.h, None, ptr(ok)) == -1
    assert lib.rle_replay_normalize_states(rep.h, ptr(ok), None) == -1
    before = rep.export_rows(0, 10)
    for bad in (0.0, float("nan"), float("inf")):
        sc = ok.copy()
        sc[3] = bad
        assert lib.rle_replay_normalize_states(rep.h, ptr(ok), ptr(sc)) == -1, bad
        assert b"scale" in lib.rle_last_error()
    sh = ok.copy()
    sh[0] = float("nan")
    assert lib.rle_replay_normalize_states(rep.h, ptr(sh), ptr(ok)) == -1
    for x, y in zip(before, rep.export_rows(0, 10)):  # (a refused call changes nothing)
        np.testing.assert_array_equal(x, y)


def test_normalize_states_once_and_the_flag_travels():
    """replay.normalize_states(eps) returns (mean, std + eps), applies it to state and next_state, raises
    RuntimeError on a second call, and the flag and vectors travel with pickle and deepcopy."""
    from rl.replay_memory import LAPReplayMemory

    rep = LAPReplayMemory(300, None, state_dim=17, action_dim=A)
    s, a, r, s2, d = _rows(200, 17, 3)
    rep.append_batch(s[:150], a[:150], r[:150], s2[:150], d[:150])
    for i in range(150, 200):  # (staged appends are flushed first)
        rep.append([s[i], a[i], r[i], s2[i], d[i]])
    assert not rep.states_normalized and rep.state_mean is None
    rep.flush()
    mean0, std0 = rep.dev.state_stats()
    mean, scale = rep.normalize_states(eps=1e-3)
    ref_m = s.astype(np.float64).mean(0).astype(np.float32)
    ref_s = s.astype(np.float64).std(0).astype(np.float32)
    assert _ulps(mean, ref_m).max() <= 1.0 and _ulps(std0, ref_s).max() <= 1.0
    np.testing.assert_array_equal(mean, mean0)
    np.testing.assert_array_equal(scale, std0 + np.float32(1e-3))  # (scale = std + eps in fp32)
    gs, _, _, gs2, _ = rep.dev.export_rows(0, 200)
    assert _ulps(gs, (s - mean) / scale).max() <= 2.0 and _ulps(gs2, (s2 - mean) / scale).max() <= 2.0
    # (each feature now has mean 0 and std = std / (std + eps) >= 0.1 / 0.101 for these rows)
    assert np.abs(gs.mean(0)).max() < 1e-4 and (gs.std(0) > 0.989).all() and (gs.std(0) < 1.0001).all()
    with pytest.raises(RuntimeError, match="already normalised"):
        rep.normalize_states()
    for other in (copy.deepcopy(rep), pickle.loads(pickle.dumps(rep))):
        assert other.states_normalized
        np.testing.assert_array_equal(other.state_mean, mean)
        np.testing.assert_array_equal(other.state_scale, scale)
        np.testing.assert_array_equal(other.dev.export_rows(0, 200)[0], gs)
        with pytest.raises(RuntimeError):
            other.normalize_states()
    empty = LAPReplayMemory(64, None, state_dim=17, action_dim=A)
    with pytest.raises(RuntimeError, match="-3"):
        empty.normalize_states()
    assert not empty.states_normalized


def test_pad_columns_stay_zero_and_the_prefetched_batch_is_redrawn():
    """S = 17 (ring rows padded to 32 columns): a TD3 engine that has taken a step -- so it holds a prefetched
    batch of un-normalised rows -- takes 4 more after normalize_states and matches the oracle stepping on
    NumPy-normalised data: indices exact, info at harness.LOSS_RTOL, parameters by the bulk criterion.  A value
    in the pad columns would enter every first-layer GEMM's reduction; a stale prefetch would show in step 2."""
    from rl.replay_memory import LAPReplayMemory

    S, H, B, seed, n_fill, n = 17, 32, 16, 31, 200, 5
    torch.set_num_threads(1)
    nets = spec.agent_params("td3", S, A, H, seed)
    s, a, r, s2, d = _rows(n_fill, S, 9)
    rep = LAPReplayMemory(256, None, state_dim=S, action_dim=A)
    rep.append_batch(s, a, r, s2, d)
    orep = oreplay.Replay(256, S, A, np.ones(A, np.float32), np.zeros(A, np.float32), True)
    for i in range(n_fill):
        orep.append(s[i], a[i], float(r[i]), s2[i], float(d[i]))
    orc = agents.TD3Oracle(nets, use_lap=True)
    eng = E.Engine(E.make_config(E.RLE_TD3, S, A, H, B, use_lap=True, seed=seed))
    for net, params in nets.items():
        for name, v in params.items():
            eng.set_param(net, name, v)
    eng.bind(rep.dev)
    rng = np.random.default_rng(77)
    tp = {"u": rng.random((n, B), dtype=np.float32), "eps": rng.standard_normal((n, B, A), dtype=np.float32)}
    eng.set_tapes(u=tp["u"], eps=tp["eps"])
    infos = [eng.step(1)[0]]
    ref_info, ref_ind = agents.run_steps(orc, "td3", orep, tp, 1, B)
    np.testing.assert_array_equal(eng.last_indices(), ref_ind[0])
    mean, scale = rep.normalize_states()
    orep.state[:n_fill] = (orep.state[:n_fill] - mean) / scale
    orep.next_state[:n_fill] = (orep.next_state[:n_fill] - mean) / scale
    for t in range(1, n):
        infos.append(eng.step(1)[0])
        i1, n1 = agents.run_steps(orc, "td3", orep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
        ref_info += i1
        np.testing.assert_array_equal(eng.last_indices(), n1[0])
    eng.set_tapes()
    keys = ("train/q_fn", "train/policy", "norm/policy")
    table = np.array([[np.nan if i[k] is None else i[k] for k in keys] for i in ref_info], np.float64)
    infos = np.asarray(infos, np.float64)[:, :3]
    for t in range(n):
        print("info", t, infos[t].tolist(), table[t].tolist())
    np.testing.assert_allclose(infos, table, rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    np.testing.assert_allclose(rep.dev.get_priority(256), orep.priority, rtol=1e-4, atol=1e-5)
    tol = 2 * 3e-4 * n + 1e-4
    for net, dd in orc.nets().items():
        for name, v in dd.items():
            v = v.detach().numpy()
            dlt = np.abs(eng.get_param(net, name, v.shape).astype(np.float64) - v)
            assert dlt.max() <= tol, (net, name, float(dlt.max()))
            assert (dlt <= 1e-5).mean() >= 0.99, (net, name, float((dlt <= 1e-5).mean()))
