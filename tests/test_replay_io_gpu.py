"""Save, restore, copy and move of the HBM replays (rle_replay_export / _import / _set_state / _copy and the
index-mode pack behind rle_replay_gather) through the C ABI and the Python replays: what comes out is what
went in, bit for bit, and an interrupted and restored training run continues like an uninterrupted one."""

import copy
import pickle

import numpy as np
import pytest
import torch

from oracle import replay as OR
from rl import _engine as E
from rl.agent import TD7
from rl.replay_memory import LAPReplayMemory, SimpleReplayMemory
from rl.runner.run import run_train_ops
from rl.utils import register_env

pytestmark = pytest.mark.gpu

register_env("Tiny-v0", 11, 3, -0.5, 0.5)
S, A, HI = 11, 3, 0.5
R = E.REPLAY_IO_ROWS
FIELDS = ("state", "action", "reward", "next_state", "notdone")


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, S)), rng.uniform(-HI, HI, (n, A)), rng.standard_normal(n),
            rng.standard_normal((n, S)), (rng.random(n) > 0.1).astype(np.float64))


def _fill(rep, n, seed):
    rep.append_batch(*_rows(n, seed))
    return rep


def _assert_sd_equal(a, b):
    assert a["meta"] == b["meta"]
    assert set(a) == set(b)
    for k in a:
        if k == "meta":
            continue
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- 1. export equals what was appended ------------------------------------------------------------------

@pytest.mark.parametrize("lap,n", [(True, 2 * R + 500), (True, 300), (False, 2 * R + 500)])
def test_state_dict_equals_the_appended_rows(lap, n):
    cap = 2 * R + 37
    rows = _rows(n, 11)
    rep = (LAPReplayMemory if lap else SimpleReplayMemory)(cap, "Tiny-v0")
    rep.append_batch(*rows)
    orc = OR.Replay(cap, S, A, np.full(A, HI, np.float32), np.zeros(A, np.float32), lap)
    for t in zip(*rows):
        orc.append(*t)
    sd = rep.state_dict()
    m = sd["meta"]
    assert (m["ptr"], m["size"]) == (orc.ptr, orc.size) == ((463, cap) if n > cap else (300, 300))
    assert np.float32(m["max_priority"]) == np.float32(orc.max_priority)
    assert (m["capacity"], m["state_dim"], m["action_dim"], m["lap"], m["env_id"]) == (cap, S, A, lap, "Tiny-v0")
    assert m["action_scale"] == [HI] * A and m["action_bias"] == [0.0] * A
    size = orc.size
    for k, ref in (("state", orc.state), ("action", orc.action), ("reward", orc.reward[:, 0]),
                   ("next_state", orc.next_state), ("notdone", orc.done[:, 0])):
        assert sd[k].dtype == np.float32 and len(sd[k]) == size
        np.testing.assert_array_equal(sd[k], ref[:size], err_msg=k)
    if lap:
        np.testing.assert_array_equal(sd["priority"], orc.priority[:size])
    else:
        assert "priority" not in sd
    assert sd["ind"] is None


# ---- 2. range edges through the ABI ----------------------------------------------------------------------

def test_export_ranges_equal_gather_of_the_same_slots():
    cap = 2 * R + 37
    rep = E.Replay(cap, S, A, True)
    rep.fill_random(cap, 5)
    for first, count in ((0, 1), (cap - 1, 1), (R - 1, 2), (R, R), (5, 0)):
        got = rep.export_rows(first, count, priority=True)
        ref = rep.gather(np.arange(first, first + count))
        assert len(got) == 6
        for g, r_ in zip(got[:5], ref):
            assert g.shape == r_.shape and len(g) == count
            np.testing.assert_array_equal(g, r_)
        np.testing.assert_array_equal(got[5], rep.get_priority()[first:first + count])
    # only some of the fields
    lib = E.lib()
    a = np.empty((3, A), np.float32)
    E._check(lib.rle_replay_export(rep.h, 7, 3, None, E._fp(a), None, None, None, None))
    np.testing.assert_array_equal(a, rep.gather(np.arange(7, 10))[1])
    # argument checks: each refused with RLE_EINVAL and a message, nothing written
    buf = np.zeros(4, np.float32)
    for first, count in ((-1, 1), (0, -1), (cap, 1), (cap - 1, 2)):
        assert lib.rle_replay_export(rep.h, first, count, None, None, E._fp(buf), None, None, None) == -1
        assert b"export" in lib.rle_last_error()
        assert lib.rle_replay_import(rep.h, first, count, None, None, E._fp(buf), None, None, None) == -1
        assert b"import" in lib.rle_last_error()
    for ptr, size, mp in ((cap, 1, 1.0), (-1, 1, 1.0), (0, cap + 1, 1.0), (0, -1, 1.0), (0, 1, 0.0), (0, 1, -2.0),
                          (0, 1, float("inf")), (0, 1, float("nan"))):
        assert lib.rle_replay_set_state(rep.h, ptr, size, mp) == -1
        assert b"set_state" in lib.rle_last_error()
    plain = E.Replay(64, S, A, False)
    assert lib.rle_replay_export(plain.h, 0, 1, None, None, None, None, None, E._fp(buf)) == -1
    assert b"LAP" in lib.rle_last_error()
    assert lib.rle_replay_copy(plain.h, rep.h) == -1
    assert b"copy" in lib.rle_last_error()
    with pytest.raises(RuntimeError, match="out of range"):
        rep.gather(np.array([0, cap]))


# ---- 3. Humanoid width -----------------------------------------------------------------------------------

def test_humanoid_width_export_import_gather():
    n, Sh, Ah = 4100, 376, 17  # (padded row widths 384 and 32)
    src = E.Replay(n, Sh, Ah, True)
    src.fill_random(n, 3)
    rows = src.export_rows(0, n, priority=True)
    assert rows[0].shape == (n, Sh) and rows[1].shape == (n, Ah)
    assert np.abs(rows[0]).max() > 0 and np.abs(rows[1]).max() > 0 and len(np.unique(rows[0][:, -1])) > n // 2
    dst = E.Replay(n, Sh, Ah, True)
    dst.import_rows(0, *rows)
    ptr, size, maxp = src.state()
    dst.set_state(ptr, size, maxp)
    assert dst.state() == src.state()
    for a, b in zip(dst.export_rows(0, n, priority=True), rows):
        np.testing.assert_array_equal(a, b)
    rng = np.random.default_rng(0)
    ind = np.concatenate([rng.integers(0, n, 256), [0, n - 1]])
    for rep in (src, dst):
        for g, full in zip(rep.gather(ind), rows[:5]):
            np.testing.assert_array_equal(g, full[ind])
    # an import into the middle of the ring leaves its neighbours alone
    part = [np.ascontiguousarray(x[100:103]) for x in rows]
    dst.import_rows(2000, *part)
    after = dst.export_rows(1999, 5, priority=True)
    for a, full, p in zip(after, rows, part):
        np.testing.assert_array_equal(a[0], full[1999])
        np.testing.assert_array_equal(a[1:4], p)
        np.testing.assert_array_equal(a[4], full[2003])


# ---- 4. LAP sums after import ----------------------------------------------------------------------------

def _td7(seed=5, **kw):
    return TD7("Tiny-v0", use_lap=True, hidden=32, batch_size=32, seed=seed, target_update_rate=4, **kw)


def _uniforms():
    u = np.random.default_rng(2).random(1024).astype(np.float32)
    u[0], u[1] = 0.0, np.nextafter(np.float32(1), np.float32(0), dtype=np.float32)
    return u


def test_lap_sums_after_import_and_deepcopy():
    B = 32
    ag = _td7()
    rep = _fill(LAPReplayMemory(4200, "Tiny-v0"), 4150, 4)
    run_train_ops(rep, ag, B, n_ops=9)
    sd = rep.state_dict()
    pri = sd["priority"]
    assert len(np.unique(pri)) > 50 and pri.min() >= 1.0  # the priorities are no longer trivial
    assert sd["ind"].shape == (B,)
    u = _uniforms()
    want = OR.lap_indices(pri, 4150, u)
    assert (want >= 4096).any() and (want < 4096).any()  # both blocks are drawn from
    ind = rep.dev.sample_indices(u)
    np.testing.assert_array_equal(ind, want)
    restored = LAPReplayMemory(4200, "Tiny-v0").load_state_dict(sd)
    twin = copy.deepcopy(rep)
    for other in (restored, twin):
        assert type(other) is LAPReplayMemory and other.dev.h.value != rep.dev.h.value
        np.testing.assert_array_equal(other.dev.sample_indices(u), ind)
        assert np.float32(other.max_priority) == np.float32(rep.max_priority)
        assert (other.ptr, other.size) == (rep.ptr, rep.size) == (4150, 4150)
        np.testing.assert_array_equal(other.ind, sd["ind"])
        _assert_sd_equal(other.state_dict(), sd)
    # the copy is its own ring: writes to it do not reach the source
    twin.update_priority(torch.full((B,), 50.0))
    twin.append([np.ones(S), np.zeros(A), 1.0, np.ones(S), 1.0])
    assert twin.size == 4151 and twin.max_priority == 50.0
    _assert_sd_equal(rep.state_dict(), sd)
    np.testing.assert_array_equal(rep.dev.sample_indices(u), ind)
    tp = twin.priority.numpy()
    np.testing.assert_array_equal(tp[sd["ind"]], 50.0)
    np.testing.assert_array_equal(twin.dev.sample_indices(u), OR.lap_indices(tp, 4151, u))


def test_load_state_dict_rejects_another_shape():
    rep = _fill(LAPReplayMemory(64, "Tiny-v0"), 10, 1)
    sd = rep.state_dict()
    with pytest.raises(ValueError, match="capacity"):
        LAPReplayMemory(65, "Tiny-v0").load_state_dict(sd)
    with pytest.raises(ValueError, match="lap"):
        SimpleReplayMemory(64, "Tiny-v0").load_state_dict(sd)
    with pytest.raises(ValueError, match="state_dim"):
        LAPReplayMemory(64, state_dim=S + 1, action_dim=A).load_state_dict(sd)
    with pytest.raises(ValueError, match="action_dim"):
        LAPReplayMemory(64, state_dim=S, action_dim=A + 1).load_state_dict(sd)
    with pytest.raises(ValueError, match="reward"):
        LAPReplayMemory(64, "Tiny-v0").load_state_dict(dict(sd, reward=sd["reward"][:9]))


# ---- 5. bitwise resume -----------------------------------------------------------------------------------

B = 32


def _fresh_run():
    return _td7(seed=9), _fill(LAPReplayMemory(512, "Tiny-v0"), 300, 6)


def _explicit_steps(ag, rep, t0, n):
    infos, inds = [], []
    for t in range(t0, t0 + n):
        torch.manual_seed(2000 + t)
        batch = rep.sample(B)
        inds.append(np.array(batch.ind))
        infos.append(ag.train_ops(batch, rep))
    return infos, inds


def _fused_steps(ag, rep, t0, n):
    infos = run_train_ops(rep, ag, B, n_ops=n)
    return infos, [np.array(rep.ind)]


def _final_state(ag, rep):
    return ag.state_dict(), rep.priority.numpy().copy(), (np.float32(rep.max_priority), rep.ptr, rep.size)


def _assert_same_run(got, ref):
    (infos, inds, (params, pri, scal)), (rinfos, rinds, (rparams, rpri, rscal)) = got, ref
    assert infos == rinfos
    assert len(inds) == len(rinds)
    for a, b in zip(inds, rinds):
        np.testing.assert_array_equal(a, b)
    for net, d in rparams.items():
        for name, v in d.items():
            np.testing.assert_array_equal(params[net][name], v, err_msg=f"{net}.{name}")
    np.testing.assert_array_equal(pri, rpri)
    assert scal == rscal


def _via_disk(ag, rep, tmp_path):
    ag.save(tmp_path / "agent.pkl")
    rep.save(tmp_path / "replay")
    return lambda: (TD7.load(tmp_path / "agent.pkl"), LAPReplayMemory.load(tmp_path / "replay"))


def _via_pickle(ag, rep, tmp_path):
    blob = pickle.dumps((ag, rep))
    return lambda: pickle.loads(blob)


def _resume(steps, how, tmp_path):
    ag, rep = _fresh_run()
    steps(ag, rep, 0, 7)
    restore = how(ag, rep, tmp_path)
    del ag, rep
    ag, rep = restore()
    infos, inds = steps(ag, rep, 7, 6)
    return infos, inds, _final_state(ag, rep)


def _uninterrupted(steps):
    ag, rep = _fresh_run()
    steps(ag, rep, 0, 7)
    infos, inds = steps(ag, rep, 7, 6)
    return infos, inds, _final_state(ag, rep)


@pytest.fixture(scope="module")
def explicit_reference():
    return _uninterrupted(_explicit_steps)


@pytest.mark.parametrize("how", [_via_disk, _via_pickle])
def test_restored_run_continues_bit_for_bit(how, tmp_path, explicit_reference):
    """replay.sample(B) + agent.train_ops(batch, replay): 7 steps, save both, drop both, load both, 6 steps
    == 13 steps in one go (infos, sampled indices, every parameter, the priorities, max_priority, ptr, size)."""
    ref = explicit_reference
    assert len(ref[0]) == 6 and len({tuple(i) for i in ref[1]}) == 6
    _assert_same_run(_resume(_explicit_steps, how, tmp_path), ref)


@pytest.fixture(scope="module")
def fused_reference():
    return _uninterrupted(_fused_steps)


@pytest.mark.parametrize("how", [_via_disk, _via_pickle])
def test_restored_run_continues_bit_for_bit_in_the_fused_loop(how, tmp_path, fused_reference):
    """The same through run_train_ops(n_ops=7) then (n_ops=6): the restored engine draws its first batch
    from the saved Philox position, as the original redraws nothing it had not already drawn there."""
    _assert_same_run(_resume(_fused_steps, how, tmp_path), fused_reference)


# ---- 6. bound engines see an import ----------------------------------------------------------------------

def test_bound_engine_redraws_its_prefetched_batch_after_an_import():
    ag, rep = _fresh_run()
    other_sd = _fill(LAPReplayMemory(512, "Tiny-v0"), 280, 77).state_dict()
    ag.train_n(rep, B, 3)  # (leaves a batch prefetched from the old contents)
    ag2 = copy.deepcopy(ag)
    rep.load_state_dict(other_sd)
    info = ag.train_n(rep, B, 1)
    ind = np.array(rep.ind)
    rep2 = LAPReplayMemory(512, "Tiny-v0").load_state_dict(other_sd)
    info2 = ag2.train_n(rep2, B, 1)
    np.testing.assert_array_equal(ind, rep2.ind)
    assert ind.max() < 280
    assert info == info2
    # (rows at or past size are not part of a state: the import leaves what the ring held there)
    np.testing.assert_array_equal(rep.priority.numpy()[:280], rep2.priority.numpy()[:280])


# ---- 7. to -----------------------------------------------------------------------------------------------

def test_to_the_current_device_is_a_no_op():
    rep = _fill(LAPReplayMemory(64, "Tiny-v0"), 40, 1)
    h = rep.dev.h.value
    for spelling in (0, "cuda:0", "cuda", "hip:0", "cpu"):
        assert rep.to(spelling) is rep
    assert rep.dev.h.value == h and rep.device == 0
    with pytest.raises(ValueError):
        rep.to("tpu:0")


def test_to_another_gpu_moves_the_ring():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    ag, rep = _fresh_run()
    run_train_ops(rep, ag, B, n_ops=3)
    sd = rep.state_dict()
    assert rep.to("cuda:1") is rep and rep.device == 1
    sd1 = rep.state_dict()
    _assert_sd_equal(sd1, sd)
    with pytest.raises(ValueError, match="replay on device 1"):
        ag.train_ops(rep.sample(B), rep)
    ag.to("cuda:1")
    infos = run_train_ops(rep, ag, B, n_ops=2)
    assert len(infos) == 2 and all(np.isfinite(v) for i in infos for v in i.values() if v is not None)
    twin = copy.deepcopy(rep)
    assert twin.device == 1
    _assert_sd_equal(twin.state_dict(), rep.state_dict())
    rep.to(0)
    _assert_sd_equal(twin.state_dict(), rep.state_dict())
