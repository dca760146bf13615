"""n-step returns on the host: the law of include/rle.h as tests/n_step_ref.py states it, the fixture rings of
tests/n_step_cases.py, the new ABI entries and the mirror's checks.  No GPU."""

import copy
import ctypes
import pickle

import numpy as np
import pytest

import n_step_cases as C
import n_step_ref as R

S, A = 5, 3


def _all(ring):
    return np.arange(ring["size"], dtype=np.int64)


# ---- the law --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", C.KINDS)
def test_n_1_is_the_identity(kind):
    r = C.ring(kind, S, A)
    ind = _all(r)
    Rn, s2, nd, hops, why = R.n_step(r, ind, 1, C.GAMMA, causes=True)
    assert Rn.tobytes() == r["reward"][ind].tobytes()
    assert s2.tobytes() == r["next_state"][ind].tobytes()
    assert nd.tobytes() == r["notdone"][ind].tobytes()
    assert (hops == 1).all() and set(why) == {"n"}


def _hand_ring():
    """8 slots, S = 2: slots 0-2 one episode that terminates, 3-4 one cut by the data alone, 5-7 one in progress;
    rewards 1, 2, 4, ... so every return is a readable sum."""
    st = np.array([[0, 0], [1, 1], [2, 2], [9, 9], [10, 10], [20, 20], [21, 21], [22, 22]], np.float32)
    nx = np.array([[1, 1], [2, 2], [3, 3], [10, 10], [11, 11], [21, 21], [22, 22], [23, 23]], np.float32)
    return dict(state=st, next_state=nx, reward=np.array([1, 2, 4, 8, 16, 32, 64, 128], np.float32),
                notdone=np.array([1, 1, 0, 1, 1, 1, 1, 1], np.float32), ptr=0, size=8)


def test_closed_forms_on_a_hand_written_ring():
    r, g = _hand_ring(), np.float32(0.5)
    one = lambda i, n: R.n_step_one(r, i, n, g)  # noqa: E731
    # slot 0, n = 3: 1 + 0.5 * 2 + 0.25 * 4, ends on the terminal row: notdone 0
    assert one(0, 3) == (np.float32(3.0), 2, np.float32(0.0), 3, "n")
    # n = 8 from slot 0 stops at the terminal row all the same
    assert one(0, 8) == (np.float32(3.0), 2, np.float32(0.0), 3, "terminated")
    # slot 1, n = 2: 2 + 0.5 * 4; slot 2 is terminal: one hop, its own reward
    assert one(1, 2) == (np.float32(4.0), 2, np.float32(0.0), 2, "n")
    assert one(2, 5) == (np.float32(4.0), 2, np.float32(0.0), 1, "terminated")
    # slots 3-4: 8 + 0.5 * 16, then next_state [11, 11] != state [20, 20]: cut, notdone stays 1, g = 0.5
    assert one(3, 4) == (np.float32(16.0), 4, np.float32(0.5), 2, "cut")
    # slots 5-7 then the ring's end: slot 0 is ptr (the oldest row), the newest row is slot 7
    assert one(5, 8) == (np.float32(32 + 32 + 32), 7, np.float32(0.25), 3, "ptr")
    # the same ring with 6 rows filled: slot 5 is the newest
    r6 = dict(r, ptr=6, size=6)
    assert R.n_step_one(r6, 5, 3, g) == (np.float32(32.0), 5, np.float32(1.0), 1, "size")
    # a full ring whose ptr is slot 6: the walk from 5 stops there although slot 6 continues it
    r_mid = dict(r, ptr=6)
    assert R.n_step_one(r_mid, 5, 3, g) == (np.float32(32.0), 5, np.float32(1.0), 1, "ptr")
    # across the ring's end: slots 7 -> 0 when the data goes on and ptr is elsewhere
    r_wrap = dict(r, ptr=4)
    r_wrap["state"] = r["state"].copy()
    r_wrap["state"][0] = r["next_state"][7]
    assert R.n_step_one(r_wrap, 7, 2, g) == (np.float32(128 + 0.5), 0, np.float32(0.5), 2, "n")
    # -0.0 and 0.0 differ as bit patterns
    r_zero = dict(r, state=r["state"].copy(), next_state=r["next_state"].copy())
    r_zero["next_state"][5] = [0.0, 0.0]
    r_zero["state"][6] = [-0.0, 0.0]
    assert R.n_step_one(r_zero, 5, 2, g)[3:] == (1, "cut")


def test_products_round_once_each():
    """g is the running float32 product and R the running float32 sum, in the law's order."""
    r = C.ring("mid", S, A)
    i = 18  # (the nine-row episode's first row)
    Rn, cur, nd, hops, _ = R.n_step_one(r, i, 5, C.GAMMA)
    g, acc = np.float32(1), np.float32(r["reward"][i])
    for k in range(1, 5):
        g = np.float32(g * np.float32(C.GAMMA))
        acc = np.float32(acc + np.float32(g * r["reward"][i + k]))
    assert (hops, cur) == (5, i + 4) and Rn.tobytes() == acc.tobytes() and nd.tobytes() == g.tobytes()


# ---- the fixtures are not vacuous -----------------------------------------------------------------------------

@pytest.mark.parametrize("S_", [5, 130])
def test_fixture_rings_cover_every_hop_count_and_stop_cause(S_):
    seen = set()
    for kind in C.KINDS:
        r = C.ring(kind, S_, A)
        assert r["state"].dtype == np.float32 and r["state"].shape == (C.CAP, S_)
        for n in C.N_TESTED[1:]:
            _, _, _, hops, why = R.n_step(r, _all(r), n, C.GAMMA, causes=True)
            assert set(hops.tolist()) == set(range(1, n + 1)), (kind, n)
            seen |= set(why)
    assert seen == set(R.CAUSES)


def test_each_ring_situation_is_decided_by_its_own_check():
    part, mid, wrap = (C.ring(k, S, A) for k in C.KINDS)
    # part: slot 45 holds a stale row that continues slot 44; only size stops the walk
    assert part["size"] == part["ptr"] == 45 < C.CAP
    assert part["next_state"][44].tobytes() == part["state"][45].tobytes() and part["notdone"][44] == 1
    assert R.n_step_one(part, 44, 2, C.GAMMA)[3:] == (1, "size")
    assert R.n_step_one(dict(part, size=C.CAP, ptr=0), 44, 2, C.GAMMA)[3] == 2
    # mid: slot 33 = ptr continues slot 32 in the data; only ptr stops the walk
    assert mid["next_state"][32].tobytes() == mid["state"][33].tobytes() and mid["notdone"][32] == 1
    assert R.n_step_one(mid, 32, 2, C.GAMMA)[3:] == (1, "ptr")
    assert R.n_step_one(dict(mid, ptr=0), 32, 2, C.GAMMA)[3] == 2
    # wrap: an episode runs across slots 63 -> 0
    assert R.n_step_one(wrap, 62, 4, C.GAMMA)[1:4:2] == (1, 4)
    # sticky: the next episode starts from the terminal row's next_state; only notdone stops the walk
    ends = np.cumsum([n for n, _ in C.EPISODES])
    k = [e for _, e in C.EPISODES].index("sticky")
    last = int(ends[k]) - 1
    assert mid["next_state"][last].tobytes() == mid["state"][last + 1].tobytes() and mid["notdone"][last] == 0
    assert R.n_step_one(mid, last, 3, C.GAMMA)[3:] == (1, "terminated")
    # trunc: notdone 1, the data alone cuts
    k = [e for _, e in C.EPISODES].index("trunc")
    last = int(ends[k]) - 1
    assert mid["notdone"][last] == 1 and R.n_step_one(mid, last, 3, C.GAMMA)[3:] == (1, "cut")


# ---- the ABI --------------------------------------------------------------------------------------------------

def test_new_entries_are_declared_and_exported():
    from rl import _engine as E

    vp, f32p, i64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_longlong)
    i32p = ctypes.POINTER(ctypes.c_int)
    assert E.SIGNATURES["rle_set_n_step"] == (ctypes.c_int, [vp, ctypes.c_int])
    assert E.SIGNATURES["rle_get_n_step"] == (ctypes.c_int, [vp, i32p])
    assert E.SIGNATURES["rle_replay_gather_nstep"] == (
        ctypes.c_int, [vp, ctypes.c_int, i64p, ctypes.c_int, ctypes.c_float, f32p, f32p, f32p, f32p, f32p, i32p])
    lib = E.lib()
    for name in ("rle_set_n_step", "rle_get_n_step", "rle_replay_gather_nstep"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == E.SIGNATURES[name][1]
    n = ctypes.c_int(0)
    assert lib.rle_set_n_step(None, 3) == -1  # (null handles are refused before any HIP call)
    assert lib.rle_get_n_step(None, ctypes.byref(n)) == -1
    assert lib.rle_replay_gather_nstep(None, 0, None, 3, 0.99, None, None, None, None, None, None) == -1
    hdr = open(E.__file__.rsplit("/sac-td3-td7_amd/", 1)[0] + "/include/rle.h").read()
    for decl in ("#define RLE_MAX_N_STEP 8", "int rle_set_n_step(rle_engine* e, int n);",
                 "int rle_get_n_step(rle_engine* e, int* n);",
                 "int rle_replay_gather_nstep(rle_replay* r, int n, const long long* ind, int n_step, float discount, "
                 "float* state,"):
        assert decl in hdr, decl
    assert "false positive" in hdr and E.MAX_N_STEP == 8


# ---- the mirror's checks, without a device ----------------------------------------------------------------------

def test_check_n_step_refuses_what_the_engine_refuses():
    from rl import _engine as E

    for alg in (E.RLE_TD3, E.RLE_SAC):
        assert [E.check_n_step(alg, n) for n in (1, 2, 8)] == [1, 2, 8]
        for bad in (0, 9, -1, 2.5, True):
            with pytest.raises(ValueError, match="n_step"):
                E.check_n_step(alg, bad)
    assert E.check_n_step(E.RLE_TD7, 1) == 1
    with pytest.raises(ValueError, match="one-step model"):
        E.check_n_step(E.RLE_TD7, 2)


class _FakeEngine:
    made = []

    def __init__(self, cfg, plan=None, ext=None):
        self.cfg, self.ext, self.replay, self.n = cfg, ext, None, 1
        _FakeEngine.made.append(self)

    def set_grad_clip(self, max_norm):
        pass

    def set_layer_norm(self, critic=True):
        pass

    def set_n_step(self, n):
        self.n = n

    def copy_state_from(self, other):
        pass

    def close(self):
        pass


@pytest.fixture
def classes(monkeypatch):
    from rl import _engine as E
    from rl.agent import SAC, TD3, TD7
    from rl.agent.engine_agent import EngineAgent
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    _FakeEngine.made.clear()
    monkeypatch.setattr(E, "Engine", _FakeEngine)
    monkeypatch.setattr(EngineAgent, "_import", lambda self, st: None)
    monkeypatch.setattr(EngineAgent, "_export", lambda self, *a, **k: {"params": {}})
    return {"td7": TD7, "td3": TD3, "sac": SAC}


KW = dict(hidden=32, batch_size=16, seed=1)


@pytest.mark.parametrize("alg", ["td3", "sac"])
def test_keyword_reaches_every_engine_the_agent_builds(classes, alg):
    cls = classes[alg]
    ag = cls("Tiny-v0", n_step=3, **KW)
    assert ag.n_step == 3 and ag.engine.n == 3 and ag._info_keys()[-1] == "replay/hops"
    ag2, ag3 = pickle.loads(pickle.dumps(ag)), copy.deepcopy(ag)
    ag._rebuild(48)
    for a in (ag, ag2, ag3):
        assert a.n_step == 3 and a.engine.n == 3
    plain = cls("Tiny-v0", **KW)
    assert plain.n_step == 1 and plain.engine.n == 1 and "n_step" not in plain.__dict__
    assert "n_step" not in plain.__getstate__() and "replay/hops" not in plain._info_keys()
    assert ag._info_keys()[:-1] == plain._info_keys()
    for bad in (0, 9):
        with pytest.raises(ValueError, match="n_step"):
            cls("Tiny-v0", n_step=bad, **KW)
    with pytest.raises(ValueError, match="no episode order"):
        ag.train_ops({"state": 0, "action": 0, "reward": np.zeros(4), "next_state": 0, "done": 0})


def test_td7_refuses_more_than_one_step(classes):
    TD7 = classes["td7"]
    n = len(_FakeEngine.made)
    with pytest.raises(ValueError, match="one-step model"):
        TD7("Tiny-v0", n_step=2, **KW)
    assert len(_FakeEngine.made) == n
    assert TD7("Tiny-v0", n_step=1, **KW).engine.n == 1
