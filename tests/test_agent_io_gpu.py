"""Agent snapshots in one device pass: rle_state_toc / _export / _import, rle_copy_nets, rle_copy_state and
the Python agents on top of them.  The per-tensor entries (rle_get_param / rle_get_adam / rle_set_*) are the
yardstick: the packed state equals what they read, bit for bit, and an engine filled through the blob
computes what an engine filled tensor by tensor computes."""

import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from rl import _engine as E
from rl.agent import SAC, TD7
from rl.replay_memory import LAPReplayMemory, SimpleReplayMemory
from rl.utils import register_env

pytestmark = pytest.mark.gpu

register_env("Tiny-v0", 11, 3, -0.5, 0.5)

# Shapes that reach every corner of the layout (S 11, A 3 unless given):
#   td7_tiny:     outputs 3 and 1 (no multiple of 16), segments 11 / 3 / 48 padded, q1 with three segments
#   td3_36_20:    a K and an out that are multiples of 4 but not of 16
#   sac:          the 2A head and log_alpha
#   td7_humanoid: more than one block row and block column in every layer, unaligned 393-float rows
CASES = {
    "td7_tiny": dict(algo=E.RLE_TD7, state_dim=11, action_dim=3, hidden=32, zs_dim=48),
    "td3_36_20": dict(algo=E.RLE_TD3, state_dim=11, action_dim=3, hidden=20, hidden_sizes=[36, 20]),
    "sac": dict(algo=E.RLE_SAC, state_dim=11, action_dim=3, hidden=32),
    "td7_humanoid": dict(algo=E.RLE_TD7, state_dim=376, action_dim=17, hidden=256),
}


def _engine(case, batch=32, seed=3, device=0):
    # (td3_36_20: the step's fused loss head reads q-dot partials, which need a last hidden width that is a
    # multiple of 16; the plan switches that fusion off, the parameter layout under test is the same)
    plan = E.make_plan(fuse_off=("qdot", "headdx")) if case == "td3_36_20" else None
    return E.Engine(E.make_config(batch=batch, seed=seed, device=device, **CASES[case]), plan)


def _replay(case, cap=256):
    c = CASES[case]
    rep = E.Replay(cap, c["state_dim"], c["action_dim"], False)
    rep.fill_random(cap, 5)
    return rep


def _random_state(eng, seed, scale=0.1):
    """{(arena, net, name): flat fp32 array} for every tensor of the full TOC (v >= 0)."""
    rng = np.random.default_rng(seed)
    out = {}
    for net, name, arena, _, n in eng.state_toc(E.STATE_ALL):
        x = (rng.standard_normal(n) * scale).astype(np.float32)
        out[arena, net, name] = np.abs(x) if arena == 2 else x
    return out


def _set_per_tensor(eng, arrays):
    for (arena, net, name), x in arrays.items():
        if arena == 0:
            eng.set_param(net, name, x)
        else:
            eng.set_adam(net, name, arena - 1, x)


def _get_per_tensor(eng, arena, net, name):
    return eng.get_param(net, name) if arena == 0 else eng.get_adam(net, name, arena - 1)


def _assert_blob_equals_per_tensor(blob, toc, eng):
    for net, name, arena, off, n in toc:
        ref = _get_per_tensor(eng, arena, net, name)
        assert ref.size == n, (net, name)
        np.testing.assert_array_equal(blob[off:off + n].view(np.uint32), ref.view(np.uint32),
                                      err_msg=f"arena {arena} {net}.{name}")


def _trained(case, steps=3, batch=32, seed=3, init_seed=1):
    eng, rep = _engine(case, batch, seed), _replay(case)
    _set_per_tensor(eng, {k: v for k, v in _random_state(eng, init_seed).items() if k[0] == 0})
    eng.bind(rep)
    if steps:
        eng.step(steps)
    return eng, rep


# ---- 1. the table of contents and the export ---------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_export_equals_the_per_tensor_reads(case):
    eng, _rep = _trained(case)
    toc = eng.state_toc(E.STATE_ALL)
    # arenas in mask order, entries contiguous, weight before bias, SAC's log_alpha last in each arena
    assert [t[2] for t in toc] == sorted(t[2] for t in toc)
    assert toc[0][3] == 0 and all(a[3] + a[4] == b[3] for a, b in zip(toc, toc[1:]))
    per_arena = [[t for t in toc if t[2] == k] for k in range(3)]
    optim = {"policy", "q1", "q2", "encoder", "tmp"}
    assert [t[:2] for t in per_arena[1]] == [t[:2] for t in per_arena[2]] == \
        [t[:2] for t in per_arena[0] if t[0] in optim]
    for ar in per_arena:
        body = ar[:-1] if case == "sac" else ar
        assert [t[1].rsplit(".", 1)[1] for t in body] == ["weight", "bias"] * (len(body) // 2)
        assert (ar[-1][:2] == ("tmp", "log_alpha") and ar[-1][4] == 1) == (case == "sac")
    if case == "td7_humanoid":
        # 3 encoders x 6 layers, the actor's 4, 4 critics x 4: 38 layers; 18 of them have an optimiser
        assert len(per_arena[0]) == 76 and len(per_arena[1]) == 36
        assert any(t[:2] == ("q1", "q01.weight") and t[4] == 256 * 393 for t in toc)
    blob = eng.state_export(E.STATE_ALL)
    assert blob.dtype == np.float32 and blob.size == toc[-1][3] + toc[-1][4]
    assert np.any(blob[per_arena[1][0][3]:] != 0)  # (the moments moved in the 3 steps)
    _assert_blob_equals_per_tensor(blob, toc, eng)
    for what in (E.STATE_PARAMS, E.STATE_ADAM_V, E.STATE_PARAMS | E.STATE_ADAM_V):
        part, ptoc = eng.state_export(what), eng.state_toc(what)
        assert {t[2] for t in ptoc} == {k for k in range(3) if what >> k & 1}
        _assert_blob_equals_per_tensor(part, ptoc, eng)


# ---- 2. the import, through the images only a forward sees ---------------------------------------------------

@pytest.mark.parametrize("case", list(CASES))
def test_import_equals_the_per_tensor_writes(case):
    c = CASES[case]
    S, A = c["state_dim"], c["action_dim"]
    td7 = c["algo"] == E.RLE_TD7
    x, rep = _trained(case)  # (its arenas hold other values: stale padding would show)
    y = _engine(case)
    y.bind(rep)
    arrays = _random_state(y, 7)
    toc = x.state_toc(E.STATE_ALL)
    blob = np.concatenate([arrays[arena, net, name] for net, name, arena, _, _ in toc])
    x.state_import(blob, E.STATE_ALL)
    _set_per_tensor(y, arrays)
    x.set_counters(y.counters())
    x.set_value_bounds(y.value_bounds())
    rng = np.random.default_rng(2)
    obs = rng.standard_normal((20, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (20, A)).astype(np.float32)
    width = 2 * A if c["algo"] == E.RLE_SAC else A

    def bits(v):
        return np.ascontiguousarray(v).view(np.uint32)

    np.testing.assert_array_equal(bits(x.act(obs, width)), bits(y.act(obs, width)))
    for q, enc in (("q1", "fixed_encoder"), ("q2", "fixed_encoder"), ("target_q1", "fixed_encoder_target")):
        np.testing.assert_array_equal(bits(x.eval_q(q, obs, act, enc)), bits(y.eval_q(q, obs, act, enc)), err_msg=q)
    if td7:
        for enc in ("encoder", "fixed_encoder", "fixed_encoder_target"):
            np.testing.assert_array_equal(bits(x.eval_zs(enc, obs)), bits(y.eval_zs(enc, obs)), err_msg=enc)
            np.testing.assert_array_equal(bits(x.eval_zsa(enc, obs, act)), bits(y.eval_zsa(enc, obs, act)), err_msg=enc)
    ind = rng.integers(0, 256, (4, 32))
    rows = []
    for eng in (x, y):
        eng.set_tapes(ind=ind)
        rows.append(eng.step(4).copy())
        eng.set_tapes()
    assert np.isfinite(rows[1]).any() and np.any(rows[1] != 0)
    np.testing.assert_array_equal(bits(rows[0]), bits(rows[1]))
    for net, name, arena, _, _ in toc:
        np.testing.assert_array_equal(bits(_get_per_tensor(x, arena, net, name)),
                                      bits(_get_per_tensor(y, arena, net, name)), err_msg=f"arena {arena} {net}.{name}")


def test_import_of_one_arena_leaves_the_others():
    x, _rep = _trained("td7_tiny")
    before = x.state_export(E.STATE_ALL)
    toc = x.state_toc(E.STATE_ALL)
    m = np.arange(x.state_size(E.STATE_ADAM_M), dtype=np.float32)
    x.state_import(m, E.STATE_ADAM_M)
    after = x.state_export(E.STATE_ALL)
    for net, name, arena, off, n in toc:
        if arena != 1:
            np.testing.assert_array_equal(after[off:off + n], before[off:off + n], err_msg=f"{arena} {net}.{name}")
    np.testing.assert_array_equal(x.state_export(E.STATE_ADAM_M), m)
    _assert_blob_equals_per_tensor(after, toc, x)


# ---- 3. drain ---------------------------------------------------------------------------------------------------

def test_export_waits_for_enqueued_steps():
    a, _ra = _trained("td7_tiny", steps=0)
    b, _rb = _trained("td7_tiny", steps=0)
    a.step_async(5)
    blob = a.state_export(E.STATE_ALL)  # (at once: the export drains the burst itself)
    b.step(5)
    _assert_blob_equals_per_tensor(blob, b.state_toc(E.STATE_ALL), b)


# ---- 4. rle_copy_nets -------------------------------------------------------------------------------------------

def _copy_nets_check(case, dst_device=0):
    src, _rs = _trained(case, steps=3, batch=32, init_seed=1)
    dst = _engine(case, batch=64, seed=4, device=dst_device)
    c = CASES[case]
    rep = E.Replay(256, c["state_dim"], c["action_dim"], False, dst_device)
    rep.fill_random(256, 6)
    _set_per_tensor(dst, {k: v for k, v in _random_state(dst, 8).items() if k[0] == 0})
    dst.bind(rep)
    dst.step(2)
    moments = dst.state_export(E.STATE_ADAM_M | E.STATE_ADAM_V)
    counters, bounds, act_counter = dst.counters(), dst.value_bounds(), dst.act_counter()
    log_alpha = dst.get_param("tmp", "log_alpha") if case == "sac" else None
    dst.copy_nets_from(src)
    got, ref, toc = dst.state_export(E.STATE_PARAMS), src.state_export(E.STATE_PARAMS), src.state_toc(E.STATE_PARAMS)
    for net, name, _, off, n in toc:
        if net != "tmp":
            np.testing.assert_array_equal(got[off:off + n].view(np.uint32), ref[off:off + n].view(np.uint32),
                                          err_msg=f"{net}.{name}")
    _assert_blob_equals_per_tensor(got, toc, dst)
    np.testing.assert_array_equal(dst.state_export(E.STATE_ADAM_M | E.STATE_ADAM_V), moments)
    np.testing.assert_array_equal(dst.counters(), counters)
    np.testing.assert_array_equal(dst.value_bounds(), bounds)
    assert dst.act_counter() == act_counter
    if case == "sac":
        np.testing.assert_array_equal(dst.get_param("tmp", "log_alpha"), log_alpha)
        assert src.get_param("tmp", "log_alpha")[0] != log_alpha[0]
    obs = np.random.default_rng(3).standard_normal((9, c["state_dim"])).astype(np.float32)
    width = 2 * c["action_dim"] if case == "sac" else c["action_dim"]
    np.testing.assert_array_equal(dst.act(obs, width), src.act(obs, width))  # (the N images came along)
    assert np.isfinite(dst.step(2)).any()  # (and it trains on)


@pytest.mark.parametrize("case", ["td7_tiny", "sac"])
def test_copy_nets_copies_the_networks_and_nothing_else(case):
    _copy_nets_check(case)


def test_copy_nets_rejects_other_shapes_and_algorithms():
    lib = E.lib()
    a = E.Engine(E.make_config(E.RLE_TD3, 11, 3, 32, 32))
    wide = E.Engine(E.make_config(E.RLE_TD3, 11, 3, 64, 32))
    sac = E.Engine(E.make_config(E.RLE_SAC, 11, 3, 32, 32))
    swapped = [E.Engine(E.make_config(E.RLE_TD3, 11, 3, h[-1], 32, hidden_sizes=h)) for h in ([36, 20], [20, 36])]
    for dst, src in ((a, wide), (wide, a), (a, sac), (sac, a), swapped, swapped[::-1]):
        assert lib.rle_copy_nets(dst.h, src.h) == -1
        assert b"copy_nets" in lib.rle_last_error()
        assert lib.rle_copy_state(dst.h, src.h) == -1
    assert lib.rle_copy_nets(a.h, a.h) == 0


def test_copy_nets_to_another_gpu():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    _copy_nets_check("td7_tiny", dst_device=1)


# ---- 5. the Python agents ---------------------------------------------------------------------------------------

B = 32


def _agent(alg, seed=9, batch=B):
    if alg == "td7":
        return TD7("Tiny-v0", use_lap=True, target_update_rate=4, hidden=32, batch_size=batch, seed=seed)
    return SAC("Tiny-v0", hidden=32, batch_size=batch, seed=seed)


def _agent_replay(alg):
    rng = np.random.default_rng(6)
    rep = (LAPReplayMemory if alg == "td7" else SimpleReplayMemory)(512, "Tiny-v0")
    rep.append_batch(rng.standard_normal((300, 11)), rng.uniform(-0.5, 0.5, (300, 3)), rng.standard_normal(300),
                     rng.standard_normal((300, 11)), (rng.random(300) > 0.1).astype(np.float64))
    return rep


def _assert_same_params(a, b):
    assert list(a) == list(b)
    for net in a:
        assert list(a[net]) == list(b[net])
        for name, v in a[net].items():
            np.testing.assert_array_equal(np.asarray(v).view(np.uint32), np.asarray(b[net][name]).view(np.uint32),
                                          err_msg=f"{net}.{name}")


@pytest.fixture(scope="module", params=["td7", "sac"])
def twin(request):
    """An uninterrupted run: 3 + 5 fused steps (TD7: hard updates at steps 4 and 8)."""
    alg = request.param
    ag, rep = _agent(alg), _agent_replay(alg)
    ag.train_n(rep, B, 3)
    infos = ag.train_n(rep, B, 5)
    return alg, infos, ag._export()


def _deepcopy(ag):
    return copy.deepcopy(ag)


def _pickle(ag):
    return pickle.loads(pickle.dumps(ag))


def _rebuild(ag):
    ag._rebuild()  # (what another replay, or replay.to(), triggers)
    return ag


@pytest.mark.parametrize("how", [_deepcopy, _pickle, _rebuild])
def test_copied_agent_continues_bit_for_bit(how, twin):
    alg, ref_infos, ref_state = twin
    ag, rep = _agent(alg), _agent_replay(alg)
    ag.train_n(rep, B, 3)
    ag2 = how(ag)
    assert type(ag2) is type(ag) and ag2.batch_size == B and ag2.n_runs == 3
    infos = ag2.train_n(rep, B, 5)
    assert infos == ref_infos
    st = ag2._export()
    _assert_same_params(st["params"], ref_state["params"])
    assert list(st["adam"]) == list(ref_state["adam"])
    for net, d in st["adam"].items():
        for name, (m, v) in d.items():
            np.testing.assert_array_equal(m, ref_state["adam"][net][name][0], err_msg=f"m {net}.{name}")
            np.testing.assert_array_equal(v, ref_state["adam"][net][name][1], err_msg=f"v {net}.{name}")
    np.testing.assert_array_equal(st["counters"], ref_state["counters"])
    np.testing.assert_array_equal(st["vbounds"], ref_state["vbounds"])


@pytest.mark.parametrize("alg", ["td7", "sac"])
def test_batch_size_rebuild_equals_the_host_route(alg):
    """32 -> 16 rows through train_n (a new engine filled by rle_copy_state) against the same agent rebuilt the
    way it was before: a full export, a fresh engine, a full import."""
    ag, rep = _agent(alg), _agent_replay(alg)
    ref, rref = _agent(alg), _agent_replay(alg)
    ag.train_n(rep, B, 3)
    ref.train_n(rref, B, 3)
    st = ref._export()
    ref.engine.close()
    ref.engine = ref._new_engine(16)
    ref._import(st)
    ref._replay = None
    assert ag.train_n(rep, 16, 5) == ref.train_n(rref, 16, 5)
    assert ag.batch_size == 16
    _assert_same_params(ag.state_dict(), ref.state_dict())


def test_rebuild_does_not_repeat_the_exploration_draw():
    obs = np.random.default_rng(1).standard_normal(11).astype(np.float32)
    ag, ref = _agent("td7"), _agent("td7")
    y1, y2 = ref.sample(obs).copy(), ref.sample(obs).copy()
    x1 = ag.sample(obs).copy()
    ag._rebuild()
    x2 = ag.sample(obs).copy()
    assert not np.array_equal(x1, x2)
    np.testing.assert_array_equal(x1, y1)
    np.testing.assert_array_equal(x2, y2)
    np.testing.assert_array_equal(copy.deepcopy(ag).sample(obs), ref.sample(obs))


@pytest.mark.parametrize("alg", ["td7", "sac"])
def test_export_dict_keeps_its_keys_and_shapes(alg):
    ag = _agent(alg)
    st = ag._export()
    assert list(st) == ["params", "adam", "counters", "vbounds", "act_counter"]
    names = ag._param_names()
    nets = [net for net, _ in names] + (["tmp"] if alg == "sac" else [])
    optim = [net for net, _ in names if net in ag.OPTIM_NETS] + (["tmp"] if alg == "sac" else [])
    assert list(st["params"]) == nets and list(st["adam"]) == optim
    for net, ns in names:
        assert list(st["params"][net]) == [n for n, _ in ns]
        for n, shp in ns:
            v = st["params"][net][n]
            assert v.dtype == np.float32 and v.shape == tuple(shp), (net, n)
            if net in optim:
                m, v2 = st["adam"][net][n]
                assert m.dtype == v2.dtype == np.float32 and m.shape == v2.shape == tuple(shp), (net, n)
    if alg == "sac":
        assert st["params"]["tmp"]["log_alpha"].shape == (1,)
        assert [x.shape for x in st["adam"]["tmp"]["log_alpha"]] == [(1,), (1,)]
    assert st["counters"].shape == (6,) and st["vbounds"].shape == (4,) and isinstance(st["act_counter"], int)
    # the dict a pickle from before the blob holds (arrays of their own, tensor by tensor) still loads
    e = ag.engine
    old = {"params": {net: {n: e.get_param(net, n, s) for n, s in ns} for net, ns in names},
           "adam": {net: {n: (e.get_adam(net, n, 0, s), e.get_adam(net, n, 1, s)) for n, s in ns}
                    for net, ns in names if net in ag.OPTIM_NETS},
           "counters": e.counters(), "vbounds": e.value_bounds(), "act_counter": e.act_counter()}
    if alg == "sac":
        old["params"]["tmp"] = {"log_alpha": e.get_param("tmp", "log_alpha")}
        old["adam"]["tmp"] = {"log_alpha": (e.get_adam("tmp", "log_alpha", 0), e.get_adam("tmp", "log_alpha", 1))}
    _assert_same_params(st["params"], old["params"])
    other = _agent(alg, seed=10)
    other._import(old)
    _assert_same_params(other.state_dict(), ag.state_dict())
    other.load_params({"policy": {k: v * 0 for k, v in st["params"]["policy"].items()}})  # (a partial dict)
    assert all(not v.any() for v in other.state_dict()["policy"].values())
    np.testing.assert_array_equal(other.state_dict()["q1"]["mlp.0.weight" if alg == "sac" else "q01.weight"],
                                  st["params"]["q1"]["mlp.0.weight" if alg == "sac" else "q01.weight"])


def test_load_state_dict_between_batch_sizes():
    a, b = _agent("td7", seed=1, batch=32), _agent("td7", seed=2, batch=64)
    rep = _agent_replay("td7")
    a.train_n(rep, 32, 2)
    assert b.load_state_dict(a) is b
    _assert_same_params(b.state_dict(), a.state_dict())
    assert b.n_runs == 0 and b.batch_size == 64
    with pytest.raises(TypeError):
        b.load_state_dict(_agent("sac"))


# ---- 6. size errors ----------------------------------------------------------------------------------------------

def test_size_and_mask_errors_come_back_through_the_abi():
    lib = E.lib()
    eng = _engine("td7_tiny")
    n = eng.state_size(E.STATE_ALL)
    buf = np.zeros(n + 1, np.float32)
    for bad in (n - 1, n + 1, 0):
        assert lib.rle_state_export(eng.h, E.STATE_ALL, E._fp(buf), bad) == -1
        assert b"n_floats" in lib.rle_last_error()
        assert lib.rle_state_import(eng.h, E.STATE_ALL, E._fp(buf), bad) == -1
        assert b"n_floats" in lib.rle_last_error()
    for what in (0, 8, -1):
        assert lib.rle_state_import(eng.h, what, E._fp(buf), n) == -1
        assert b"mask" in lib.rle_last_error()
        assert lib.rle_state_export(eng.h, what, E._fp(buf), n) == -1
        cnt = ctypes.c_int()
        assert lib.rle_state_toc(eng.h, what, None, 0, ctypes.byref(cnt)) == -1
    assert lib.rle_state_export(eng.h, E.STATE_ALL, None, n) == -1
    assert not eng.state_export(E.STATE_ALL).any()  # (a fresh engine; and the failures above left it usable)
