"""Gradient-norm clipping in the device step (rle_set_grad_clip) against the clipped CPU oracle
(tests/grad_clip_oracle.py) at the cases of tests/grad_clip_cases.py, through the C ABI and the Python mirror.

Tolerances are the project's existing ones (DESIGN "Oracle and parity", tests/harness.py): indices exact,
priorities rtol 1e-4 / atol 1e-5, TD7 value bounds 1e-4, info columns and rle_grad_clip_stats rtol 1e-3 / atol
1e-4, the Adam m and v of every tensor after step 1 (TD7's policy: after step 2, its first update) within
1e-4 |ref| + 1e-4 max |ref|, end parameters every element within 2 lr n + 1e-4 and 99% of each tensor within 1e-5.
"""

import copy
import math
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
import edge_cases as EC  # noqa: E402
import grad_clip_cases as C  # noqa: E402
import grad_clip_oracle as GO  # noqa: E402
from harness import LOSS_RTOL  # noqa: E402
from test_engine_gpu import assert_params_close  # noqa: E402

ALL_FUSIONS = [k for k in E.FUSE if k != "priosample"]  # (priosample is opt-in: off unless switched on)
UNSET = object()


def clip_engine(name, max_norm=UNSET, plan=None, extra=None):
    """(engine, replay) of a case; max_norm: the case's own by default, None = rle_set_grad_clip is never called.
    extra: other constructor hyper-parameters of an edge case (its golden's meta_extra)."""
    c = C.CLIP_CASES[name]
    if c.kind == "edge":
        from test_shape_edges_gpu import _engine

        g = dict(EC.golden(c.src))
        if extra:
            g["meta_extra_keys"] = np.array(list(extra), dtype="<U32")
            g["meta_extra_vals"] = np.array(list(extra.values()), np.float64)
        with C.registered(name):
            eng, rep = _engine(name, plan, g)
    elif c.kind == "td3bc":
        from test_offline_td3_gpu import offline_engine

        with C.td3bc_env():
            eng, rep = offline_engine(C.td3bc_golden(), C.TD3BC_ALPHA, plan)
    else:
        from test_offline_sac_gpu import offline_engine

        eng, rep = offline_engine(c.src, plan=plan)
    if max_norm is not None:
        eng.set_grad_clip(c.max_norm if max_norm is UNSET else max_norm)
    return eng, rep


def tapes(name):
    return C.build(name)[2]


def _tape(eng, tp):
    eng.set_tapes(u=tp["u"], eps=tp["eps"], eps_pi=tp.get("eps_pi"))


def _moments(eng, ref):
    def got(key):
        name, which = key.rsplit(":", 1)
        net, pname = name.split(".", 1)
        return eng.get_adam(net, pname, 0 if which == "m" else 1, ref[key].shape)

    return C.moment_shortfalls(got, ref)


def _stats(eng):
    st = eng.grad_clip_stats()
    return np.array([x for k in GO.ORDER for x in st[k]], np.float64)


def check_case(name, max_norm=UNSET, plan=None):
    """One run of the case step by step against the clipped float32 oracle; returns the moment shortfalls (the other
    criteria are asserted unless the engine runs unclipped on purpose, max_norm None)."""
    ref = C.reference(name)["f32"]
    n, alg = ref["n"], C.alg_of(name)
    lap = ref["prio"][0] is not None
    eng, rep = clip_engine(name, max_norm, plan)
    clipped = max_norm is not None
    _tape(eng, tapes(name))
    infos, bad = [], []
    for t in range(n):
        infos.append(eng.step(1)[0].copy())
        np.testing.assert_array_equal(eng.last_indices(), ref["ind"][t])
        if t == 0:
            bad += _moments(eng, ref["m"])
        if t == 1 and ref["m2"]:
            bad += _moments(eng, ref["m2"])
        if not clipped:
            continue
        if lap:
            np.testing.assert_allclose(rep.get_priority(len(ref["prio"][t])), ref["prio"][t], rtol=1e-4, atol=1e-5)
        if alg == "td7":
            np.testing.assert_allclose(eng.value_bounds(), ref["vb"][t].astype(np.float32), rtol=1e-4, atol=1e-4)
        st, want = _stats(eng), C.stats_after(ref, t)
        print("CLIP", name, "step", t + 1, "stats", st.tolist(), "oracle", want.tolist())
        np.testing.assert_allclose(st, want, rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    eng.set_tapes()
    print("CLIP", name, "moment shortfalls", bad)
    if not clipped:
        return bad
    k = len(ref["keys"])
    infos = np.asarray(infos, np.float64)[:, :k]
    np.testing.assert_array_equal(np.isnan(infos), np.isnan(ref["table"]))
    np.testing.assert_allclose(infos, ref["table"], rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    tol = 2 * 3e-4 * n + 1e-4
    for (net, pname), v in ref["params"].items():
        assert_params_close(eng.get_param(net, pname, v.shape), v, tol, (net, pname), bulk=0.99)
    if alg == "sac" and C.CLIP_CASES[name].kind == "edge":  # (the autotuned temperature; AWAC's is fixed at 0)
        np.testing.assert_allclose(eng.get_param("tmp", "log_alpha"), ref["log_alpha"].reshape(-1), rtol=1e-5, atol=1e-7)
    assert "clip" in eng.describe(0) and "gsq" in eng.describe(0)
    return bad


@pytest.mark.parametrize("name", list(C.CLIP_CASES))
def test_clipped_steps_match_the_clipped_oracle(name):
    assert check_case(name) == []


def test_unclipped_engine_misses_the_moment_criterion_of_the_clipped_oracle():
    """The same case without rle_set_grad_clip against the clipped oracle: at clip-sac-h260 the critics' coef is
    0.14-0.16, so their first moments are off by a factor of about 6 and the moment criterion must be missed."""
    bad = check_case("clip-sac-h260", max_norm=None)
    assert any(key.startswith("q1.") and key.endswith(":m") and worst > 1000 for key, _, worst in bad), bad


@pytest.mark.parametrize("name", ["clip-td7-odd", "clip-td3-k49"])
def test_clipped_steps_with_every_fusion_off_match_the_oracle(name):
    assert check_case(name, plan=E.make_plan(fuse_off=ALL_FUSIONS)) == []


def _run(eng, rep, name, calls):
    _tape(eng, tapes(name))
    infos = []
    for k in calls:
        infos += [r.copy() for r in eng.step(k)]
    eng.set_tapes()
    return {"info": np.asarray(infos, np.float32), "state": eng.state_export(E.STATE_ALL).copy(),
            "ind": eng.last_indices().copy()}


def _same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum())
                                                  if a[k].dtype == np.float32 else k)


@pytest.mark.parametrize("name", ["clip-td7-odd", "clip-td3-k49", "clip-sac-a25"])
def test_clipping_off_is_the_unclipped_program(name):
    """No call, rle_set_grad_clip(0) and (+inf): the same rle_graph_describe text of every program and bitwise the
    same parameters, moments and info after the case's steps; the setting reads back 0 and the stats NaN."""
    n = EC.CASES[C.CLIP_CASES[name].src].n_steps
    runs, texts = [], []
    for max_norm in (None, 0.0, math.inf):
        eng, rep = clip_engine(name, max_norm)
        assert eng.grad_clip() == 0.0
        runs.append(_run(eng, rep, name, (1,) * n))
        texts.append([eng.describe(w) for w in ((0, 3) if C.alg_of(name) == "sac" else (0, 1, 3))])
        assert np.isnan(_stats(eng)).all()
        assert "clip" not in texts[-1][0] and "gsq" not in texts[-1][0]
    assert texts[0] == texts[1] == texts[2]
    _same(runs[0], runs[1], (name, "0"))
    _same(runs[0], runs[2], (name, "inf"))


@pytest.mark.parametrize("name", ["clip-td7-odd", "clip-td3-k49", "clip-sac-a25"])
def test_clipped_burst_equals_single_steps_bitwise(name):
    """rle_step(20) of a clipped engine -- the default multi-step program, its remainder programs and single steps --
    against 20 x rle_step(1), and a second burst against the first: bit for bit.  (TD7: target_update_rate 250, so
    no hard update breaks the burst up; the draws are the engine's own Philox streams.)"""
    extra = {"target_update_rate": 250} if C.alg_of(name) == "td7" else None
    out = []
    for calls in ((1,) * 20, (20,), (20,)):
        eng, rep = clip_engine(name, extra=extra)
        l0 = eng.launch_count()
        infos = []
        for k in calls:
            infos += [r.copy() for r in eng.step(k)]
        out.append({"info": np.asarray(infos, np.float32), "state": eng.state_export(E.STATE_ALL).copy(),
                    "stats": _stats(eng).astype(np.float32)})
        out[-1]["launches"] = eng.launch_count() - l0
        assert eng.plan()["steps_per_graph"] == {"td7": 6, "td3": 16, "sac": 8}[C.alg_of(name)]
    launches = [o.pop("launches") for o in out]
    assert launches[1] == launches[2] and 0 < launches[1] <= launches[0], launches
    _same(out[0], out[1], (name, "burst vs single"))
    _same(out[1], out[2], (name, "burst vs burst"))
    assert np.isfinite(out[1]["info"][:, 0]).all()


@pytest.mark.parametrize("check", ["RLE_AUDIT", "RLE_HAZARD"])
@pytest.mark.parametrize("name", ["clip-td7-odd_bc", "clip-td3bc-odd", "clip-awac-b17", "clip-sac-h260"])
def test_clipped_programs_pass_audit_and_hazard_checks(name, check, monkeypatch):
    """The address replay of every GEMM (the norm passes and the scaled Adam passes among them) and the byte-level
    race check of every level (OP_CLIP's partials, stats and scalar) over a clipped engine's single-step and
    multi-step programs; then steps run."""
    monkeypatch.setenv(check, "1")
    eng, rep = clip_engine(name)
    eng.step(3)


def test_setter_errors():
    eng, rep = clip_engine("clip-td3-k49", None)
    lib = E.lib()
    assert lib.rle_set_grad_clip(eng.h, -1.0) == -1  # RLE_EINVAL
    assert lib.rle_set_grad_clip(eng.h, float("nan")) == -1
    assert b"max_norm" in lib.rle_last_error()
    eng.set_grad_clip(0.5)
    assert eng.grad_clip() == 0.5
    eng.set_grad_clip(math.inf)
    assert eng.grad_clip() == 0.0
    eng.set_grad_clip(0.3)
    eng.step(1)
    rc = lib.rle_set_grad_clip(eng.h, 1.0)
    assert rc not in (0, -1) and b"first step" in lib.rle_last_error(), rc  # RLE_ESTATE
    assert eng.grad_clip() == np.float32(0.3)


def test_state_copies_between_clipped_and_unclipped_engines():
    """rle_copy_state from a clipped into an unclipped engine and back; rle_copy_nets and the packed state too."""
    name = "clip-td3-k49"
    on, _ = clip_engine(name)
    off, rep_off = clip_engine(name, None)
    on.step(4)
    off.copy_state_from(on)
    assert on.state_export(E.STATE_ALL).tobytes() == off.state_export(E.STATE_ALL).tobytes()
    np.testing.assert_array_equal(on.counters(), off.counters())
    off.step(2)
    assert np.isnan(_stats(off)).all()
    on2, _ = clip_engine(name)
    on2.copy_state_from(off)
    assert on2.state_export(E.STATE_ALL).tobytes() == off.state_export(E.STATE_ALL).tobytes()
    on2.step(2)
    st = on2.grad_clip_stats()
    assert np.isfinite(st["critics"]).all() and 0 < st["critics"][1] <= 1
    on3, _ = clip_engine(name)
    on3.copy_nets_from(off)
    np.testing.assert_array_equal(on3.get_param("q1", "mlp.0.weight"), off.get_param("q1", "mlp.0.weight"))
    on3.state_import(off.state_export(E.STATE_ALL), E.STATE_ALL)
    np.testing.assert_array_equal(on3.get_adam("q1", "mlp.0.weight", 1), off.get_adam("q1", "mlp.0.weight", 1))


# ---- the Python mirror ------------------------------------------------------------------------------------

def _dataset(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 11)).astype(np.float32), rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32),
            (3 * rng.standard_normal(n)).astype(np.float32), rng.standard_normal((n, 11)).astype(np.float32),
            (rng.random(n) > 0.1).astype(np.float32))


@pytest.mark.parametrize("alg", ["td7", "td3", "sac"])
def test_mirror_keyword_reaches_the_engine_and_survives_copies(alg):
    from rl.agent import SAC, TD3, TD7
    from rl.replay_memory import LAPReplayMemory, SimpleReplayMemory
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    cls = {"td7": TD7, "td3": TD3, "sac": SAC}[alg]
    lap = alg != "sac"
    kw = dict(hidden=32, batch_size=16, seed=5, use_lap=lap)
    ag = cls("Tiny-v0", clip_grad_norm=0.05, **kw)
    assert ag.clip_grad_norm == 0.05 and ag.engine.grad_clip() == np.float32(0.05)
    assert set(ag.grad_clip_stats()) == ({"critics", "policy", "encoder"} if alg == "td7" else {"critics", "policy"})
    rep = (LAPReplayMemory if lap else SimpleReplayMemory)(512, "Tiny-v0")
    rep.append_batch(*_dataset(300, 11))
    ag.train_n(rep, 16, 4)
    st = ag.grad_clip_stats()
    assert st["critics"][1] < 1 and abs(st["critics"][0] * st["critics"][1] - 0.05) < 1e-4, st
    for other in (pickle.loads(pickle.dumps(ag)), copy.deepcopy(ag)):
        assert other.clip_grad_norm == 0.05 and other.engine.grad_clip() == np.float32(0.05)
    ag.train_n(rep, 17, 2)  # (a batch-size rebuild)
    assert ag.batch_size == 17 and ag.engine.grad_clip() == np.float32(0.05)
    assert ag.grad_clip_stats()["critics"][1] < 1
    ag.to("cuda:0")
    assert ag.engine.grad_clip() == np.float32(0.05)
    # an agent pickled without the attribute trains unclipped
    plain = cls("Tiny-v0", **kw)
    assert "clip_grad_norm" not in plain.__dict__ and plain.engine.grad_clip() == 0.0
    old = pickle.loads(pickle.dumps(plain))
    assert old.clip_grad_norm == math.inf and old.engine.grad_clip() == 0.0
    old.train_n(rep, 16, 2)
    plain.train_n(rep, 16, 2)
    assert all(math.isnan(x) for v in old.grad_clip_stats().values() for x in v)
    if alg == "sac":  # the reference's positional max_grad_norm alone changes nothing
        ref_style = SAC("Tiny-v0", max_grad_norm=1.0, **kw)
        assert ref_style.max_grad_norm == 1.0 and ref_style.engine.grad_clip() == 0.0
        ref_style.train_n(rep, 16, 2)
        assert ref_style.engine.describe(0) == plain.engine.describe(0)
        assert "clip" not in plain.engine.describe(0) and "clip" in ag.engine.describe(0)
