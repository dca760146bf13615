"""Offline SAC (rle_config_ext awac_lambda, SAC(offline=True)): the CPU side.

The oracle's restatement with the AWAC policy step (tests/offline_sac_oracle.py) is pinned against the online
oracle and against its own hand-written gradient, every parity case of tests/offline_sac_cases.py is shown to be a
valid reference (float32 against float64 under the engine's criteria, with the action and clamp edges present),
and the ABI and the Python class carry and validate the setting without a GPU.
"""

import copy
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import offline_sac_cases as C
from conftest import REPO
from offline_sac_oracle import A_MAX, INFO_KEYS, W_MAX, awac_grads, awac_logp
from oracle import agents

torch.set_num_threads(1)


# ---- the oracle -------------------------------------------------------------------------------------------

def _state(orc):
    out = {f"{net}.{k}": v.detach().numpy().copy() for net, d in orc.nets().items() for k, v in d.items()}
    out.update(agents.moments(orc))
    return out


@pytest.mark.parametrize("case", ["base", "a25"])
def test_awac_oracle_with_the_term_off_is_the_online_oracle_bitwise(case):
    """Four steps: info, every parameter and every Adam moment of AWACOracle(lmbda=0) equal those of
    oracle.agents.SACOracle(tmp=0) bit for bit -- the restated step is the online step plus the term."""
    on, rep_on = C.build_oracle(case, online=True)
    off, rep_off = C.build_oracle(case, lmbda=0.0)
    tp = C.tapes(case)
    B = C.CASES[case].B
    i_on, ind_on = agents.run_steps(on, "sac", rep_on, tp, C.N_STEPS, B)
    i_off, ind_off = agents.run_steps(off, "sac", rep_off, tp, C.N_STEPS, B)
    for a, b in zip(ind_on, ind_off):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(i_on, i_off):
        assert a == b and list(b) == ["train/q_fn", "train/policy", "entropy"]
    s_on, s_off = _state(on), _state(off)
    assert s_on.keys() == s_off.keys()
    for k in s_on:
        np.testing.assert_array_equal(s_on[k], s_off[k], err_msg=k)


def _gradient_rows(dtype):
    """[mean | raw log_std | dataset action] rows that cover a = +1, a = -1, a = 0, log_std above and below the
    clamps [-2, 1] and exactly on them (where the clamp passes gradient), and plain rows."""
    rng = np.random.default_rng(5)
    n, A = 12, 4
    mean = rng.standard_normal((n, A))
    ls = rng.uniform(-1.5, 0.5, (n, A))
    a = rng.uniform(-0.95, 0.95, (n, A))
    a[0, :] = 1.0
    a[1, :] = -1.0
    a[2, :] = 0.0
    a[3, 0], a[3, 1], a[3, 2] = 1.0, -1.0, 0.0
    ls[4, :] = 3.5
    ls[5, :] = -7.0
    ls[6, 0], ls[6, 1] = 1.0, -2.0
    ls[7, 0], ls[7, 1], a[7, 0], a[7, 1] = 2.0, -2.5, 1.0, -1.0
    w = np.concatenate([rng.uniform(0.2, 3.0, n - 1), [W_MAX]])
    return tuple(torch.tensor(x, dtype=dtype) for x in (mean, ls, a, w))


def test_hand_written_gradients_equal_autograd_in_float64():
    """dL/dmu = -(w/B) (u - mu) / sigma^2 and dL/dl = -(w/B) ((u - mu)^2 / sigma^2 - 1) where the clamp passes
    gradient, else 0 (the device op's formulas, offline_sac_oracle.awac_grads) against autograd of
    L = -mean(w logp) in float64."""
    mean, ls, a, w = _gradient_rows(torch.float64)
    mean.requires_grad_(True)
    ls.requires_grad_(True)
    loss = -(w.reshape(-1, 1) * awac_logp(mean, ls, a, C.MIN_LOG_STD, C.MAX_LOG_STD)).mean()
    g_mu, g_ls = torch.autograd.grad(loss, [mean, ls])
    h_mu, h_ls = awac_grads(mean.detach(), ls.detach(), a, w, C.MIN_LOG_STD, C.MAX_LOG_STD)
    np.testing.assert_allclose(h_mu.numpy(), g_mu.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(h_ls.numpy(), g_ls.numpy(), rtol=1e-12, atol=1e-14)
    assert (g_ls[4] == 0).all() and (g_ls[5] == 0).all() and (g_ls[7, :2] == 0).all()  # beyond either clamp
    assert (g_ls[6, :2] != 0).all()                                                      # on the bound: passes
    assert torch.isfinite(g_mu).all() and (g_mu[0].abs() > 0).all()
    # a = +-1 is clamped to the fp32 value of 1 - 1e-6 before atanh
    u = torch.atanh(torch.clamp(a, -A_MAX, A_MAX))
    assert A_MAX == float(np.float32(1.0) - np.float32(1e-6))
    assert float(u.abs().max()) == pytest.approx(0.5 * np.log((1 + A_MAX) / (1 - A_MAX)), rel=1e-12)  # 7.2477


def test_oracle_step_uses_those_gradients_and_the_issue_objective():
    """One step of the baseline case: the raw-head gradient autograd took equals the hand-written one, w is
    min(exp(adv / lmbda), 100) of the reported mean advantage's rows, and the info keys are the five."""
    orc, rep = C.build_oracle("base")
    tp = C.tapes("base")
    info, _ = agents.run_steps(orc, "sac", rep, {k: v[:1] for k, v in tp.items()}, 1, C.CASES["base"].B)
    assert tuple(info[0]) == INFO_KEYS
    L = orc.last
    h_mu, h_ls = awac_grads(L["mean"], L["log_std"], L["a"], L["w"], C.MIN_LOG_STD, C.MAX_LOG_STD)
    np.testing.assert_allclose(h_mu.numpy(), L["g_mean"].numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(h_ls.numpy(), L["g_log_std"].numpy(), rtol=1e-5, atol=1e-7)
    assert info[0]["train/weight"] == pytest.approx(float(L["w"].mean()))
    assert float(L["w"].max()) <= W_MAX and float(L["w"].min()) > 0


@pytest.mark.parametrize("case", list(C.CASES))
def test_case_is_a_valid_reference(case):
    """The float32 oracle meets the engine's criteria against its float64 run at the recorded seed, and the
    case's batches hold a +1, a -1 and a 0 action entry and a row at each log-std clamp."""
    ref = C.reference(case)
    bad = C.shortfalls(ref["f32"], ref["f64"], C.N_STEPS)
    assert not bad, bad
    assert all(ref["f32"]["seen"].values()), ref["f32"]["seen"]
    assert np.isfinite(ref["f64"]["table"]).all()


# ---- the ABI without a GPU ---------------------------------------------------------------------------------

def test_config_ext_matches_the_header_layout(tmp_path):
    """rl/_engine.py ConfigExt mirrors rle_config_ext field by field (a C program compiled against include/rle.h),
    awac_lambda is its last field, after bc_alpha."""
    import shutil
    import subprocess

    from rl import _engine as E

    assert [f for f, *_ in E.ConfigExt._fields_] == ["size", "bc_alpha", "awac_lambda"]
    assert E.make_config_ext().awac_lambda == 0.0 and E.make_config_ext(awac_lambda=0.5).awac_lambda == 0.5
    assert E.make_config_ext(awac_lambda=0.5).size == ctypes.sizeof(E.ConfigExt) == 12
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['printf("rle_config_ext %zu\\n", sizeof(rle_config_ext));']
    for f, *_ in E.ConfigExt._fields_:
        lines.append(f'printf("rle_config_ext.{f} %zu\\n", offsetof(rle_config_ext, {f}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rle.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.splitlines())
    assert int(got["rle_config_ext"]) == ctypes.sizeof(E.ConfigExt)
    for f, *_ in E.ConfigExt._fields_:
        assert int(got[f"rle_config_ext.{f}"]) == getattr(E.ConfigExt, f).offset, f


def _create(algo, ext, **cfg_kw):
    from rl import _engine as E

    lib = E.lib()
    out = ctypes.c_void_p()
    cfg = E.make_config(algo, 11, 3, 32, 16, **cfg_kw)
    rc = lib.rle_create_ext(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(out))
    err = lib.rle_last_error()
    if rc == 0:  # (a host with a GPU: the engine exists)
        lib.rle_destroy(out)
    return rc, err


def test_create_ext_rejects_bad_awac_lambda_before_any_hip_call():
    """Negative, NaN, infinite, > 0 with TD7 / TD3, > 0 with tmp != 0 (auto or fixed) or with use_lap, and a size
    that is no field boundary of the struct: RLE_EINVAL with a message naming awac_lambda, on a host without a
    GPU."""
    from rl import _engine as E

    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        rc, err = _create(E.RLE_SAC, E.make_config_ext(awac_lambda=bad), tmp=0.0)
        assert rc == -1 and b"awac_lambda" in err, (bad, err)
    for algo in (E.RLE_TD7, E.RLE_TD3):
        rc, err = _create(algo, E.make_config_ext(awac_lambda=1.0))
        assert rc == -1 and b"awac_lambda" in err, (algo, err)
    for tmp in (-1.0, 0.2):
        rc, err = _create(E.RLE_SAC, E.make_config_ext(awac_lambda=1.0), tmp=tmp)
        assert rc == -1 and b"awac_lambda" in err and b"tmp" in err, (tmp, err)
    rc, err = _create(E.RLE_SAC, E.make_config_ext(awac_lambda=1.0), tmp=0.0, use_lap=True)
    assert rc == -1 and b"awac_lambda" in err and b"use_lap" in err, err
    for size in (0, -4, 4, 9, 10, 11, 13, 16):
        ext = E.make_config_ext(awac_lambda=1.0)
        ext.size = size
        rc, err = _create(E.RLE_SAC, ext, tmp=0.0)
        assert rc == -1 and b"8 (bc_alpha), 12 (awac_lambda)" in err, (size, err)


def test_size_8_reads_awac_lambda_as_unset():
    """A caller compiled before the field existed passes size = 8: whatever lies behind it is not read, so the
    engine is the online one (here: TD3, SAC with an automatic temperature and SAC with LAP pass validation, which
    awac_lambda > 0 would refuse), and create gets as far as the device."""
    from rl import _engine as E

    for algo, kw in ((E.RLE_TD3, {}), (E.RLE_SAC, dict(tmp=-1.0)), (E.RLE_SAC, dict(tmp=0.0, use_lap=True))):
        ext = E.make_config_ext(awac_lambda=1.0)
        ext.size = 8
        rc, err = _create(algo, ext, **kw)
        assert rc in (0, -2), (rc, err)  # (RLE_EHIP: no device on this host)
        assert rc == 0 or b"awac_lambda" not in err


# ---- the Python class without a device ---------------------------------------------------------------------

class _FakeEngine:
    """Stands in for rl._engine.Engine: keeps what the agent built it with."""

    made = []

    def __init__(self, cfg, plan=None, ext=None):
        self.cfg, self.ext, self.replay = cfg, ext, None
        _FakeEngine.made.append(self)

    def copy_state_from(self, other):
        pass

    def close(self):
        pass


@pytest.fixture
def sac_cls(monkeypatch):
    from rl import _engine as E
    from rl.agent import SAC
    from rl.agent.engine_agent import EngineAgent
    from rl.utils import register_env

    register_env("Tiny-v0", 11, 3, -0.5, 0.5)
    _FakeEngine.made.clear()
    monkeypatch.setattr(E, "Engine", _FakeEngine)
    monkeypatch.setattr(EngineAgent, "_import", lambda self, st: None)
    monkeypatch.setattr(EngineAgent, "_export", lambda self, *a, **k: {"params": {}})
    return SAC


def test_constructor_refusals(sac_cls):
    for kw in (dict(lmbda=0.0), dict(lmbda=-1.0), dict(lmbda=float("nan")), dict(lmbda=float("inf")),
               dict(tmp=0.2), dict(tmp=-0.5)):
        with pytest.raises(ValueError):
            sac_cls("Tiny-v0", hidden=32, batch_size=16, seed=1, offline=True, **kw)
    assert not _FakeEngine.made  # (refused before any engine)
    with pytest.raises(TypeError):
        sac_cls("Tiny-v0", 0.99, 3e-4, 3e-4, -20.0, 2.0, 0.005, -1.0, False, float("inf"), None, True)  # keyword-only
    for tmp in (-1.0, 0.0):
        ag = sac_cls("Tiny-v0", tmp=tmp, hidden=32, batch_size=16, seed=1, offline=True)
        assert ag.engine.cfg.tmp == 0.0 and ag.engine.ext.awac_lambda == 1.0 and not ag.auto_tmp_mode
    lap = sac_cls("Tiny-v0", use_lap=True, hidden=32, batch_size=16, seed=1)
    with pytest.raises(AttributeError, match="_lap_huber"):
        lap.train_n(None, 16, 1)
    # offline=False ignores lmbda
    on = sac_cls("Tiny-v0", hidden=32, batch_size=16, seed=1, lmbda=-3.0)
    assert not on.offline and on.engine.ext is None and on.auto_tmp_mode and len(on._info_keys()) == 6


def test_info_keys_and_the_mode_through_pickle_deepcopy_and_rebuild(sac_cls):
    ag = sac_cls("Tiny-v0", hidden=32, batch_size=16, seed=1, offline=True, lmbda=0.7)
    keys = ("train/q_fn", "train/policy", "entropy", "train/adv", "train/weight")
    assert ag._info_keys() == keys and ag.offline and ag.lmbda == 0.7 and ag.tmp == 0.0
    assert ag._info(np.arange(8, dtype=np.float32)) == dict(zip(keys, [0.0, 1.0, 2.0, 3.0, 4.0]))
    assert ag.__getstate__()["_ext"] == {"awac_lambda": 0.7}
    ag2 = pickle.loads(pickle.dumps(ag))
    ag3 = copy.deepcopy(ag)
    ag._rebuild(48)
    for a in (ag, ag2, ag3):
        assert a.offline and a.lmbda == 0.7 and a._info_keys() == keys
        assert a.engine.ext.awac_lambda == pytest.approx(0.7) and a.engine.cfg.tmp == 0.0
    assert ag.batch_size == 48 and ag2.batch_size == 16
    # a pickle written before the mode existed (none of its attributes) loads as online
    on = sac_cls("Tiny-v0", tmp=0.0, hidden=32, batch_size=16, seed=1)
    st = on.__getstate__()
    for k in ("offline", "lmbda"):
        st.pop(k)
    assert "_ext" not in st
    old = sac_cls.__new__(sac_cls)
    old.__setstate__(copy.deepcopy(st))
    assert not old.offline and old.engine.ext is None and old._info_keys() == ("train/q_fn", "train/policy", "entropy")
