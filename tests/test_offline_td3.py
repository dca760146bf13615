"""Offline TD3 (rle_config_ext bc_alpha, TD3(offline=True)) and the replay's state normalisation: the CPU side.

The oracle's restatement with the TD3+BC objective (tests/offline_td3_oracle.py) is pinned against the online
oracle, both terms of the action gradient are shown to matter at alpha = 2.5 on every golden the GPU parity
tests use, and the ABI carries and validates the extension struct without a GPU.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
from offline_td3_oracle import build_offline_td3
from oracle import agents
from test_oracle import build_from_golden

torch.set_num_threads(1)

ALPHA = 2.5
GOLDENS = ["td3_tiny", "td3_tiny_lap", "td3_tiny_b100", "td3_tiny_deep", "td3_tiny_act", "td3_tiny_hp"]


def _state(orc):
    out = {}
    for net, d in orc.nets().items():
        for k, v in d.items():
            out[f"{net}.{k}"] = v.detach().numpy().copy()
    out.update(agents.moments(orc))
    return out


def _first_policy_step(orc, alg, rep, tp, B, limit=8):
    """Run to the first policy step; returns (its info, the number of steps taken)."""
    for t in range(limit):
        i1, _ = agents.run_steps(orc, alg, rep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
        if i1[0]["train/policy"] is not None:
            return i1[0], t + 1
    raise AssertionError("no policy step")


@pytest.mark.parametrize("name", ["td3_tiny", "td3_tiny_lap"])
def test_bc_oracle_with_alpha_zero_is_the_online_oracle_bitwise(name):
    """The golden's own steps (6 / 4, policy steps among them): info, every parameter, every Adam moment and the
    priorities of TD3BCOracle(alpha=0) equal oracle.agents.TD3Oracle's bit for bit -- the restated step is the
    online step plus the term."""
    g = load_golden(name)
    alg, on, rep_on, tp, n, B = build_from_golden(g)
    off, rep_off, _, _, _ = build_offline_td3(g, 0.0)
    i_on, ind_on = agents.run_steps(on, alg, rep_on, tp, n, B)
    i_off, ind_off = agents.run_steps(off, alg, rep_off, tp, n, B)
    assert any(i["train/policy"] is not None for i in i_on)
    for a, b in zip(ind_on, ind_off):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(i_on, i_off):
        for k in a:
            assert a[k] == b[k], k
        assert b["train/bc"] is None and b["train/lmbda"] is None
    s_on, s_off = _state(on), _state(off)
    assert s_on.keys() == s_off.keys()
    for k in s_on:
        np.testing.assert_array_equal(s_on[k], s_off[k], err_msg=k)
    np.testing.assert_array_equal(rep_on.priority, rep_off.priority)


@pytest.mark.parametrize("name", GOLDENS)
def test_both_terms_are_visible_at_alpha_2_5(name):
    """Sensitivity guard for the GPU parity tests: on the first policy step of each golden they use, the Q part
    and the BC part are each at least 10% of the norm of the full action gradient (a parity test could
    otherwise pass with either term missing), and the actor's Adam m differs from the online oracle's by far
    more (100 x) than the 1e-4 |m| + 1e-4 max|m| the engine's moments are held to after that step."""
    g = load_golden(name)
    alg, on, rep_on, tp, _, B = build_from_golden(g)
    off, rep_off, _, _, _ = build_offline_td3(g, ALPHA)
    _first_policy_step(on, alg, rep_on, tp, B)
    info, _ = _first_policy_step(off, alg, rep_off, tp, B)
    assert info["train/bc"] > 0 and info["train/lmbda"] > 0
    g_q, g_bc = off.last_action_grads
    full = float((g_q + g_bc).norm())
    share = min(float(g_q.norm()), float(g_bc.norm())) / full
    print(name, "shares of the full action gradient: Q", float(g_q.norm()) / full, "BC", float(g_bc.norm()) / full)
    assert share >= 0.1, share
    m_on, m_off = agents.moments(on), agents.moments(off)
    worst = 0.0
    for k in m_on:
        if k.startswith("policy.") and k.endswith(":m"):
            worst = max(worst, float(np.abs(m_on[k] - m_off[k]).max()) / (2e-4 * float(np.abs(m_on[k]).max())))
    print(name, "actor m: online vs offline, in units of the parity bound:", worst)
    assert worst >= 100.0, worst


def test_bc_oracle_objective_is_the_issue_formula():
    """train/policy = -lmbda * mean(Q) + bc with the returned lmbda and bc; mean(Q) is minus the online oracle's
    train/policy of the same step (same nets and batches up to the first policy step)."""
    g = load_golden("td3_tiny")
    alg, on, rep_on, tp, _, B = build_from_golden(g)
    off, rep_off, _, _, _ = build_offline_td3(g, ALPHA)
    i_on, n_on = _first_policy_step(on, alg, rep_on, tp, B)
    i_off, n_off = _first_policy_step(off, alg, rep_off, tp, B)
    assert n_on == n_off
    mean_q = -i_on["train/policy"]
    want = -i_off["train/lmbda"] * mean_q + i_off["train/bc"]
    np.testing.assert_allclose(i_off["train/policy"], want, rtol=1e-6)


# ---- the ABI without a GPU ---------------------------------------------------------------------------------

def test_config_ext_matches_the_header_layout(tmp_path):
    """rl/_engine.py ConfigExt mirrors rle_config_ext field by field (a C program compiled against include/rle.h,
    as tests/test_abi.py does for rle_config), and rle_config is as it was: bc_lambda its last field."""
    import shutil
    import subprocess

    from rl import _engine as E

    assert E.Config._fields_[-1][0] == "bc_lambda"
    assert E.make_config_ext().size == ctypes.sizeof(E.ConfigExt) and E.make_config_ext().bc_alpha == 0.0
    assert E.make_config_ext(bc_alpha=2.5).bc_alpha == 2.5
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


def test_create_ext_rejects_bad_bc_alpha_before_any_hip_call():
    """Negative, NaN, infinite, > 0 with TD7 / SAC, and a size that does not reach the field: RLE_EINVAL with a
    message naming bc_alpha, through the ABI on a host without a GPU."""
    from rl import _engine as E

    lib = E.lib()
    out = ctypes.c_void_p()

    def create(algo, ext):
        cfg = E.make_config(algo, 11, 3, 32, 16)
        return lib.rle_create_ext(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(out))

    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        assert create(E.RLE_TD3, E.make_config_ext(bc_alpha=bad)) == -1, bad
        assert b"bc_alpha" in lib.rle_last_error()
    for algo in (E.RLE_TD7, E.RLE_SAC):
        assert create(algo, E.make_config_ext(bc_alpha=2.5)) == -1, algo
        assert b"bc_alpha" in lib.rle_last_error()
    for size in (0, -4, 4, E.ConfigExt.bc_alpha.offset, ctypes.sizeof(E.ConfigExt) - 1):
        ext = E.make_config_ext(bc_alpha=2.5)
        ext.size = size
        assert create(E.RLE_TD3, ext) == -1, size
        assert b"bc_alpha" in lib.rle_last_error()
    # (rle_config's own validation is unchanged behind the new entry: bc_lambda stays TD7's)
    cfg = E.make_config(E.RLE_TD3, 11, 3, 32, 16, bc_lambda=0.1)
    ext = E.make_config_ext()
    assert lib.rle_create_ext(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(out)) == -1
    assert b"bc_lambda" in lib.rle_last_error()
    assert lib.rle_create_ext(ctypes.byref(cfg), None, ctypes.byref(out)) == -1
    assert lib.rle_create_ext(None, None, ctypes.byref(out)) == -1


def test_normalisation_entries_reject_null_pointers_before_any_hip_call():
    """rle_replay_state_stats / rle_replay_normalize_states with a NULL replay or a NULL vector: RLE_EINVAL."""
    from rl import _engine as E

    lib = E.lib()
    v = np.ones(4, np.float32)
    p = v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.rle_replay_state_stats(None, p, p) == -1
    assert b"state_stats" in lib.rle_last_error()
    assert lib.rle_replay_normalize_states(None, p, p) == -1
    assert b"normalize_states" in lib.rle_last_error()
