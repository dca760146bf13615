"""TD7 offline mode (rle_config bc_lambda, TD7(offline=True)): the CPU side.

The oracle's restatement with the behaviour-cloning term (tests/offline_oracle.py) is pinned against the
online oracle, the term is shown to matter at the larger test weight, and the ABI carries and validates
the new field without a GPU.
"""

import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from offline_oracle import build_offline
from oracle import agents
from test_oracle import build_from_golden

torch.set_num_threads(1)

LMBDA_BIG = 5.0  # the larger test weight (the paper's 0.1 is the other)


def _state(orc):
    out = {}
    for net, d in orc.nets().items():
        for k, v in d.items():
            out[f"{net}.{k}"] = v.detach().numpy().copy()
    out.update(agents.moments(orc))
    return out


def test_bc_oracle_with_lmbda_zero_is_the_online_oracle_bitwise():
    """8 steps of the td7_tiny shape: info, every parameter and every Adam moment of TD7BCOracle(lmbda=0)
    equal oracle.agents.TD7Oracle's bit for bit -- the restated step is the online step plus the term."""
    g = load_golden("td7_tiny")
    alg, on, rep_on, tp, _, B = build_from_golden(g)
    off, rep_off, _, _, _ = build_offline(g, 0.0)
    i_on, ind_on = agents.run_steps(on, alg, rep_on, tp, 8, B)
    i_off, ind_off = agents.run_steps(off, alg, rep_off, tp, 8, B)
    for a, b in zip(ind_on, ind_off):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(i_on, i_off):
        for k in a:
            assert a[k] == b[k], k
        assert b["train/bc"] is None and b["train/q_abs"] is None
    s_on, s_off = _state(on), _state(off)
    assert s_on.keys() == s_off.keys()
    for k in s_on:
        np.testing.assert_array_equal(s_on[k], s_off[k], err_msg=k)
    np.testing.assert_array_equal(rep_on.priority, rep_off.priority)


def test_bc_term_is_visible_at_the_larger_weight():
    """Sensitivity guard for the parity tests (Tiny shape, lmbda 5): on the first policy step the BC part is at
    least 10% of the norm of the full action gradient, and the actor's Adam m differs from the online oracle's
    by far more (100 x) than the 1e-4 |m| + 1e-4 max|m| the engine's moments are held to after that step."""
    g = load_golden("td7_tiny")
    alg, on, rep_on, tp, _, B = build_from_golden(g)
    off, rep_off, _, _, _ = build_offline(g, LMBDA_BIG)
    agents.run_steps(on, alg, rep_on, tp, 2, B)
    infos, _ = agents.run_steps(off, alg, rep_off, tp, 2, B)
    assert infos[0]["train/bc"] is None and infos[1]["train/bc"] is not None and infos[1]["train/q_abs"] > 0
    g_q, g_bc = off.last_action_grads
    assert float(g_bc.norm()) >= 0.1 * float((g_q + g_bc).norm()), (float(g_bc.norm()), float((g_q + g_bc).norm()))
    m_on, m_off = agents.moments(on), agents.moments(off)
    worst = 0.0
    for k in m_on:
        if k.startswith("policy.") and k.endswith(":m"):
            worst = max(worst, float(np.abs(m_on[k] - m_off[k]).max()) / (2e-4 * float(np.abs(m_on[k]).max())))
    print("actor m: online vs offline, in units of the parity bound:", worst)
    assert worst >= 100.0, worst


def test_bc_oracle_objective_is_the_issue_formula():
    """train/policy = -(sum q1 + q2) / (2B) + lmbda * q_abs * bc with the returned q_abs and bc."""
    g = load_golden("td7_tiny")
    alg, on, rep_on, tp, _, B = build_from_golden(g)
    off, rep_off, _, _, _ = build_offline(g, LMBDA_BIG)
    i_on, _ = agents.run_steps(on, alg, rep_on, tp, 2, B)
    i_off, _ = agents.run_steps(off, alg, rep_off, tp, 2, B)
    # (same nets and batches up to the first policy step: the Q part is the online objective)
    want = i_on[1]["train/policy"] + LMBDA_BIG * i_off[1]["train/q_abs"] * i_off[1]["train/bc"]
    np.testing.assert_allclose(i_off[1]["train/policy"], want, rtol=1e-6)


def test_config_carries_bc_lambda():
    from rl import _engine as E

    cfg = E.make_config(E.RLE_TD7, 11, 3, 32, 16)
    assert cfg.bc_lambda == 0.0
    cfg = E.make_config(E.RLE_TD7, 11, 3, 32, 16, bc_lambda=0.1)
    assert cfg.bc_lambda == pytest.approx(0.1)
    assert E.Config._fields_[-1][0] == "bc_lambda"  # (at the struct's end: rle.h)


def test_create_rejects_bad_bc_lambda_before_any_hip_call():
    """Negative, NaN, and > 0 with TD3 / SAC: RLE_EINVAL through the ABI on a host without a GPU."""
    from rl import _engine as E

    lib = E.lib()
    out = ctypes.c_void_p()
    for bad in (-0.1, float("nan"), float("inf")):
        cfg = E.make_config(E.RLE_TD7, 11, 3, 32, 16, bc_lambda=bad)
        assert lib.rle_create(ctypes.byref(cfg), ctypes.byref(out)) == -1, bad
        assert b"bc_lambda" in lib.rle_last_error()
    for algo in (E.RLE_TD3, E.RLE_SAC):
        cfg = E.make_config(algo, 11, 3, 32, 16, bc_lambda=0.1)
        assert lib.rle_create(ctypes.byref(cfg), ctypes.byref(out)) == -1, algo
        assert b"TD7" in lib.rle_last_error()
