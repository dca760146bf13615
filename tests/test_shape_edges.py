"""The shape-edge table (tests/edge_cases.py) on the host: the oracle is a valid reference at every case,
and rle_create's domain ends where include/rle.h says it does.  No GPU."""

import ctypes

import numpy as np
import pytest
import torch

from edge_cases import CASES, float64_oracle, moment_distance, reference
from oracle import agents, spec


@pytest.mark.parametrize("case", list(CASES))
def test_float32_oracle_agrees_with_float64(case):
    """The float32 oracle against its float64 run meets the criteria the engine is held to, with room to
    spare: the same draws; step 1's Adam first moments within 1e-5 of each tensor's max |m|; per-step
    losses rel 1e-3; end parameters every element within 2 lr n + 1e-4 and every element of every tensor
    within 1e-5.  A case that does not is no reference for the GPU sweep."""
    ref = reference(case)
    f32, f64 = ref["f32"], ref["f64"]
    n = CASES[case].n_steps
    for t in range(n):
        np.testing.assert_array_equal(f32["ind"][t], f64["ind"][t])
    assert set(f32["m"]) == set(f64["m"]) and f32["m"]
    worst = max(moment_distance(f32["m"][k], f64["m"][k]) for k in f64["m"])
    print(case, "step-1 moments: worst distance", worst)
    for k in f64["m"]:
        assert moment_distance(f32["m"][k], f64["m"][k]) <= 1e-5, k
    np.testing.assert_array_equal(np.isnan(f32["table"]), np.isnan(f64["table"]))
    np.testing.assert_allclose(f32["table"], f64["table"], rtol=1e-3, atol=0, equal_nan=True)
    tol = 2 * 3e-4 * n + 1e-4
    for key, v64 in f64["params"].items():
        d = np.abs(f32["params"][key].astype(np.float64) - v64)
        assert d.max() <= tol, (key, float(d.max()))
        assert (d <= 1e-5).all(), (key, float((d <= 1e-5).mean()), float(d.max()))
    assert np.isfinite(f64["table"][~np.isnan(f64["table"])]).all()


def test_float64_run_leaves_the_float32_oracle_as_it_was():
    before = agents._params, agents._tt
    with float64_oracle():
        assert agents._tt(np.zeros(2, np.float32)).dtype == torch.float64
        assert torch.zeros(1).dtype == torch.float64
    assert (agents._params, agents._tt) == before
    assert torch.get_default_dtype() == torch.float32
    assert agents._tt(np.zeros(2)).dtype == torch.float32
    assert all(v.dtype == torch.float32 for v in agents._params({"w": np.zeros(2)}).values())
    assert "Edge-v0" not in spec.TASKS


def test_table_covers_the_edges_it_names():
    """The quantities the step builder switches on, at their limits and one past them (engine.cpp's
    predicates restated on the table, so an edit of a case that moves it off its edge fails here)."""
    c = CASES
    assert c["td7-a32"].A == 32 and c["td7-a33"].A == 33 and c["td3-a33"].A == 33           # actor_pre: A <= 32
    assert 2 * c["sac-a24"].A == 48 and 2 * c["sac-a25"].A == 50                            # sac_fwd_fused: 2A <= 48
    assert c["td3-k48"].S + c["td3-k48"].A == 48 and c["td3-k49"].S == 49                   # prelayer_shape: K <= 48
    assert c["td3-a17"].A == 17                                                             # two-stage segment <= 16
    assert c["td7-h272"].H == 272 and c["td7-h272"].H % 16 == 0 and c["td7-h272"].zs_dim is None
    assert c["td7-odd"].H % 16 and c["td7-odd"].zs_dim != c["td7-odd"].H and c["td7-odd"].S % 16 == 1
    assert c["sac-h260"].H == 260 and c["td7-h512"].H == 512
    assert (c["td7-max_in"].S, c["td7-max_in"].A) == (1024, 128) == (c["sac-max_in"].S, c["sac-max_in"].A)
    assert {x.B for x in c.values()} >= {1, 15, 17, 31, 33, 1023}
    assert all(x.S == 1 and x.A == 1 and x.H == 4 for k, x in c.items() if k.endswith("-min"))
    assert len(c["td3-deep6"].hidden_sizes) == 6
    assert len({x.seed for x in c.values()}) == len(c)
    # wide_tiles: every row piece whole 64-row blocks (B pads to 16 rows first)
    r16 = lambda b: -(-b // 16) * 16  # noqa: E731
    assert r16(c["td7-w50"].B) == 64 == r16(c["sac-w50"].B) and c["td7-w50"].B == 50 == c["sac-w50"].B
    assert r16(c["td3-w100"].B) == 112 and r16(c["td3-w100"].B) % 64
    assert c["td7-w50"].H == c["sac-w50"].H == c["td3-w100"].H == 64                        # N % wide == 0 for 32, 64


def _create(cfg):
    from rl import _engine as E

    out = ctypes.c_void_p()
    rc = E.lib().rle_create(ctypes.byref(cfg), ctypes.byref(out))
    assert not out.value
    return rc, E.lib().rle_last_error()


BORDER = {
    "batch0": (dict(batch=0), b"batch"), "batch1025": (dict(batch=1025), b"batch"),
    "state0": (dict(state_dim=0), b"dims"), "state1025": (dict(state_dim=1025), b"state_dim <= 1024"),
    "action0": (dict(action_dim=0), b"dims"), "action129": (dict(action_dim=129), b"action_dim <= 128"),
    "hidden0": (dict(hidden=0), b"hidden"), "hidden6": (dict(hidden=6), b"multiple of 4"),
    "hidden516": (dict(hidden=516), b"hidden <= 512"),
    "zs6": (dict(zs_dim=6), b"zs_dim"), "zs516": (dict(zs_dim=516), b"zs_dim"),
}


@pytest.mark.parametrize("algo", ["td7", "td3", "sac"])
@pytest.mark.parametrize("which", list(BORDER))
def test_create_rejects_dims_outside_the_domain_before_any_hip_call(which, algo):
    """One step outside each bound of include/rle.h's rle_config: RLE_EINVAL with a message naming the
    limit, before rle_create touches a device (so this runs on a host without a GPU)."""
    from rl import _engine as E

    fields, msg = BORDER[which]
    if "zs_dim" in fields and algo != "td7":
        fields, msg = dict(zs_dim=32), b"TD7 only"  # a legal TD7 value: the field itself is TD7's
    cfg = E.make_config({"td7": E.RLE_TD7, "td3": E.RLE_TD3, "sac": E.RLE_SAC}[algo], 17, 6, 32, 16)
    for k, v in fields.items():
        setattr(cfg, k, v)
    rc, err = _create(cfg)
    assert rc == -1 and msg in err, err


@pytest.mark.parametrize("algo", ["td3", "sac"])
def test_create_rejects_layer_lists_outside_the_domain_before_any_hip_call(algo):
    from rl import _engine as E

    code = {"td3": E.RLE_TD3, "sac": E.RLE_SAC}[algo]
    for n_hidden in (1, 7, -1):
        cfg = E.make_config(code, 17, 6, 32, 16)
        cfg.n_hidden = n_hidden
        for i in range(8):
            cfg.hidden_sizes[i] = 32
        rc, err = _create(cfg)
        assert rc == -1 and b"n_hidden" in err, (n_hidden, err)
    for bad in (6, 0, 516, -4):
        for pos in (0, 2):
            hs = [32, 32, 32]
            hs[pos] = bad
            cfg = E.make_config(code, 17, 6, 32, 16, hidden_sizes=[32, 32, 32])
            cfg.hidden_sizes[pos] = bad
            cfg.hidden = hs[-1]
            rc, err = _create(cfg)
            assert rc == -1 and (b"hidden_sizes" in err or b"hidden" in err), (bad, pos, err)
    with pytest.raises(ValueError, match="2..6"):
        E.make_config(code, 17, 6, 32, 16, hidden_sizes=[32])
    with pytest.raises(ValueError, match="2..6"):
        E.make_config(code, 17, 6, 32, 16, hidden_sizes=[32] * 7)


def test_create_rejects_a_layer_list_for_td7_before_any_hip_call():
    from rl import _engine as E

    cfg = E.make_config(E.RLE_TD7, 17, 6, 32, 16, hidden_sizes=[32, 32])
    rc, err = _create(cfg)
    assert rc == -1 and b"TD3 / SAC only" in err, err
