"""LeakyReLU, SiLU and GELU as hidden activations, on the host: the oracle with the three torch functions
registered (tests/more_acts.py) reproduces the nine goldens the reference wrote, the Python mirror and the ABI
accept exactly the forms they document, and the shape-edge cases the GPU tests run are valid references.
No GPU."""

import ctypes
import functools

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn import functional as F

import more_acts
import test_oracle as TO
import test_shape_edges as TSE
from conftest import acts_of, load_golden
from more_acts import ACT_CASES, GOLDENS, NAMES

torch.set_num_threads(1)


# ---- the oracle against the reference's goldens ------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_matches_reference(name):
    """tests/test_oracle.py's check of a tiny golden, unchanged: indices, infos, priorities, Adam moments, TD7
    value bounds, end parameters."""
    TO.test_oracle_matches_reference(name)


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_bitwise_on_this_host(name):
    TO.test_oracle_bitwise_on_this_host(name)


def test_goldens_rotate_every_activation_through_every_role():
    seen = {"actor": set(), "critic": set(), "encoder": set()}
    for name in GOLDENS:
        g = load_golden(name)
        acts = acts_of(g)
        assert set(acts) == ({"actor", "critic", "encoder"} if name.startswith("td7") else {"actor", "critic"})
        assert set(acts.values()) <= set(NAMES)
        H, B, ncap, n_fill, n_steps = (int(x) for x in g["meta"][:5])
        assert (H, B, ncap, n_fill) == (32, 16, 64, 50) and 6 <= n_steps <= 8
        for alg in ("td7", "td3", "sac"):
            if name.startswith(alg):
                for role, a in acts.items():
                    seen[role].add((alg, a))
    for role, s in seen.items():
        algs = ("td7",) if role == "encoder" else ("td7", "td3", "sac")
        assert s == {(alg, a) for alg in algs for a in NAMES}, (role, s)


# ---- the forms the mirror accepts and refuses --------------------------------------------------------------------

ACCEPTED = [(nn.LeakyReLU(), "leaky_relu"), (nn.LeakyReLU(0.01), "leaky_relu"), (F.leaky_relu, "leaky_relu"),
            (nn.SiLU(), "silu"), (F.silu, "silu"), (nn.GELU(), "gelu"), (nn.GELU(approximate="none"), "gelu"),
            (F.gelu, "gelu")]


@pytest.mark.parametrize("fn,name", ACCEPTED, ids=[f"{n}-{i}" for i, (_, n) in enumerate(ACCEPTED)])
def test_act_name_accepts_the_documented_forms(fn, name):
    from rl._engine import ACT_CODES
    from rl.nn.modules import _act_name

    assert _act_name(fn) == name
    assert ACT_CODES[name] == {"leaky_relu": 4, "silu": 5, "gelu": 6}[name]


REFUSED = [nn.LeakyReLU(0.2), nn.GELU(approximate="tanh"), nn.Softplus(), nn.Tanh(), torch.tanh, nn.ELU(0.5),
           functools.partial(F.leaky_relu, negative_slope=0.01), functools.partial(F.gelu, approximate="tanh"), F.mish]


@pytest.mark.parametrize("fn", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_act_name_refuses_everything_else(fn):
    from rl.nn.modules import _act_name

    with pytest.raises(NotImplementedError, match="ReLU, ELU"):
        _act_name(fn)


def test_nets_from_make_nn_reads_the_new_activations():
    from rl.nn import MLPActor, MLPCritic, SALEActor, SALECritic, SALEEncoder
    from rl.nn.modules import nets_from_make_nn

    def mk7(state_dim, action_dim, **kw):
        return (SALEActor(state_dim, action_dim, 32, 32, activ=F.silu),
                SALECritic(state_dim, action_dim, 32, 32, activ=F.gelu),
                SALECritic(state_dim, action_dim, 32, 32, activ=nn.GELU()),
                SALEEncoder(state_dim, action_dim, 32, 32, activ=nn.LeakyReLU()))

    def mk3(state_dim, action_dim, **kw):
        return (MLPActor(state_dim, action_dim, 32, action_fn="GELU"),
                MLPCritic(state_dim, action_dim, 32, action_fn="SiLU"),
                MLPCritic(state_dim, action_dim, 32, action_fn=nn.SiLU()))

    def mks(state_dim, action_dim, **kw):
        return (MLPActor(state_dim, 2 * action_dim, [48, 32], action_fn="LeakyReLU"),
                MLPCritic(state_dim, action_dim, [48, 32], action_fn=nn.GELU()),
                MLPCritic(state_dim, action_dim, [48, 32], action_fn="GELU"))

    assert nets_from_make_nn("td7", mk7, 11, 3, {})[3] == {"act_actor": "silu", "act_critic": "gelu",
                                                            "act_encoder": "leaky_relu"}
    assert nets_from_make_nn("td3", mk3, 11, 3, {})[3] == {"act_actor": "gelu", "act_critic": "silu"}
    assert nets_from_make_nn("sac", mks, 11, 3, {})[3] == {"act_actor": "leaky_relu", "act_critic": "gelu"}

    def slope(state_dim, action_dim, **kw):
        return (MLPActor(state_dim, action_dim, 32, action_fn=nn.LeakyReLU(0.2)),
                MLPCritic(state_dim, action_dim, 32), MLPCritic(state_dim, action_dim, 32))

    with pytest.raises(NotImplementedError, match="ReLU, ELU"):
        nets_from_make_nn("td3", slope, 11, 3, {})

    def twins(state_dim, action_dim, **kw):
        return (MLPActor(state_dim, action_dim, 32), MLPCritic(state_dim, action_dim, 32, action_fn="SiLU"),
                MLPCritic(state_dim, action_dim, 32, action_fn="GELU"))

    with pytest.raises(NotImplementedError, match="one activation for both critics"):
        nets_from_make_nn("td3", twins, 11, 3, {})


def test_make_config_names():
    from rl import _engine as E

    cfg = E.make_config(E.RLE_TD7, 11, 3, 32, 16, act_actor="silu", act_critic="gelu", act_encoder="leaky_relu")
    assert (cfg.act_actor, cfg.act_critic, cfg.act_encoder) == (5, 6, 4)
    for bad in ("mish", "tanh", "GELU", "leaky"):
        with pytest.raises(ValueError, match="activation"):
            E.make_config(E.RLE_TD3, 11, 3, 32, 16, act_critic=bad)


# ---- the ABI's validation, before any device call ----------------------------------------------------------------

def _create(cfg):
    from rl import _engine as E

    out = ctypes.c_void_p()
    rc = E.lib().rle_create(ctypes.byref(cfg), ctypes.byref(out))
    err = E.lib().rle_last_error()
    if out.value:  # (a host with a GPU: the engine was made)
        E.lib().rle_destroy(out)
    return rc, err


@pytest.mark.parametrize("field", ["act_actor", "act_critic", "act_encoder"])
@pytest.mark.parametrize("code", [4, 5, 6])
def test_create_takes_codes_4_to_6(code, field):
    """Codes 4..6 pass rle_create's validation: whatever it then returns (no device on this host, or an
    engine), it is not the activation error."""
    from rl import _engine as E

    cfg = E.make_config(E.RLE_TD7, 11, 3, 32, 16)
    setattr(cfg, field, code)
    rc, err = _create(cfg)
    assert rc == 0 or b"activation" not in err, err


@pytest.mark.parametrize("code", [7, -1, 8, 100])
def test_create_rejects_other_codes_before_any_hip_call(code):
    from rl import _engine as E

    for algo, field in ((E.RLE_TD7, "act_encoder"), (E.RLE_TD3, "act_critic"), (E.RLE_SAC, "act_actor")):
        cfg = E.make_config(algo, 11, 3, 32, 16)
        setattr(cfg, field, code)
        rc, err = _create(cfg)
        assert rc == -1 and b"activation" in err, err


def test_act_encoder_stays_td7_only():
    from rl import _engine as E

    cfg = E.make_config(E.RLE_TD3, 11, 3, 32, 16)
    cfg.act_encoder = 5
    rc, err = _create(cfg)
    assert rc == -1 and b"act_encoder" in err, err


# ---- the GPU tests' edge cases are valid references --------------------------------------------------------------

def test_edge_cases_name_their_sources_and_seeds():
    import edge_cases as EC

    assert [s for _, _, s in ACT_CASES.values()][:1] == [301]
    for i, (name, (src, acts, seed)) in enumerate(ACT_CASES.items()):
        assert src in EC.CASES and name not in EC.CASES
        assert (seed - (301 + i)) % 100 == 0 and seed >= 301 + i, (name, seed)
        assert set(acts.values()) <= set(NAMES)
        assert "encoder" not in acts or EC.CASES[src].alg == "td7"
    assert len({s for _, _, s in ACT_CASES.values()} | {c.seed for c in EC.CASES.values()}) == \
        len(ACT_CASES) + len(EC.CASES)


@pytest.mark.parametrize("case", list(ACT_CASES))
def test_float32_oracle_agrees_with_float64(case):
    """tests/test_shape_edges.py's host criteria, unchanged, on each case of the GPU tests."""
    more_acts.reference(case)
    with more_acts.registered(case):
        TSE.test_float32_oracle_agrees_with_float64(case)
