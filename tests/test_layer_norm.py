"""LayerNorm critics on the host: the oracle composite is the mirror's module, the seven cases are valid
references, the mirror accepts what the engine runs and refuses the rest, and the agents' keyword reaches every
engine they build.  No GPU."""

import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch
from torch import nn

import layer_norm as LN
from edge_cases import moment_distance
from oracle import nets as N

ACTS = {"relu": "ReLU", "elu": "ELU", "identity": "Identity", "leaky_relu": "LeakyReLU", "silu": "SiLU", "gelu": "GELU"}


# ---- the composite is the mirror's LayerNorm critic ---------------------------------------------------------

@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("sizes", [[4, 4], [20, 36, 260]])
def test_composite_equals_the_mirror_critic_bitwise(act, sizes):
    """oracle.nets.mlp_critic with "ln_<act>" against rl.nn.MLPCritic(layer_norm=True): forward and the gradient
    with respect to the inputs, bit for bit; the state_dict names are those of a critic without the norm."""
    from rl.nn.modules import MLPCritic, NormAct

    torch.manual_seed(7)
    torch.set_num_threads(1)
    S, A, n = 5, 3, 19
    m = MLPCritic(S, A, sizes, layer_norm=True, action_fn=ACTS[act], init_bias="normal_")
    plain = MLPCritic(S, A, sizes, action_fn=ACTS[act])
    assert m.layer_norm and not plain.layer_norm and m.act == act
    assert list(m.state_dict()) == list(plain.state_dict()) == [f"mlp.{2 * i}.{p}" for i in range(len(sizes) + 1)
                                                                 for p in ("weight", "bias")]
    assert [type(x) for x in m.mlp][1::2] == [NormAct] * len(sizes) and isinstance(m.mlp[-1], nn.Linear)
    for i, w in enumerate(sizes):
        ln = m.mlp[2 * i + 1].norm
        assert ln.normalized_shape == (w,) and not ln.elementwise_affine and ln.eps == 1e-5
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    s = torch.randn(n, S, requires_grad=True)
    a = torch.randn(n, A, requires_grad=True)
    s2, a2 = s.detach().clone().requires_grad_(True), a.detach().clone().requires_grad_(True)
    q = m.estimate_q_value(s, a)
    q2 = N.mlp_critic(P, s2, a2, N.ACTS[LN.PREFIX + act])
    assert torch.equal(q, q2) and q.shape == (n, 1)
    q.square().sum().backward()
    q2.square().sum().backward()
    assert torch.equal(s.grad, s2.grad) and torch.equal(a.grad, a2.grad)
    assert not torch.equal(q, plain.estimate_q_value(s, a))


def test_normact_is_the_documented_formula():
    """act((z - mu) / sqrt(var + 1e-5)) with the biased variance, in float64, against the module."""
    from rl.nn.modules import NormAct

    torch.manual_seed(3)
    z = torch.randn(6, 20, dtype=torch.float64) * 3 + 1
    z[2] = 0.75  # a constant row: var 0, finite through eps
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    want = torch.nn.functional.elu((z - mu) / torch.sqrt(var + 1e-5))
    got = NormAct(20, nn.ELU()).double()(z)
    assert torch.allclose(got, want, rtol=0, atol=1e-12) and torch.isfinite(got).all()
    assert (got[2] == 0).all()


# ---- the cases are valid references -------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(LN.LN_CASES))
def test_float32_oracle_agrees_with_float64(case):
    """tests/test_shape_edges.py's host criteria on the LayerNorm cases: the same draws; step 1's Adam first
    moments within 1e-5 of each tensor's max |m|; losses rel 1e-3; end parameters within 2 lr n + 1e-4, every
    element within 1e-5."""
    ref = LN.reference(case)
    f32, f64 = ref["f32"], ref["f64"]
    assert str(ref["g"]["meta_acts"][1]) == LN.LN_CASES[case][1]
    n = len(f32["ind"])
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


def test_cases_differ_from_their_sources_and_registration_is_undone():
    """The norm changes what the oracle computes (so a GPU run without it cannot pass), and registered() leaves
    edge_cases and the oracle's activation table as they were."""
    import edge_cases as EC

    before = (dict(EC.CASES), EC.golden)
    ref = LN.reference("ln-td3-min")
    assert (dict(EC.CASES), EC.golden) == before
    with LN.registered("ln-td3-min"):
        assert "ln-td3-min" in EC.CASES and EC.CASES["ln-td3-min"].seed == 501
        g = EC.golden("ln-td3-min")
        assert list(g["meta_acts"]) == ["default", "ln_relu", "default"]
        assert list(LN.strip(g)["meta_acts"]) == ["default", "relu", "default"]
        assert "meta_acts" not in EC.golden("td3-min")
    assert (dict(EC.CASES), EC.golden) == before
    assert len({v[3] for v in LN.LN_CASES.values()}) == len(LN.LN_CASES)
    assert np.isfinite(ref["f32"]["table"][:, 0]).all()


# ---- the mirror: accepted and refused forms -----------------------------------------------------------------

def test_mirror_accepts_the_one_form_the_engine_runs():
    from rl.nn.modules import MLPCritic, nets_from_make_nn, MLPActor

    for form in (True, nn.LayerNorm(8, elementwise_affine=False), dict(elementwise_affine=False),
                 dict(elementwise_affine=False, eps=1e-5)):
        assert MLPCritic(3, 2, [8, 8], layer_norm=form).layer_norm
    for form in (False, None):
        assert not MLPCritic(3, 2, [8, 8], layer_norm=form).layer_norm

    def mk(state_dim, action_dim, ln=(True, True), out=None):
        return (MLPActor(state_dim, out or action_dim, [8, 12]), MLPCritic(state_dim, action_dim, [8, 12], layer_norm=ln[0]),
                MLPCritic(state_dim, action_dim, [8, 12], layer_norm=ln[1]))

    r = nets_from_make_nn("td3", mk, 3, 2, {})
    assert len(r) == 5 and r[4] is True and r[1] == {"hidden_sizes": [8, 12]}
    assert r[3] == {"act_actor": "relu", "act_critic": "relu"}
    assert list(r[2]["q1"]) == [f"mlp.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    assert nets_from_make_nn("td3", lambda **k: mk(ln=(False, False), **k), 3, 2, {})[4] is False
    assert nets_from_make_nn("sac", lambda **k: mk(out=4, **k), 3, 2, {})[4] is True
    with pytest.raises(NotImplementedError, match="both critics"):
        nets_from_make_nn("td3", lambda **k: mk(ln=(True, False), **k), 3, 2, {})


def test_mirror_refuses_what_the_engine_does_not_run():
    from rl.nn.modules import MLPActor, MLPCritic, SALEActor, SALECritic, SALEEncoder

    supported = "elementwise_affine=False.*eps 1e-5"
    with pytest.raises(NotImplementedError, match=supported):
        MLPActor(3, 2, [8, 8], layer_norm=True)
    with pytest.raises(NotImplementedError, match="affine.*" + supported):
        MLPCritic(3, 2, [8, 8], layer_norm=nn.LayerNorm(8))
    with pytest.raises(NotImplementedError, match="affine.*" + supported):
        MLPCritic(3, 2, [8, 8], layer_norm=dict(eps=1e-5))
    with pytest.raises(NotImplementedError, match="eps.*" + supported):
        MLPCritic(3, 2, [8, 8], layer_norm=nn.LayerNorm(8, eps=1e-6, elementwise_affine=False))
    with pytest.raises(NotImplementedError, match="eps.*" + supported):
        MLPCritic(3, 2, [8, 8], layer_norm=dict(elementwise_affine=False, eps=1e-3))
    with pytest.raises(NotImplementedError, match=supported):
        MLPCritic(3, 2, [8, 8], layer_norm="rms")
    for cls in (SALEActor, SALECritic, SALEEncoder):
        with pytest.raises(NotImplementedError, match="TD3 / SAC only.*" + supported):
            cls(3, 2, layer_norm=True)
        assert cls(3, 2, zs_dim=8, hdim=8) is not None


# ---- the ABI ------------------------------------------------------------------------------------------------

def test_signatures_hold_both_entries():
    from rl import _engine as E

    vp = ctypes.c_void_p
    assert E.SIGNATURES["rle_set_layer_norm"] == (ctypes.c_int, [vp, ctypes.c_int])
    assert E.SIGNATURES["rle_get_layer_norm"] == (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int)])
    lib = E.lib()
    for name in ("rle_set_layer_norm", "rle_get_layer_norm"):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == E.SIGNATURES[name][1]
    out = ctypes.c_int(7)
    assert lib.rle_set_layer_norm(None, 1) == -1  # (null handles are refused before any HIP call)
    assert lib.rle_get_layer_norm(None, ctypes.byref(out)) == -1
    hdr = open(E.__file__.rsplit("/sac-td3-td7_amd/", 1)[0] + "/include/rle.h").read()
    for decl in ("int rle_set_layer_norm(rle_engine* e, int critic);", "int rle_get_layer_norm(rle_engine* e, int* critic);"):
        assert decl in hdr


# ---- the agents' keyword without a device -------------------------------------------------------------------

class _FakeEngine:
    """Stands in for rl._engine.Engine: keeps what the agent built it with and the settings it was given."""

    made = []

    def __init__(self, cfg, plan=None, ext=None):
        self.cfg, self.ext, self.replay, self.clip, self.ln = cfg, ext, None, None, False
        _FakeEngine.made.append(self)

    def set_grad_clip(self, max_norm):
        self.clip = max_norm

    def set_layer_norm(self, critic=True):
        self.ln = bool(critic)

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
    ag = cls("Tiny-v0", critic_layer_norm=True, **KW)
    assert ag.critic_layer_norm is True and ag.engine.ln is True
    assert "_ext" not in ag.__dict__ and ag.engine.ext is None  # (not an extension field)
    ag2 = pickle.loads(pickle.dumps(ag))
    ag3 = copy.deepcopy(ag)
    ag._rebuild(48)
    for a in (ag, ag2, ag3):
        assert a.critic_layer_norm is True and a.engine.ln is True
    both = cls("Tiny-v0", critic_layer_norm=True, clip_grad_norm=0.5, **KW)  # (composes with clipping)
    assert both.engine.ln is True and both.engine.clip == 0.5
    with pytest.raises(TypeError):  # keyword-only
        cls("Tiny-v0", 0.99, 3e-4, 3e-4, *([True] * 13))


@pytest.mark.parametrize("alg", ["td3", "sac"])
def test_default_and_older_pickles_have_no_norm(classes, alg):
    cls = classes[alg]
    plain = cls("Tiny-v0", **KW)
    assert plain.critic_layer_norm is False and plain.engine.ln is False and "critic_layer_norm" not in plain.__dict__
    assert cls("Tiny-v0", critic_layer_norm=False, **KW).engine.ln is False
    st = plain.__getstate__()
    assert "critic_layer_norm" not in st  # (what an agent pickled before the keyword existed holds)
    old = cls.__new__(cls)
    old.__setstate__(copy.deepcopy(st))
    assert old.critic_layer_norm is False and old.engine.ln is False


def test_make_nn_critics_switch_the_agent_setting(classes):
    from rl.nn.modules import MLPActor, MLPCritic

    def mk(state_dim, action_dim, ln=True):
        return (MLPActor(state_dim, action_dim, [8, 12]), MLPCritic(state_dim, action_dim, [8, 12], layer_norm=ln),
                MLPCritic(state_dim, action_dim, [8, 12], layer_norm=ln))

    ag = classes["td3"]("Tiny-v0", make_nn=mk, batch_size=16, seed=1)
    assert ag.critic_layer_norm is True and ag.engine.ln is True
    assert pickle.loads(pickle.dumps(ag)).engine.ln is True
    assert classes["td3"]("Tiny-v0", make_nn=mk, batch_size=16, seed=1, ln=False).engine.ln is False
    with pytest.raises(ValueError, match="carry no LayerNorm"):
        classes["td3"]("Tiny-v0", make_nn=mk, batch_size=16, seed=1, ln=False, critic_layer_norm=True)


def test_td7_refuses_the_keyword(classes):
    TD7 = classes["td7"]
    n = len(_FakeEngine.made)
    with pytest.raises(TypeError, match="critic_layer_norm"):
        TD7("Tiny-v0", critic_layer_norm=True, **KW)
    assert len(_FakeEngine.made) == n
    assert TD7("Tiny-v0", **KW).engine.ln is False
