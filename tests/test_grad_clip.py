"""Gradient-norm clipping (rle_set_grad_clip, clip_grad_norm=): the CPU side.

The clipping wrapper of the CPU oracles (tests/grad_clip_oracle.py) is pinned bitwise to
torch.nn.utils.clip_grad_norm_, every case of tests/grad_clip_cases.py is shown to clip where its table says and
to be a valid reference (float32 against float64 under the engine's criteria), and the ABI and the Python
classes carry and validate the setting without a GPU.
"""

import copy
import ctypes
import math
import pickle

import numpy as np
import pytest
import torch

import grad_clip_cases as C
import grad_clip_oracle as GO

torch.set_num_threads(1)


# ---- the oracle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [0.05, 1.0, 7.0, 1e9])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_clipped_is_torch_clip_grad_norm_bitwise(max_norm, dtype):
    gen = torch.Generator().manual_seed(3)
    shapes = [(36, 50), (36,), (1, 36), (1,), (260, 260)]
    for scale in (1e-3, 1.0, 40.0):
        ps = [torch.nn.Parameter(torch.zeros(s, dtype=dtype)) for s in shapes]
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=gen, dtype=torch.float64) * scale).to(dtype)
        grads = [p.grad.clone() for p in ps]
        total_t = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=False)
        got, total, coef = GO.clipped(grads, max_norm)
        assert total.dtype == dtype and torch.equal(total, total_t)
        assert float(coef) == min(1.0, float(max_norm / (total + 1e-6)))
        for a, p in zip(got, ps):
            assert torch.equal(a, p.grad)


def test_clipped_propagates_a_nonfinite_norm_as_torch_does():
    for bad in (float("nan"), float("inf")):
        ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
        ps[0].grad, ps[1].grad = torch.tensor([1.0, bad, 2.0]), torch.tensor([0.5, -1.0])
        grads = [p.grad.clone() for p in ps]
        torch.nn.utils.clip_grad_norm_(ps, 1.0, error_if_nonfinite=False, foreach=False)
        got, total, coef = GO.clipped(grads, 1.0)
        for a, p in zip(got, ps):
            np.testing.assert_array_equal(a.numpy(), p.grad.numpy())  # (NaN == NaN here)
        assert not math.isfinite(float(total))


def test_wrapper_logs_every_clipped_optimizer_and_leaves_the_temperature_alone():
    orc, rep, tp, n, B, alg, keys, lap = C.build("clip-sac-a25")
    log = GO.clip(orc, 10.0)
    plain_t = orc.opt_t.step
    from oracle import agents

    agents.run_steps(orc, alg, rep, tp, 2, B)
    assert [x[0] for x in log] == ["critics", "policy"] * 2
    assert orc.opt_t.step == plain_t and orc.opt_t.t == 2
    orc7 = C.build("clip-td7-odd")[0]
    assert set(GO.NAMES) == {"opt_q", "opt_pi", "opt_enc"} and all(hasattr(orc7, a) for a in GO.NAMES)


# ---- the cases --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.CLIP_CASES))
def test_case_clips_where_its_table_says(name):
    """From the clipped float32 oracle's log: an update with coef < 1 in every case, one with coef == 1 too in the
    mixed ones; the logged optimizers are the algorithm's, in the same order clipped or not; unclipped, every coef is 1."""
    c = C.CLIP_CASES[name]
    ref = C.reference(name)
    coefs = [co for step in ref["f32"]["log"] for _, _, co in step]
    q = [co for step in ref["f32"]["log"] for o, _, co in step if o == "critics"]
    assert min(coefs) < 1.0
    if c.mixed:
        assert min(q) < 1.0 and max(q) == 1.0
    names = {o for step in ref["f32"]["log"] for o, _, _ in step}
    assert names == ({"critics", "policy", "encoder"} if C.alg_of(name) == "td7" else {"critics", "policy"})
    assert all(co == 1.0 for step in ref["plain"]["log"] for _, _, co in step)
    for a, b in zip(ref["f32"]["log"], ref["plain"]["log"]):
        assert [x[0] for x in a] == [x[0] for x in b]


@pytest.mark.parametrize("name,norm", [("clip-td3bc-odd", C.TD3BC_NORM), ("clip-awac-b17", C.AWAC_NORM)])
def test_offline_thresholds_are_half_the_median_unclipped_critics_norm(name, norm):
    totals = [t for step in C.reference(name)["plain"]["log"] for o, t, _ in step if o == "critics"]
    half = float(np.median(totals)) / 2
    assert norm == float(f"{half:.1g}") == C.CLIP_CASES[name].max_norm, (half, norm)


@pytest.mark.parametrize("name", list(C.CLIP_CASES))
def test_clipped_float32_oracle_agrees_with_float64(name):
    """The host criteria of tests/test_shape_edges.py on the clipped runs: the same draws; the Adam moments behind
    the engine's moment check within 1e-5 of each tensor's max; per-step losses rel 1e-3; end parameters every
    element within 2 lr n + 1e-4 and within 1e-5; and the clip log (total, coef) rel 1e-3."""
    ref = C.reference(name)
    f32, f64 = ref["f32"], ref["f64"]
    n = f32["n"]
    for t in range(n):
        np.testing.assert_array_equal(f32["ind"][t], f64["ind"][t])
    for key in ("m", "m2"):
        if f64[key] is None:
            continue
        assert set(f32[key]) == set(f64[key]) and f32[key]
        for k in f64[key]:
            assert f64[key][k].dtype == np.float64 and f32[key][k].dtype == np.float32
            d = C.EC.moment_distance(f32[key][k], f64[key][k])
            assert d <= 1e-5, (k, d)
        assert C.moment_shortfalls(lambda k: f32[key][k], f64[key]) == []
    np.testing.assert_array_equal(np.isnan(f32["table"]), np.isnan(f64["table"]))
    np.testing.assert_allclose(f32["table"], f64["table"], rtol=1e-3, atol=0, equal_nan=True)
    tol = 2 * 3e-4 * n + 1e-4
    for key, v64 in f64["params"].items():
        d = np.abs(f32["params"][key].astype(np.float64) - v64)
        assert d.max() <= tol, (key, float(d.max()))
        assert (d <= 1e-5).all(), (key, float((d <= 1e-5).mean()), float(d.max()))
    for t in range(n):
        np.testing.assert_allclose(C.stats_after(f32, t), C.stats_after(f64, t), rtol=1e-3, atol=0, equal_nan=True)


def test_unclipped_moments_miss_the_criterion_of_the_clipped_oracle():
    """What the GPU test of the same name relies on: at clip-sac-h260 the unclipped oracle's critic moments are
    about 6 x the clipped ones, far outside the moment bound."""
    ref = C.reference("clip-sac-h260")
    bad = C.moment_shortfalls(lambda k: ref["plain"]["m"][k], ref["f32"]["m"])
    assert any(k.startswith("q1.") and k.endswith(":m") and worst > 1000 for k, _, worst in bad)
    k = "q1.mlp.0.weight:m"
    ratio = np.abs(ref["plain"]["m"][k]).max() / np.abs(ref["f32"]["m"][k]).max()
    assert 5.5 < ratio < 7.5, ratio


# ---- the ABI ----------------------------------------------------------------------------------------------

def test_ctypes_prototypes_of_the_new_entries():
    from rl import _engine as E

    lib = E.lib()
    vp, f32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    for name, args in (("rle_set_grad_clip", [vp, ctypes.c_float]), ("rle_get_grad_clip", [vp, f32p]),
                       ("rle_grad_clip_stats", [vp, f32p])):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, name
    # null handles are refused before any HIP call
    out = (ctypes.c_float * 6)()
    assert lib.rle_set_grad_clip(None, 1.0) == -1
    assert lib.rle_get_grad_clip(None, out) == -1
    assert lib.rle_grad_clip_stats(None, out) == -1
    hdr = open(E.__file__.rsplit("/sac-td3-td7_amd/", 1)[0] + "/include/rle.h").read()
    for decl in ("int rle_set_grad_clip(rle_engine* e, float max_norm);", "int rle_get_grad_clip(rle_engine* e, float* max_norm);",
                 "int rle_grad_clip_stats(rle_engine* e, float* out6);"):
        assert decl in hdr


# ---- the Python classes without a device -------------------------------------------------------------------

class _FakeEngine:
    """Stands in for rl._engine.Engine: keeps what the agent built it with and the threshold it was given."""

    made = []

    def __init__(self, cfg, plan=None, ext=None):
        self.cfg, self.ext, self.replay, self.clip = cfg, ext, None, None
        _FakeEngine.made.append(self)

    def set_grad_clip(self, max_norm):
        self.clip = max_norm

    def grad_clip_stats(self):
        return {"critics": (1.0, 0.5), "policy": (2.0, 1.0), "encoder": (3.0, 0.25)}

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


@pytest.mark.parametrize("alg", ["td7", "td3", "sac"])
def test_keyword_reaches_every_engine_the_agent_builds(classes, alg):
    cls = classes[alg]
    ag = cls("Tiny-v0", clip_grad_norm=0.7, **KW)
    assert ag.clip_grad_norm == 0.7 and ag.engine.clip == 0.7
    assert "_ext" not in ag.__dict__ and ag.engine.ext is None  # (not an extension field: _ext's content is pinned)
    ag2 = pickle.loads(pickle.dumps(ag))
    ag3 = copy.deepcopy(ag)
    ag._rebuild(48)
    for a in (ag, ag2, ag3):
        assert a.clip_grad_norm == 0.7 and a.engine.clip == 0.7
    assert set(ag.grad_clip_stats()) == ({"critics", "policy", "encoder"} if alg == "td7" else {"critics", "policy"})
    assert ag.grad_clip_stats()["critics"] == (1.0, 0.5)
    with pytest.raises(TypeError):  # keyword-only
        cls("Tiny-v0", 0.99, 3e-4, 3e-4, *([0.7] * 12))
    for bad in (-1.0, float("nan")):
        n = len(_FakeEngine.made)
        with pytest.raises(ValueError, match="clip_grad_norm"):
            cls("Tiny-v0", clip_grad_norm=bad, **KW)
        assert len(_FakeEngine.made) == n  # (refused before any engine)


@pytest.mark.parametrize("alg", ["td7", "td3", "sac"])
def test_default_and_older_pickles_train_unclipped(classes, alg):
    cls = classes[alg]
    plain = cls("Tiny-v0", **KW)
    assert plain.clip_grad_norm == math.inf and plain.engine.clip is None and "clip_grad_norm" not in plain.__dict__
    assert cls("Tiny-v0", clip_grad_norm=math.inf, **KW).engine.clip is None
    st = plain.__getstate__()
    assert "clip_grad_norm" not in st  # (what an agent pickled before the keyword existed holds)
    old = cls.__new__(cls)
    old.__setstate__(copy.deepcopy(st))
    assert old.clip_grad_norm == math.inf and old.engine.clip is None
    zero = cls("Tiny-v0", clip_grad_norm=0, **KW)  # (0: off, as rle_set_grad_clip reads it)
    assert zero.engine.clip == 0.0


def test_sac_max_grad_norm_alone_changes_nothing(classes):
    SAC = classes["sac"]
    ag = SAC("Tiny-v0", 0.99, 3e-4, 3e-4, -20.0, 2.0, 0.005, -1.0, False, 1.0, **KW)  # (the reference's positional form)
    assert ag.max_grad_norm == 1.0 and ag.clip_grad_norm == math.inf and ag.engine.clip is None
    assert "clip_grad_norm" in SAC.__doc__ or "clip_grad_norm" in (SAC.__init__.__doc__ or "")
