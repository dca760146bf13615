"""The device's own random streams against the host Philox reference (tests/philox_ref.py): what production and
bench.py run -- no tapes.

(a) the exploration normals read out directly (zeroed policy, sigma 2^-4: act_sample * 16 is the draw), through
    the n = 1 act chain and the n > 1 act graph, across the counter's carry and engine copies;
(b) the sampler's u, bit for bit through the index laws of oracle.replay, across the step counter's carry and a
    burst that replays the multi-step program;
(c) the step noise: an un-taped engine against an identical engine on the reference's tapes (the taped path is
    what every parity test pins to the oracle);
(d) fill_random.

Tolerances (tests/rng_cases.py, DESIGN.md "Random streams"): a device normal within DELTA of the float64
Box-Muller; u, indices, uniform actions, not-done flags and priorities exact; info rows within the relative T that
rng_cases.reference derives on the CPU oracle; priorities, value bounds and parameters as everywhere in the suite.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
import philox_ref as P  # noqa: E402
import rng_cases as R  # noqa: E402
from harness import ALGO  # noqa: E402
from oracle import replay as oreplay  # noqa: E402
from oracle import spec  # noqa: E402
from test_engine_gpu import assert_params_close  # noqa: E402

S, H = R.S, R.H
HI_SEED = (1 << 40) | 12345


# ---- (a) exploration normals ---------------------------------------------------------------------------------

def _act_engine(alg, A, seed, pseed=3):
    """An engine whose deterministic action is 0 (SAC: mean 0, log-std -4) whatever the observation."""
    eng = E.Engine(E.make_config(ALGO[alg], S, A, H, 32, seed=seed))
    for net, params in spec.agent_params(alg, S, A, H, pseed).items():
        for name, v in params.items():
            if net == "policy":
                v = np.zeros_like(v)
                if alg == "sac" and name == "mlp.4.bias":
                    v[A:] = -4.0
            eng.set_param(net, name, v)
    eng.set_action_map(1.0, 0.0, exploration_noise=2.0 ** -4)
    return eng


def _draw(eng, alg, obs):
    """One mode-1 call's draws, float64 [n, A]: exact for TD7 / TD3 (a power-of-two sigma, nothing clips at
    |normal| / 16 <= 0.36); SAC's through atanh (rng_cases.SAC_READOUT)."""
    out = eng.act_sample(obs, 1).astype(np.float64)
    if alg == "sac":
        return np.arctanh(out) * np.exp(4.0)
    return out * 16.0


def _check_draws(got, seed, ctr, alg, what):
    n, A = got.shape
    ref = P.act_eps(seed, ctr, n, A)
    d = np.abs(got - ref)
    i = int(d.argmax())
    x, y, _, _ = P.philox4x32_10(P.act_key(seed), P.act_counter(i, ctr))
    u1, u2 = P.box_muller_uniforms(x, y)
    bound = R.DELTA + (R.SAC_READOUT if alg == "sac" else 0.0)
    print(f"RNG delta {what} ctr {ctr} n {n} A {A}: max |dev - ref| {d.max():.3e} at element {i} "
          f"(u1 {float(u1):.9g}, u2 {float(u2):.9g}, ref {ref.ravel()[i]:+.6f}); bound {bound:.3e}")
    assert d.max() <= bound, (what, float(d.max()), i)


def _obs(n, k=0):
    return np.random.default_rng(100 + k).standard_normal((n, S)).astype(np.float32)


@pytest.mark.parametrize("alg,seed", [("td3", HI_SEED), ("td7", (0xFEDCBA98 << 32) | 0x76543210), ("sac", (7 << 32) | 3),
                                      ("td3", 12345)])
def test_act_draws_equal_the_reference(alg, seed):
    """n = 1 (the act chain), then 2, 17 and 1,024 rows (the act graph): one stream.  Each mode-1 call advances
    act_counter by exactly one; deterministic and taped calls leave it alone."""
    A = R.A
    eng = _act_engine(alg, A, seed)
    assert eng.act_counter() == 0
    ctr = 0
    for k, n in enumerate((1, 2, 17, 1024, 1, 17)):
        _check_draws(_draw(eng, alg, _obs(n, k)), seed, ctr, alg, f"{alg} n={n}")
        ctr += 1
        assert eng.act_counter() == ctr
        assert np.all(eng.act_sample(_obs(n, k), 0) == 0.0)  # (the zeroed policy; SAC: tanh(0))
        eng.act_sample(_obs(n, k), 2, np.ones((n, A), np.float32))
        assert eng.act_counter() == ctr
    # a one-row call and the first row of a 17-row call at the same counter: the same draws
    eng.set_act_counter(40)
    one = _draw(eng, alg, _obs(1)).copy()
    eng.set_act_counter(40)
    many = _draw(eng, alg, _obs(17)).copy()
    np.testing.assert_array_equal(one[0], many[0])


def test_act_draws_wide_action_space():
    """A = 128, n = 1,024: 131,072 draws of one call, element row * A + j with the unpadded A."""
    eng = _act_engine("td3", 128, HI_SEED)
    eng.set_act_counter(5)
    _check_draws(_draw(eng, "td3", _obs(1024)), HI_SEED, 5, "td3", "td3 A=128")
    _check_draws(_draw(eng, "td3", _obs(1)), HI_SEED, 6, "td3", "td3 A=128")


@pytest.mark.parametrize("alg", ["td3", "sac"])
def test_act_counter_carry_and_engine_copies(alg):
    """The counter's high word reaches the device (graph and chain), and a copied or rebuilt engine continues
    the stream where the first one stood."""
    seed = (0xABCD << 32) | 99
    eng = _act_engine(alg, R.A, seed)
    eng.set_act_counter(2 ** 32 - 1)
    for k, n in enumerate((17, 1, 17, 1)):  # counters 2^32 - 1 (graph), 2^32 (chain), 2^32 + 1, 2^32 + 2
        _check_draws(_draw(eng, alg, _obs(n)), seed, 2 ** 32 - 1 + k, alg, f"{alg} carry n={n}")
    assert eng.act_counter() == 2 ** 32 + 3
    copy = _act_engine(alg, R.A, seed)
    copy.copy_state_from(eng)  # (what copy.deepcopy of an agent does)
    assert copy.act_counter() == 2 ** 32 + 3
    _check_draws(_draw(copy, alg, _obs(2)), seed, 2 ** 32 + 3, alg, f"{alg} copied engine")
    rebuilt = _act_engine(alg, R.A, seed)
    rebuilt.set_act_counter(eng.act_counter())  # (what loading an agent's state does)
    _check_draws(_draw(rebuilt, alg, _obs(1)), seed, 2 ** 32 + 3, alg, f"{alg} rebuilt engine")
    _check_draws(_draw(eng, alg, _obs(1)), seed, 2 ** 32 + 3, alg, f"{alg} first engine")


# ---- (b) the sampler's u -------------------------------------------------------------------------------------

def _sampler_case(alg, B, seed, use_lap, **extra):
    return R.Case(alg, B, seed, 41, 0, use_lap, extra)


@pytest.mark.parametrize("B", [1, 17, 32])
def test_uniform_sampler_u_is_the_reference(B):
    seed = HI_SEED + B
    eng, rep = R.build_engine(_sampler_case("td3", B, seed, False))
    for t in range(4):
        step = int(eng.counters()[4])
        assert step == t
        eng.step(1)
        np.testing.assert_array_equal(eng.last_indices(), oreplay.uniform_indices(R.NCAP, P.step_u(seed, step, B)))
    # the step counter's carry: steps 2^32 - 2 .. 2^32 + 1
    c = eng.counters()
    c[4] = 2 ** 32 - 2
    eng.set_counters(c)
    for t in range(4):
        eng.step(1)
        assert int(eng.counters()[4]) == 2 ** 32 - 1 + t
        np.testing.assert_array_equal(eng.last_indices(),
                                      oreplay.uniform_indices(R.NCAP, P.step_u(seed, 2 ** 32 - 2 + t, B)))


@pytest.mark.parametrize("alg,B,seed", [("td7", 17, (5 << 32) | 1), ("td3", 32, 77), ("td7", 1, HI_SEED)])
def test_lap_sampler_u_is_the_reference(alg, B, seed):
    """Step t draws from the device's own priorities as they stood after step t - 1: the exact index law on exact
    inputs (TD7: a hard update after every third step)."""
    extra = {"target_update_rate": 3} if alg == "td7" else {}
    eng, rep = R.build_engine(_sampler_case(alg, B, seed, True, **extra))
    prio = rep.get_priority(R.NCAP)
    for t in range(7):
        eng.step(1)
        np.testing.assert_array_equal(eng.last_indices(), oreplay.lap_indices(prio, R.NCAP, P.step_u(seed, t, B)))
        prio = rep.get_priority(R.NCAP)
    c = eng.counters()
    c[4] = 2 ** 32 - 1
    eng.set_counters(c)
    for t in range(2):
        eng.step(1)
        np.testing.assert_array_equal(eng.last_indices(),
                                      oreplay.lap_indices(prio, R.NCAP, P.step_u(seed, 2 ** 32 - 1 + t, B)))
        prio = rep.get_priority(R.NCAP)


# (n: TD3's 16-step program from step 0; SAC's 8-step one; TD7's first step is no policy step, so its 6-step
# program starts at the second -- target_update_rate 250 keeps hard updates out of it)
@pytest.mark.parametrize("alg,n,extra", [("td3", 20, {}), ("sac", 11, {}), ("td7", 8, {"target_update_rate": 250})])
def test_burst_ends_on_the_reference_step(alg, n, extra):
    seed, B, step0 = (9 << 32) | 4, 17, 2 ** 32 - 5
    eng, rep = R.build_engine(_sampler_case(alg, B, seed, False, **extra))
    for s0 in (0, step0):  # (the second burst: across the carry)
        c = eng.counters()
        c[4] = s0
        eng.set_counters(c)
        eng.step(n)
        assert int(eng.counters()[4]) == s0 + n
        np.testing.assert_array_equal(eng.last_indices(), oreplay.uniform_indices(R.NCAP, P.step_u(seed, s0 + n - 1, B)))


# ---- (c) the step noise --------------------------------------------------------------------------------------

def _compare(case, X, Y, rx, ry, ix, iy, n, what):
    c = R.CASES[case]
    T = R.reference(case)["T"]
    k = len(R.INFO_KEYS[c.alg])
    ix, iy = np.asarray(ix, np.float64)[:, :k], np.asarray(iy, np.float64)[:, :k]
    np.testing.assert_array_equal(np.isnan(ix), np.isnan(iy))
    assert not np.isnan(iy).all(axis=0).any()
    with np.errstate(invalid="ignore"):
        rel = np.abs(ix - iy) / np.abs(iy)
    print(f"RNG noise {case} {what}: max relative info distance {np.nanmax(rel):.3e} (T {T:.3e}, r {R.reference(case)['r']:.3e})")
    assert np.nanmax(rel) <= T, (case, what, float(np.nanmax(rel)), T)
    np.testing.assert_array_equal(X.last_indices(), Y.last_indices())
    np.testing.assert_array_equal(X.counters()[:4], Y.counters()[:4])
    assert int(X.counters()[4]) == n
    if c.use_lap:
        np.testing.assert_allclose(rx.get_priority(R.NCAP), ry.get_priority(R.NCAP), rtol=1e-4, atol=1e-5)
    if c.alg == "td7":
        np.testing.assert_allclose(X.value_bounds(), Y.value_bounds(), rtol=1e-4, atol=1e-4)
    tol = 2 * 3e-4 * n + 1e-4
    for net, params in spec.agent_params(c.alg, S, R.A, H, c.pseed).items():
        for name, v in params.items():
            assert_params_close(X.get_param(net, name, v.shape), Y.get_param(net, name, v.shape), tol, (net, name), bulk=0.99)


@pytest.mark.parametrize("burst", [False, True], ids=["per_step", "burst"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_untaped_steps_equal_steps_on_the_reference_tapes(case, burst):
    """Engine X draws on the device; engine Y, built alike, reads rng_cases.ref_tapes.  Same kernels in the same
    order: they differ by the last bits of the draws alone."""
    c = R.CASES[case]
    n = c.n_steps
    tp = R.reference(case)["tapes"]
    X, rx = R.build_engine(case)
    Y, ry = R.build_engine(case)
    Y.set_tapes(u=tp["u"], eps=tp["eps"], eps_pi=tp.get("eps_pi"))
    if burst:
        ix, iy = X.step(n), Y.step(n)
    else:
        ix, iy = [], []
        for t in range(n):
            ix.append(X.step(1)[0])
            iy.append(Y.step(1)[0])
            np.testing.assert_array_equal(X.last_indices(), Y.last_indices())
    Y.set_tapes()
    _compare(case, X, Y, rx, ry, ix, iy, n, "burst" if burst else "per step")


# ---- (d) fill_random -----------------------------------------------------------------------------------------

def test_fill_random_equals_the_reference():
    n, Sf, Af, seed = 300, 17, 6, (0xBEEF << 32) | 0x80000000
    rep = E.Replay(n, Sf, Af, True)
    rep.fill_random(n, seed)
    assert rep.state() == (0, n, 1.0)
    s, a, r, s2, d, p = rep.export_rows(0, n, priority=True)
    ref = P.fill_rows(seed, n, Sf, Af)
    for got, key in ((s, "state"), (s2, "next_state"), (r, "reward")):
        err = np.abs(got.astype(np.float64) - ref[key])
        dist, i = float(err.max()), int(err.argmax())
        print(f"RNG delta fill {key}: max |dev - ref| {dist:.3e} at element {i} (ref {ref[key].ravel()[i]:+.6f}); "
              f"bound {R.DELTA:.3e}")
        assert dist <= R.DELTA, (key, dist)
    np.testing.assert_array_equal(a, ref["action"])
    np.testing.assert_array_equal(d, ref["notdone"])
    np.testing.assert_array_equal(p, ref["priority"])
    np.testing.assert_array_equal(rep.get_priority(n), ref["priority"])
    rep.fill_random(n, seed ^ (1 << 32))  # (another high word alone)
    s_b, a_b = rep.export_rows(0, n)[:2]
    other = P.fill_rows(seed ^ (1 << 32), n, Sf, Af)
    assert np.abs(s_b.astype(np.float64) - other["state"]).max() <= R.DELTA
    np.testing.assert_array_equal(a_b, other["action"])
    assert not np.array_equal(a_b, a) and np.abs(s_b - s).max() > 1.0
