"""The random streams' host reference (tests/philox_ref.py), checked without a GPU: the Philox core against the
Random123 known-answer vectors, the separation of the streams that share a key, the distribution of every
stream, and how sharply the CPU oracle's losses tell a right noise tape from a wrong one (the condition under
which tests/test_rng_streams_gpu.py's engine-against-engine test means anything).

Statistical thresholds follow from the sample size N = 2^20 alone: a mean within 5 / sqrt(N) and a variance
within 5 sqrt(2 / N) (five standard errors of a unit normal's), a Kolmogorov distance below 1.95 / sqrt(N) (the
0.1% point of Kolmogorov's distribution), a correlation within 5 / sqrt(N).
"""

import math

import numpy as np
import pytest
import torch

import philox_ref as P
import rng_cases as R

N = 1 << 20
SEEDS = [12345, (1 << 40) | 12345, (0xDEADBEEF << 32) | 0x9E3779B9]


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("key,ctr,out", [
    ((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 2, (0xFFFFFFFF,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(key, ctr, out):
    assert _hex(P.philox4x32_10(key, ctr)) == out
    # vectorised: the same answer in every lane of an array call
    lanes = P.philox4x32_10(key, tuple(np.full(5, c, np.uint64) for c in ctr))
    assert all(_hex(w[i] for w in lanes) == out for i in range(5))


def test_float_maps():
    assert P.u01(0) == 0.0 and P.u01(0xFFFFFFFF) == np.float32(1.0 - 2.0 ** -24) and P.u01(0x100) == np.float32(2.0 ** -24)
    assert P.u01(np.arange(0, 1 << 32, 99991, dtype=np.uint64)).dtype == np.float32
    u1, u2 = P.box_muller_uniforms(np.array([0, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF]))
    assert u1.tolist() == [2.0 ** -24, 1.0] and u2.tolist() == [0.0, 1.0 - 2.0 ** -24]
    assert P.normal(0, 0) == math.sqrt(48 * math.log(2.0))  # the largest draw: u1 = 2^-24, cos(0)
    assert P.normal(0xFFFFFFFF, 12345) == 0.0  # u1 = 1
    assert abs(P.normal(0, 0x80000000) + math.sqrt(48 * math.log(2.0))) < 1e-12
    assert P.key_of((7 << 32) | 9) == (9, 7)
    assert P.act_key(0) == P.key_of(P.ACT_KEY_ADD) and P.act_key(1) == P.key_of((P.ACT_KEY_MUL + P.ACT_KEY_ADD) % (1 << 64))


def test_same_key_streams_never_share_a_counter():
    """u and the step noise share cfg.seed's key, the three fill draws the fill seed's: within each group a
    constant counter word differs, whatever the element and the step / row -- so no two draws of a group come
    from one Philox block.  The act stream has another key."""
    rng = np.random.default_rng(1)
    idx = rng.integers(0, 1 << 17, 4096)
    steps = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) + 12345] + rng.integers(0, 1 << 62, 16).tolist()
    for s in steps:
        cu, ce = P.u_counter(idx, s), P.eps_counter(idx, s)
        assert np.all(np.asarray(cu[1]) == 0) and np.all(np.asarray(ce[1]) == 1)
        assert (cu[2], cu[3]) == (s & 0xFFFFFFFF, s >> 32) == (ce[2], ce[3])  # no carry lost
    rows = np.concatenate([idx, rng.integers(0, 1 << 40, 64)])
    zs = [np.asarray(P.fill_counter(rows, idx[:rows.size] % 128, z)[2]) for z in (P.Z_FILL_STATE, P.Z_FILL_ACTION, P.Z_FILL_REWARD)]
    assert [np.unique(z).tolist() for z in zs] == [[7], [8], [9]]
    c = P.fill_counter(rows, 0, 9)
    assert np.array_equal(c[0] + (c[3] << np.uint64(32)), rows.astype(np.uint64))
    for seed in SEEDS + [c.cfg_seed for c in R.CASES.values()]:
        assert P.act_key(seed) != P.key_of(seed)
    # and the blocks do differ: same element, same step, the two streams' first words
    a = P.philox4x32_10(P.key_of(5), P.u_counter(idx, 3))[0]
    b = P.philox4x32_10(P.key_of(5), P.eps_counter(idx, 3))[0]
    assert not np.any(a == b)


def _phi(x):
    return (0.5 * (1.0 + torch.special.erf(torch.from_numpy(x) / math.sqrt(2.0)))).numpy()


def _kolmogorov(cdf_sorted):
    n = cdf_sorted.size
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - cdf_sorted).max(), (cdf_sorted - (i - 1) / n).max()))


def _check_normal(x, what):
    x = np.asarray(x, np.float64).ravel()
    assert x.size == N
    d = _kolmogorov(_phi(np.sort(x)))
    print(f"RNG {what}: mean {x.mean():+.2e} var-1 {x.var() - 1:+.2e} kolmogorov {d:.2e} (bound {1.95 / math.sqrt(N):.2e})")
    assert abs(x.mean()) < 5 / math.sqrt(N), what
    assert abs(x.var() - 1.0) < 5 * math.sqrt(2.0 / N), what
    assert d < 1.95 / math.sqrt(N), what


def _check_uniform(u, what):
    u = np.asarray(u, np.float64).ravel()
    assert u.size == N and u.min() >= 0.0 and u.max() < 1.0
    d = _kolmogorov(np.sort(u))
    print(f"RNG {what}: kolmogorov {d:.2e}")
    assert d < 1.95 / math.sqrt(N), what


def _check_uncorrelated(a, b, what):
    c = float(np.corrcoef(np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel())[0, 1])
    print(f"RNG corr {what}: {c:+.2e}")
    assert abs(c) < 5 / math.sqrt(N), what


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_streams_are_standard_normal_uniform_and_uncorrelated(seed):
    """N = 2^20 draws of each stream: elements 0 .. 2^20 - 1 of one step / one act call (the reference has no
    row limit), 2^16 fill rows of 16 columns."""
    B, A = N // 4, 4
    step = 1000 + (seed & 0xFF)
    eps, eps2 = P.step_eps(seed, step, B, A)
    eps_next, _ = P.step_eps(seed, step + 1, B, A)
    u = P.step_u(seed, step, N)
    act, act_next = P.act_eps(seed, 77, B, A), P.act_eps(seed, 78, B, A)
    fill = P.fill_rows(seed, N // 16, 16, 16)
    _check_normal(eps, "eps")
    _check_normal(eps2, "eps2")
    _check_normal(act, "act")
    _check_normal(fill["state"], "fill state")
    _check_normal(fill["next_state"], "fill next_state")
    _check_uniform(u, "u")
    _check_uniform((fill["action"].astype(np.float64) + 1.0) / 2.0, "fill action")
    _check_uncorrelated(eps, eps2, "eps / eps2 of one step")
    _check_uncorrelated(u[:B], eps[:, 0], "u[b] / eps[b, 0] of one step")
    _check_uncorrelated(eps, eps_next, "eps of steps t / t + 1")
    _check_uncorrelated(act, act_next, "act draws at ctr / ctr + 1")
    _check_uncorrelated(fill["state"], fill["next_state"], "fill state / next_state")
    _check_uncorrelated(act, eps, "act / eps")


def test_fill_reward_and_notdone():
    f = P.fill_rows(SEEDS[1], N, 1, 1)
    _check_normal(f["reward"], "fill reward")
    p = float(f["notdone"].mean())  # Bernoulli(0.99): five standard errors
    assert abs(p - 0.99) < 5 * math.sqrt(0.99 * 0.01 / N), p
    assert np.all(f["priority"] == 1.0)
    # rows by number: the same draws, and the high word of a row past 2^32 is used
    g = P.fill_rows(SEEDS[1], np.array([5, 5 + (1 << 32)]), 3, 2)
    assert np.array_equal(g["state"][0], P.fill_rows(SEEDS[1], 6, 3, 2)["state"][5])
    assert not np.array_equal(g["state"][0], g["state"][1])


def test_tapes_layout():
    tp = P.tapes("sac", SEEDS[1], (1 << 32) - 1, 3, 5, 3)
    assert {k: (v.shape, v.dtype) for k, v in tp.items()} == {
        "u": ((3, 5), np.float32), "eps": ((3, 5, 3), np.float32), "eps_pi": ((3, 5, 3), np.float32)}
    e, e2 = P.step_eps(SEEDS[1], 1 << 32, 5, 3)  # (the second step: across the carry)
    assert np.array_equal(tp["eps"][1], e.astype(np.float32)) and np.array_equal(tp["eps_pi"][1], e2.astype(np.float32))
    assert np.array_equal(tp["u"][2], P.step_u(SEEDS[1], (1 << 32) + 1, 5))
    assert "eps_pi" not in P.tapes("td3", 1, 0, 1, 2, 2)
    # element e = b * A + j with the unpadded A: a wider action space continues the row-major stream
    assert np.array_equal(P.step_eps(9, 4, 4, 6)[0].ravel(), P.step_eps(9, 4, 8, 3)[0].ravel())


@pytest.mark.parametrize("case", list(R.CASES))
def test_oracle_losses_tell_a_wrong_noise_tape(case):
    """The engine-against-engine test of tests/test_rng_streams_gpu.py compares info rows within T (derived in
    rng_cases.reference from the oracle's response to a jitter of DELTA).  That bound is only a check of the noise
    streams if a wrong stream moves the infos far more: every mutation of rng_cases.mutations must move some info
    entry by at least 10 T on the float32 oracle."""
    ref = R.reference(case)
    worst = {}
    for name, tp in R.mutations(case, ref["tapes"]).items():
        worst[name] = R.rel_move(R.oracle_table(case, tp), ref["table"])
    print(f"RNG discrimination {case}: r {ref['r']:.2e} T {ref['T']:.2e} smallest effect {min(worst.values()):.2e} {worst}")
    assert min(worst.values()) >= 10 * ref["T"], (ref["T"], worst)
