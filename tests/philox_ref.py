"""The engine's random streams restated in numpy (TEST INFRASTRUCTURE ONLY; no GPU import).

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
known-answer vectors pin it in tests/test_rng_streams.py), vectorised with uint64 arithmetic, and the two
float maps of kernels.hip:

* ``u01(x) = (x >> 8) / 2^24`` -- exact in float32.
* ``normal(a, b) = sqrt(-2 ln(((a >> 8) + 1) / 2^24)) * cos(2 pi (b >> 8) / 2^24)`` -- Box-Muller, computed
  here in float64 (the device uses the hardware's log2 and cosine units; this is the formula, not an
  imitation of them).  ``|normal| <= sqrt(48 ln 2) = 5.77``.

The stream map, read from kernels.hip (op_sample_gather, op_noise, act_noise, rle_fill_kernel) and
engine.cpp (fill_sample_args, act_args, rle_act_sample).  A key is a 64-bit seed as (low word, high word); a
counter is written (.x, .y, .z, .w) and the output words likewise:

* Step sampler ``u``: key ``cfg.seed``; counter ``(b, 0, step_lo, step_hi)``; ``u[b] = u01(.x)``, ``b < B``.
* Step noise: key ``cfg.seed``; counter ``(e = b * A + j, 1, step_lo, step_hi)`` with ``b < B`` and the
  unpadded ``A``; ``eps[b, j] = normal(.x, .y)`` (TD7 / TD3 target smoothing, SAC next-state rsample) and
  ``eps2[b, j] = normal(.z, .w)`` (SAC policy rsample).
* Act exploration: key ``cfg.seed * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D mod 2^64``; counter
  ``(row * A + j, 7, ctr_lo, ctr_hi)``; ``normal(.x, .y)``.  ``ctr`` is ``act_counter`` before the call; only a
  mode-1 call advances it, by one.
* ``fill_random(seed)``: key the fill seed; row ``row``, column ``k``:
  counter ``(row, k, 7, row >> 32)``: ``state = normal(.x, .y)``, ``next_state = normal(.z, .w)``;
  counter ``(row, k, 8, row >> 32)``: ``action = 2 * u01(.x) - 1`` in float32;
  counter ``(row, 0, 9, row >> 32)``: ``reward = normal(.x, .y)``, ``notdone = u01(.z) < 0.99f``;
  ``priority = 1``.

``step`` is ``rle_get_counters()[4]`` as read before the step that consumes the batch (the prefetch draws
it one step early, with ``ahead = 1``).

Same-key streams are kept apart by a constant counter word: ``.y`` is 0 for ``u`` and 1 for the noise (a
sampler counter and a noise counter of any two steps differ there); ``.z`` is 7 / 8 / 9 for the three fill
draws.  The act stream has a key of its own.
"""

from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key schedule (Weyl) increments
MASK = 0xFFFFFFFF
ACT_KEY_MUL, ACT_KEY_ADD = 0x9E3779B97F4A7C15, 0x5851F42D4C957F2D

# constant counter words (see the module docstring)
Y_U, Y_EPS, Y_ACT = 0, 1, 7
Z_FILL_STATE, Z_FILL_ACTION, Z_FILL_REWARD = 7, 8, 9


def philox4x32_10(key2, ctr4, rounds=10):
    """key2: two 32-bit words; ctr4: four words, each a scalar or an array (broadcast together).
    Returns the four output words as uint64 arrays holding 32-bit values."""
    k0, k1 = (int(k) & MASK for k in key2)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & np.uint64(MASK) for c in ctr4])
    m32 = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0  # (32 x 32 bits: fits 64)
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def key_of(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & MASK, seed >> 32


def act_key(seed):
    return key_of((int(seed) * ACT_KEY_MUL + ACT_KEY_ADD) & 0xFFFFFFFFFFFFFFFF)


def u01(x):
    """float32, exact: a 24-bit integer times 2^-24."""
    return ((np.asarray(x, np.uint64) >> np.uint64(8)).astype(np.float64) / 16777216.0).astype(np.float32)


def box_muller_uniforms(a, b):
    """(u1 in (0, 1], u2 in [0, 1)) of normal(a, b), float64 (exact)."""
    u1 = ((np.asarray(a, np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (np.asarray(b, np.uint64) >> np.uint64(8)).astype(np.float64) / 16777216.0
    return u1, u2


def normal(a, b):
    """float64."""
    u1, u2 = box_muller_uniforms(a, b)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def _split(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v & MASK, v >> 32


def u_counter(b, step):
    """Counter words of the sampler's draw of query b at step ``step``."""
    lo, hi = _split(step)
    return np.asarray(b, np.uint64), Y_U, lo, hi


def eps_counter(e, step):
    """Counter words of noise element e = b * A + j at step ``step``."""
    lo, hi = _split(step)
    return np.asarray(e, np.uint64), Y_EPS, lo, hi


def act_counter(e, ctr):
    """Counter words of exploration element e = row * A + j of the act call at ``act_counter == ctr``."""
    lo, hi = _split(ctr)
    return np.asarray(e, np.uint64), Y_ACT, lo, hi


def fill_counter(row, k, z):
    """Counter words of fill_random's draw ``z`` (Z_FILL_*) at row ``row``, column ``k``."""
    row = np.asarray(row, np.uint64)
    return row & np.uint64(MASK), np.asarray(k, np.uint64), z, row >> np.uint64(32)


def step_u(seed, step, B):
    """The sampler's u of step ``step``: float32 [B]."""
    return u01(philox4x32_10(key_of(seed), u_counter(np.arange(B), step))[0])


def step_eps(seed, step, B, A):
    """(eps, eps2) of step ``step``: float64 [B, A] each."""
    x, y, z, w = philox4x32_10(key_of(seed), eps_counter(np.arange(B * A).reshape(B, A), step))
    return normal(x, y), normal(z, w)


def act_eps(seed, ctr, n, A):
    """Exploration draws of the mode-1 act call made at ``act_counter == ctr``: float64 [n, A]."""
    x, y, _, _ = philox4x32_10(act_key(seed), act_counter(np.arange(n * A).reshape(n, A), ctr))
    return normal(x, y)


def fill_rows(seed, rows, S, A):
    """Rows ``rows`` (a count: 0 .. rows-1, or an array of row numbers) of ``fill_random(seed)``:
    {"state", "next_state" float64 [n, S]; "action" float32 [n, A]; "reward" float64 [n]; "notdone",
    "priority" float32 [n]}."""
    r = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, np.uint64)
    key = key_of(seed)
    x, y, z, w = philox4x32_10(key, fill_counter(r[:, None], np.arange(S)[None], Z_FILL_STATE))
    out = {"state": normal(x, y), "next_state": normal(z, w)}
    x, _, _, _ = philox4x32_10(key, fill_counter(r[:, None], np.arange(A)[None], Z_FILL_ACTION))
    out["action"] = np.float32(2.0) * u01(x) - np.float32(1.0)  # (exact in float32: (k - 2^23) / 2^23, k < 2^24)
    x, y, z, _ = philox4x32_10(key, fill_counter(r, 0, Z_FILL_REWARD))
    out["reward"] = normal(x, y)
    out["notdone"] = (u01(z) < np.float32(0.99)).astype(np.float32)
    out["priority"] = np.ones(r.size, np.float32)
    return out


def tapes(alg, seed, step0, n, B, A):
    """Steps step0 .. step0 + n - 1 as tapes in the layout rle_set_tapes / oracle.agents.run_steps take:
    {"u" [n, B], "eps" [n, B, A], and for SAC "eps_pi" [n, B, A]}, float32."""
    u = np.stack([step_u(seed, step0 + t, B) for t in range(n)])
    pairs = [step_eps(seed, step0 + t, B, A) for t in range(n)]
    out = {"u": u, "eps": np.stack([p[0] for p in pairs]).astype(np.float32)}
    if alg == "sac":
        out["eps_pi"] = np.stack([p[1] for p in pairs]).astype(np.float32)
    return out
