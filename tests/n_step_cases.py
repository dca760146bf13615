"""Episodic replay rings for the n-step tests (TEST INFRASTRUCTURE): ``state[i + 1] = next_state[i]`` bit for bit
inside an episode, mixed episode lengths, terminated and truncated ends, in the three ring situations the device
gather has to tell apart.

Every ring has 64 slots and holds the same twelve episodes (EPISODES: length and how it ends) laid end to end:

* ``term``   the last row has notdone 0 and the next row starts from a fresh state;
* ``trunc``  the last row has notdone 1 (a time limit) and the next row starts from a fresh state: only the data
             says that the episode is over;
* ``sticky`` the last row has notdone 0 and the next episode starts from exactly its next_state (a reset into the
             terminal state): only notdone says that the episode is over.

The situations (``ring(kind, S, A)``):

* ``part``   size 45 < cap, ptr = size, in the middle of an episode; the slots from 45 on hold stale rows that go on
             with that episode, so only ``nxt >= size`` stops a walk at slot 44;
* ``mid``    a full ring whose ptr 33 lies in the middle of an episode whose rows are all there, so only
             ``nxt == ptr`` stops a walk at slot 32;
* ``wrap``   a full ring turned by four slots, so that the last episode runs across slots 63 -> 0, with ptr at an
             episode's first row elsewhere.

Lengths 9, 12, 8 and 11 give every hop count 1 .. 8 for every n <= 8; tests/test_n_step.py checks that and that
every stop cause occurs.
"""

from __future__ import annotations

import numpy as np

CAP = 64
# (length, end) -- 64 rows in all
EPISODES = ((1, "term"), (2, "trunc"), (3, "sticky"), (5, "trunc"), (7, "term"), (9, "trunc"), (1, "trunc"),
            (12, "term"), (8, "trunc"), (2, "term"), (3, "trunc"), (11, "term"))
assert sum(n for n, _ in EPISODES) == CAP
KINDS = ("part", "mid", "wrap")
N_TESTED = (1, 2, 3, 5, 8)
GAMMA = 0.97  # (not a power of two: every product rounds)


def _episodes(S, A, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    state = np.empty((CAP, S), np.float32)
    nxt = rng.standard_normal((CAP, S), dtype=np.float32)
    action = rng.uniform(-1.0, 1.0, (CAP, A)).astype(np.float32)
    reward = rng.standard_normal(CAP, dtype=np.float32)
    notdone = np.ones(CAP, np.float32)
    row, carry = 0, None
    for length, end in EPISODES:
        for k in range(length):
            if k:
                state[row] = nxt[row - 1]
            elif carry is not None:
                state[row] = carry
            else:
                state[row] = rng.standard_normal(S, dtype=np.float32)
            carry = None
            row += 1
        if end in ("term", "sticky"):
            notdone[row - 1] = 0.0
        if end == "sticky":
            carry = nxt[row - 1].copy()
    return dict(state=state, next_state=nxt, action=action, reward=reward, notdone=notdone)


def ring(kind, S, A, seed=7):
    """dict(state, next_state, action, reward, notdone: float32 over all 64 slots; ptr, size)."""
    r = _episodes(S, A, seed + KINDS.index(kind))
    if kind == "part":
        r.update(ptr=45, size=45)
    elif kind == "mid":
        r.update(ptr=33, size=CAP)
    else:
        for k in ("state", "next_state", "action", "reward", "notdone"):
            r[k] = np.roll(r[k], 4, axis=0)
        r.update(ptr=4 + 27, size=CAP)  # (the first row of the one-row episode after the nine-row one)
    return r


def load(rep, r):
    """The ring into an rl._engine.Replay of 64 slots: every slot's row, then ptr and size."""
    rep.import_rows(0, r["state"], r["action"], r["reward"], r["next_state"], r["notdone"])
    rep.set_state(r["ptr"], r["size"], 1.0)
