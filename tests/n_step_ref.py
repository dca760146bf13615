"""The n-step law of include/rle.h in NumPy float32 (TEST INFRASTRUCTURE): the host reference of the device
sampler's multi-hop gather (rle_set_n_step, rle_replay_gather_nstep).

For a sampled slot ``i`` of a ring with capacity ``cap``, ``size`` rows and write pointer ``ptr``:

    cur = i; R = reward[cur]; g = 1; hops = 1
    while hops < n:
        notdone[cur] == 0                                   -> stop   ("terminated")
        nxt = cur + 1 (cap -> 0);  nxt >= size              -> stop   ("size")
                                   nxt == ptr               -> stop   ("ptr")
        bits(next_state[cur]) != bits(state[nxt])           -> stop   ("cut")
        g = g * gamma;  R = R + g * reward[nxt];  cur = nxt;  hops += 1

Every product and sum is one float32 operation (np.float32 scalars: no contraction), as on the device, whose
``nstep_mul`` / ``nstep_madd`` (kernels.hip) keep each product and sum uncontracted: the two match bit for bit.
``causes`` names why each walk ended ("n": it reached n).
"""

from __future__ import annotations

import numpy as np

CAUSES = ("n", "terminated", "size", "ptr", "cut")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def n_step_one(ring, i, n, gamma):
    """(R, final row, g * notdone[final], hops, cause) of slot i; ring: dict of state, next_state, reward,
    notdone (float32 arrays over the whole capacity), ptr, size."""
    cap = ring["state"].shape[0]
    size, ptr = int(ring["size"]), int(ring["ptr"])
    reward, notdone = ring["reward"], ring["notdone"]
    gamma = np.float32(gamma)
    cur, R, g, hops, cause = int(i), np.float32(reward[i]), np.float32(1.0), 1, "n"
    while hops < n:
        if notdone[cur] == 0:
            cause = "terminated"
            break
        nxt = cur + 1
        if nxt == cap:
            nxt = 0
        if nxt >= size:
            cause = "size"
            break
        if nxt == ptr:
            cause = "ptr"
            break
        if not np.array_equal(_bits(ring["next_state"][cur]), _bits(ring["state"][nxt])):
            cause = "cut"
            break
        g = np.float32(g * gamma)
        R = np.float32(R + np.float32(g * np.float32(reward[nxt])))
        cur = nxt
        hops += 1
    return R, cur, np.float32(g * np.float32(notdone[cur])), hops, cause


def n_step(ring, ind, n, gamma, causes=False):
    """(R [k], next_state [k, S], notdone [k], hops [k]) for the indices ``ind``; causes=True appends the list of
    stop causes."""
    ind = np.asarray(ind, np.int64).reshape(-1)
    S = ring["state"].shape[1]
    R = np.empty(ind.size, np.float32)
    s2 = np.empty((ind.size, S), np.float32)
    nd = np.empty(ind.size, np.float32)
    hops = np.empty(ind.size, np.int32)
    why = []
    for k, i in enumerate(ind):
        R[k], cur, nd[k], hops[k], c = n_step_one(ring, int(i), n, gamma)
        s2[k] = ring["next_state"][cur]
        why.append(c)
    return (R, s2, nd, hops, why) if causes else (R, s2, nd, hops)
