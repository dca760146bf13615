"""Critic dropout (TEST INFRASTRUCTURE): ``Linear -> Dropout(p) -> LayerNorm -> activation`` in every hidden layer
of the TD3 / SAC critics -- the DroQ critic -- as a stateful composite activation of the CPU oracle, with the masks
rebuilt on the host from the device's Philox stream.

The host mask law (``mask``), on tests/philox_ref.py's public functions: key ``cfg.seed``; counter
``(b * 128 + j4, 2 + site, step_lo, step_hi)``; the four output words are columns ``4 j4 .. 4 j4 + 3`` of batch row
``b``; ``keep = u01(word) >= float32(p)``; the mask is ``keep * s`` with ``s = float32(1) / (float32(1) - float32(p))``.
``site = (pass * 2 + twin) * 8 + layer``; pass 0 target, 1 online, 2 policy (AWAC: Q(s, a_pi)), 3 AWAC's Q(s, a).

``DropLN`` is the composite: registered as ``"dropln_<act>"`` in ``oracle.nets.ACTS`` (as tests/layer_norm.py
registers ``"ln_<act>"``), it multiplies its input by the mask of the call's ``(pass, twin, layer)`` in the input's
dtype and applies ``act(F.layer_norm(.))``.  It finds the site by counting its calls within a step: the oracles
call target ``tq1``, ``tq2``, then online ``q1``, ``q2``, then (policy steps) policy ``q1``, ``q2``; AWAC
(tests/offline_sac_oracle.py) calls Q(s, a) of ``q1``, ``q2`` (pass 3) and then Q(s, a_pi) (pass 2) after the online
pass.  While a case is registered the oracles' ``step`` methods are wrapped: the wrapper sets the step word (the
oracle's ``n_runs``, the engine's RNG step counter) and resets the count, and asserts at the step's end that the
count was 4 L or 6 L (AWAC: 8 L).  oracle/ itself does not change and edge_cases.float64_oracle() works on it as it
stands.
"""

from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import edge_cases as EC
import layer_norm as LN
import philox_ref as PR
from oracle import agents
from oracle import nets as N

PREFIX = "dropln_"
Y_DROP = 2  # counter word .y of site 0 (the step streams use 0 and 1)
PASS_TARGET, PASS_ONLINE, PASS_POLICY, PASS_AWAC_DATA = 0, 1, 2, 3
MAX_SITE = (PASS_AWAC_DATA * 2 + 1) * 8 + 7


def site_of(pas, twin, layer):
    return (pas * 2 + twin) * 8 + layer


def scale(p):
    """s = 1 / (1 - p), one float32 division."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_counter(b, j4, site, step):
    """Counter words of the Philox block of columns 4 j4 .. 4 j4 + 3 of batch row b."""
    step = int(step) & 0xFFFFFFFFFFFFFFFF
    lo, hi = step & PR.MASK, step >> 32
    return (np.asarray(b, np.uint64) * np.uint64(128) + np.asarray(j4, np.uint64)) & np.uint64(PR.MASK), Y_DROP + site, lo, hi


def keep_words(seed, step, site, rows, width):
    """The stream's words as [rows, width] (uint64 holding 32-bit values)."""
    assert width % 4 == 0 and 4 <= width <= 512
    b = np.arange(rows, dtype=np.uint64)[:, None]
    j4 = np.arange(width // 4, dtype=np.uint64)[None]
    w = PR.philox4x32_10(PR.key_of(seed), drop_counter(b, j4, site, step))
    return np.stack(w, -1).reshape(rows, width)


def mask(seed, p, step, site, rows, width):
    """float32 [rows, width]: 0 where the unit is dropped, s where it is kept."""
    keep = PR.u01(keep_words(seed, step, site, rows, width)) >= np.float32(p)
    return np.where(keep, scale(p), np.float32(0.0)).astype(np.float32)


class DropLN:
    """The stateful composite (see the module docstring).  order: the pass of each run of 2 L calls."""

    def __init__(self, act, seed, p, L, awac=False, step0=0):
        self.act, self.seed, self.p, self.L, self.step0 = act, int(seed), float(p), int(L), int(step0)
        self.order = (PASS_TARGET, PASS_ONLINE, PASS_AWAC_DATA, PASS_POLICY) if awac else (PASS_TARGET, PASS_ONLINE, PASS_POLICY)
        self.legal = (8 * L,) if awac else (4 * L, 6 * L)
        self.step, self.calls = None, 0
        self.seen = {}  # (step, site) -> mask, of the last run (the seed conditions read it)

    def begin(self, step):
        self.step, self.calls = self.step0 + int(step), 0

    def end(self):
        assert self.calls in self.legal, (self.calls, self.legal)
        self.step = None

    def __call__(self, x):
        assert self.step is not None, "DropLN called outside a wrapped oracle step"
        k = self.calls
        self.calls += 1
        pas, twin, layer = self.order[k // (2 * self.L)], (k // self.L) % 2, k % self.L
        site = site_of(pas, twin, layer)
        m = mask(self.seed, self.p, self.step, site, x.shape[0], x.shape[1])
        self.seen[(self.step, site)] = m
        return self.act(F.layer_norm(x * torch.from_numpy(m).to(x.dtype), x.shape[-1:]))


def _wrap(cls):
    plain = cls.__dict__["step"]

    def step(self, *a, **k):
        comp = self.ac if isinstance(self.ac, DropLN) else None
        if comp is None:
            return plain(self, *a, **k)
        comp.begin(self.n_runs)
        out = plain(self, *a, **k)
        comp.end()
        return out

    step._plain = plain
    return step


def _oracle_classes():
    import offline_sac_oracle
    import offline_td3_oracle

    return [agents.TD3Oracle, agents.SACOracle, offline_td3_oracle.TD3BCOracle, offline_sac_oracle.AWACOracle]


@contextlib.contextmanager
def composite(act, seed, p, L, awac=False, step0=0):
    """``"dropln_<act>"`` in oracle.nets.ACTS and the oracles' steps wrapped, while the block runs: the DropLN."""
    name = PREFIX + act
    assert name not in N.ACTS
    comp = DropLN(N.ACTS[act], seed, p, L, awac, step0)
    N.ACTS[name] = comp
    classes = _oracle_classes()
    for cls in classes:
        cls.step = _wrap(cls)
    try:
        yield comp
    finally:
        for cls in classes:
            cls.step = cls.__dict__["step"]._plain
        del N.ACTS[name]


# name -> (source case of edge_cases.CASES, plain critic activation, p, seed): tests/layer_norm.py LN_CASES' seven
# sources again.  p = 0.5 on the two minimum shapes (4 columns, one row) and 0.25 elsewhere: DroQ's 0.01 would drop
# nothing at these sizes.  The seed is the engine's cfg.seed: the first of 601 + position + 100 k, chosen on the host
# before any GPU run, at which the case meets the sweep's host criteria (float32 against float64), every site has a
# dropped and a kept element over the run, and -- td3-min -- some site has an all-dropped row at some step
# (tests/test_critic_dropout.py asserts all of it).  Three cases missed the host criteria at their first seed and took
# the next: drop-td3-min (601: the policy's step-1 moments 1.9e-4 from float64), drop-sac-h260 (604: one policy
# weight 4.3e-5 from float64 after 4 steps) and drop-sac-min (606: q2's step-1 moments 6.4e-4 from float64).
DROP_CASES = {
    "drop-td3-min": ("td3-min", "relu", 0.5, 701),
    "drop-td3-k49": ("td3-k49", "relu", 0.25, 602),
    "drop-td3-deep6": ("td3-deep6", "elu", 0.25, 603),
    "drop-sac-h260": ("sac-h260", "relu", 0.25, 704),
    "drop-sac-a25": ("sac-a25", "gelu", 0.25, 605),
    "drop-sac-min": ("sac-min", "relu", 0.5, 706),
    "drop-td3-w100": ("td3-w100", "identity", 0.25, 607),
}


def depth(case):
    c = EC.CASES[DROP_CASES[case][0]]
    return len(c.hidden_sizes) if c.hidden_sizes else 2


def strip(g):
    """The golden the engine is built from: the critic's composite replaced by its plain activation."""
    g = dict(g)
    acts = [str(v) for v in g["meta_acts"]]
    assert acts[1].startswith(PREFIX), acts
    acts[1] = acts[1][len(PREFIX):]
    g["meta_acts"] = np.array(acts)
    return g


def drop_engine(g, p, plan=None, build=None):
    """engine_from_golden (or ``build``) on strip(g) with the critics' LayerNorm and dropout p: (engine, replay)."""
    from harness import engine_from_golden

    out = (build or engine_from_golden)(strip(g), plan=plan)
    eng, rep = out[0], out[1]
    eng.set_layer_norm(True)
    if p is not None:
        eng.set_critic_dropout(p)
        assert eng.critic_dropout() == float(np.float32(p))
    return eng, rep


@contextlib.contextmanager
def registered(name, engine=False, engine_p="case", seed=None):
    """edge_cases.CASES[name], a golden(name) carrying the composite and the composite itself, while the block runs;
    engine=True: the GPU sweep's ``_engine`` builds LayerNorm + dropout engines for the case (engine_p: another p
    for the engine than the oracle's; None: the setter is not called).  seed: another seed than the table's."""
    src, act, p, seed0 = DROP_CASES[name]
    seed = seed0 if seed is None else seed
    assert name not in EC.CASES
    plain = EC.golden

    def golden(case):
        g = plain(case)
        if case == name:
            g["meta_acts"] = LN.meta_acts(PREFIX + act)
        return g

    EC.CASES[name] = EC.CASES[src]._replace(seed=seed)
    EC.golden = golden
    sweep = plain_engine = None
    if engine:
        import test_shape_edges_gpu as sweep

        plain_engine = sweep._engine

        def _engine(case, plan=None, g=None):
            if case != name:
                return plain_engine(case, plan, g)
            g = EC.reference(case)["g"] if g is None else g
            with EC.edge_env(case):
                return drop_engine(g, p if engine_p == "case" else engine_p, plan)

        sweep._engine = _engine
    try:
        with composite(act, seed, p, depth(name)) as comp:
            yield comp
    finally:
        if engine:
            sweep._engine = plain_engine
        EC.golden = plain
        del EC.CASES[name]


_SEEN = {}


def reference(name, seed=None):
    """edge_cases.reference of a DROP_CASES entry (float32 and float64 oracle runs, computed once, shared), with the
    masks the float64 run drew under "masks": {(step, site): float32 [rows, width]}."""
    key = (name, seed)
    with registered(name, seed=seed) as comp:
        if seed is not None:
            EC._REF.pop(name, None)
        ref = EC.reference(name)
        if key not in _SEEN:
            _SEEN[key] = dict(comp.seen)
        if seed is not None:
            EC._REF.pop(name, None)
    out = dict(ref)
    out["masks"] = _SEEN[key]
    return out


def seed_conditions(name, ref):
    """The seed rules of DROP_CASES beyond the host criteria: (every site drops and keeps, some row all dropped)."""
    by_site = {}
    for (step, site), m in ref["masks"].items():
        d, k = by_site.get(site, (False, False))
        by_site[site] = (d or bool((m == 0).any()), k or bool((m != 0).any()))
    both = bool(by_site) and all(d and k for d, k in by_site.values())
    all_dropped = any(bool((m == 0).all(-1).any()) for m in ref["masks"].values())
    return both, all_dropped, sorted(by_site)


def host_shortfalls(ref):
    """tests/test_shape_edges.py's host criteria (as tests/test_layer_norm.py restates them) on a reference: the
    same draws; step 1's Adam first moments within 1e-5 of each tensor's max |m|; losses rel 1e-3; end parameters
    within 2 lr n + 1e-4, every element within 1e-5.  Returns what falls short (empty: the case is a valid
    reference) and the worst step-1 moment distance."""
    f32, f64 = ref["f32"], ref["f64"]
    bad = []
    n = len(f32["ind"])
    for t in range(n):
        if not np.array_equal(f32["ind"][t], f64["ind"][t]):
            bad.append(("ind", t))
    if set(f32["m"]) != set(f64["m"]) or not f32["m"]:
        bad.append(("moment keys",))
    worst = max(EC.moment_distance(f32["m"][k], f64["m"][k]) for k in f64["m"])
    bad += [("moment", k) for k in f64["m"] if not EC.moment_distance(f32["m"][k], f64["m"][k]) <= 1e-5]
    nan32, nan64 = np.isnan(f32["table"]), np.isnan(f64["table"])
    if not np.array_equal(nan32, nan64):
        bad.append(("info nan",))
    elif not np.allclose(f32["table"], f64["table"], rtol=1e-3, atol=0, equal_nan=True):
        bad.append(("info",))
    if not np.isfinite(f64["table"][~nan64]).all():
        bad.append(("info finite",))
    tol = 2 * 3e-4 * n + 1e-4
    for key, v64 in f64["params"].items():
        d = np.abs(f32["params"][key].astype(np.float64) - v64)
        if not d.max() <= tol or not (d <= 1e-5).all():
            bad.append(("param", key, float(d.max())))
    return bad, worst
