"""The shape-edge table (tests/edge_cases.py) on the GPU: every case trains like the CPU oracle, takes the
path it was written for, and the forward entry points agree with oracle.nets at the row-count edges.

Tolerances are the project's own (tests/test_engine_gpu.py): indices exact; info columns rel 1e-3 (atol
1e-4); priorities rtol 1e-4 / atol 1e-5; TD7 value bounds 1e-4; parameters after n steps every element
within 2 lr n + 1e-4 and 99% of each tensor within 1e-5; forward outputs 1e-5 + 1e-5 |ref|; sampled actions
2e-6 + 1e-5 |ref|.  Step 1's gradients are read through the Adam first moments and compared with the
float64 oracle: within max(1e-5, 4 d32) of the tensor's max |m|, d32 being the float32 oracle's own
distance from float64 for that tensor (the 1e-5 is test_wide_hidden_steps_match_oracle's; the 4 x term
only matters where the oracle itself is several 1e-6 away, as at the 1152-column input layers).
"""

import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
from edge_cases import CASES, capacity, edge_env, info_keys, moment_distance, reference  # noqa: E402
from harness import LOSS_RTOL, engine_from_golden  # noqa: E402
from oracle import nets as N  # noqa: E402
from oracle import spec  # noqa: E402
from test_engine_gpu import assert_params_close  # noqa: E402
from test_offline_gpu import offline_engine  # noqa: E402


def _engine(case, plan=None, g=None):
    """(g: a golden other than the table's, e.g. another target_update_rate -- no oracle run then)"""
    c = CASES[case]
    g = reference(case)["g"] if g is None else g
    with edge_env(case):
        if c.bc_lambda:
            return offline_engine(g, c.bc_lambda, plan)
        eng, rep, _ = engine_from_golden(g, plan=plan)
    return eng, rep


def _tapes(case):
    g = reference(case)["g"]
    return {k[5:]: v for k, v in g.items() if k.startswith("tape_")}


def _check_lap_and_bounds(case, eng, rep, run, t):
    c = CASES[case]
    ncap = capacity(case)
    np.testing.assert_array_equal(eng.last_indices(), run["ind"][t])
    if c.use_lap:
        got = rep.get_priority(ncap)
        np.testing.assert_allclose(got, run["prio"][t], rtol=1e-4, atol=1e-5)
        drawn = np.zeros(ncap, bool)
        for i in run["ind"][:t + 1]:
            drawn[i] = True
        p0 = spec.init_priorities(ncap, c.seed + 2)
        np.testing.assert_array_equal(got[~drawn], p0[~drawn])  # rows never drawn: untouched
    if c.alg == "td7":  # a padded row leaking into the min / max shows here
        np.testing.assert_allclose(eng.value_bounds(), run["vb"][t].astype(np.float32), rtol=1e-4, atol=1e-4)


def check_trains_like_the_oracle(case, plan=None):
    """The criteria of test_edge_case_trains_like_the_oracle for ``case`` under ``plan`` (None: the default plan;
    tests/test_plan_edges_gpu.py calls it per (case, plan) pair).  Returns the worst distances it printed."""
    c = CASES[case]
    ref = reference(case)
    f32, f64 = ref["f32"], ref["f64"]
    n = c.n_steps
    eng, rep = _engine(case, plan)
    tp = _tapes(case)
    eng.set_tapes(u=tp["u"], eps=tp["eps"], eps_pi=tp.get("eps_pi"))
    infos = [eng.step(1)[0]]
    _check_lap_and_bounds(case, eng, rep, f32, 0)
    # step 1's gradients: every Adam first moment against the float64 oracle
    worst, failed = 0.0, []
    for key, m64 in f64["m"].items():
        net, pname = key.split(".", 1)
        got = eng.get_adam(net, pname, 0, m64.shape)
        d32 = moment_distance(f32["m"][key], m64)
        d = moment_distance(got, m64)
        worst = max(worst, d)
        if not d <= max(1e-5, 4 * d32):
            failed.append((key, d, d32))
    print(f"EDGE {case} step-1 gradient distance (of max |m64|): worst {worst:.2e}")
    assert not failed, failed
    infos += list(eng.step(n - 1))
    eng.set_tapes()
    _check_lap_and_bounds(case, eng, rep, f32, n - 1)
    k = len(info_keys(case))
    infos = np.asarray(infos, np.float64)[:, :k]
    for t in range(n):
        print("EDGE", case, "info", t, infos[t].tolist(), f32["table"][t].tolist())
    np.testing.assert_array_equal(np.isnan(infos), np.isnan(f32["table"]))
    np.testing.assert_allclose(infos, f32["table"], rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    tol = 2 * 3e-4 * n + 1e-4
    bulk, far = 1.0, 0.0
    for (net, name), v in f32["params"].items():
        d = np.abs(eng.get_param(net, name, v.shape).astype(np.float64) - v)
        bulk, far = min(bulk, float((d <= 1e-5).mean())), max(far, float(d.max()))
    print(f"EDGE {case} parameters after {n} steps: worst bulk {bulk:.4f}, worst |d| {far:.2e}")
    for (net, name), v in f32["params"].items():
        assert_params_close(eng.get_param(net, name, v.shape), v, tol, (net, name), bulk=0.99)
    if c.alg == "sac":
        np.testing.assert_allclose(eng.get_param("tmp", "log_alpha"), f32["log_alpha"].reshape(-1), rtol=1e-5, atol=1e-7)
    return {"gradient": worst, "bulk": bulk, "far": far}


@pytest.mark.parametrize("case", list(CASES))
def test_edge_case_trains_like_the_oracle(case):
    """Step 1 alone (single-step program), then the remaining steps as one burst.  TD3 / SAC: the burst replays
    the multi-step and remainder programs at this shape.  TD7: every case hard-updates every 3 steps, so each
    window of its 6-step program holds a hard update and the burst replays single-step programs around the
    hard updates only; TD7's multi-step programs run at edge shapes in tests/test_plan_edges_gpu.py
    (test_multistep_program_equals_single_steps, target_update_rate 250)."""
    check_trains_like_the_oracle(case)


@pytest.mark.parametrize("case", list(CASES))
def test_edge_programs_pass_audit_and_hazard_checks(case, monkeypatch):
    """RLE_AUDIT + RLE_HAZARD while every step program of the case is built (no step runs): each GEMM's
    address replay stays inside live allocations, and no level holds two ops touching one byte."""
    monkeypatch.setenv("RLE_AUDIT", "1")
    monkeypatch.setenv("RLE_HAZARD", "1")
    eng, rep = _engine(case)
    assert eng.describe(0) and eng.describe(1)


# What the program descriptions (rle_graph_describe 0: a policy step) name of each edge's fusion, as regular
# expressions: (case, pattern, present).  "+pl]" / "+pl2]": the pre-layer recomputed in its consumer's tile /
# the two-stage one behind the in-tile actor output; "sacfwd]": SAC's raw head + rsample as a GEMM epilogue,
# a bare "sacfwd": the standalone op; "st+sacpre": the target critics' in-tile rsample; "head+dx": the critic
# loss head inside a DX, a bare "head": the standalone head; a bare "bc": the offline term's op.  (The
# description does not name actor_pre or the folded zsa3; td7-a32 / a33 and td3-a33 are held by the sweep alone.)
_BARE = r"(?m)[: ]%s( |$)"
PATHS = [
    ("td3-k48", r"\+pl\]", True), ("td3-k48", r"qdot\+pl2\]", True), ("td3-k49", r"\+pl", False),
    ("td3-a17", r"qdot\+pl\]", True), ("td3-a17", r"qdot\+pl2\]", False),
    ("sac-a24", r"sacfwd\]", True), ("sac-a24", r"st\+sacpre", True), ("sac-a24", _BARE % "sacfwd", False),
    ("sac-a25", r"sacfwd\]", False), ("sac-a25", r"st\+sacpre", False), ("sac-a25", _BARE % "sacfwd", True),
    ("sac-h260", r"sacfwd\]", False), ("sac-h260", _BARE % "sacfwd", True), ("sac-h260", r"head\+dx", False),
    ("sac-h260", _BARE % "head", True), ("sac-a24", r"head\+dx", True),
    ("td7-b1", r"head\+dx", True), ("td7-b1", _BARE % "head", False),
    ("td7-odd", r"head\+dx", False), ("td7-odd", _BARE % "head", True),
    ("td7-h272", r"head\+dx", False), ("td7-h272", _BARE % "head", True),
    ("td7-h512", r"head\+dx", False), ("td7-h512", _BARE % "head", True),
    ("td7-odd_bc", _BARE % "bc", True), ("td7-odd", _BARE % "bc", False),
]


@pytest.mark.parametrize("case,pattern,present", PATHS,
                         ids=[f"{c}-{'has' if p else 'no'}-{i}" for i, (c, t, p) in enumerate(PATHS)])
def test_edge_takes_the_intended_path(case, pattern, present):
    """A later change of a predicate must not move an edge case off the path it was written for."""
    eng, rep = _engine(case)
    desc = eng.describe(0)
    assert bool(re.search(pattern, desc)) == present, (pattern, desc)


# ---- forward entry points at the row-count edges -------------------------------------------------------------

FWD_CASES = ["td7-odd", "td3-k49", "sac-a25"]
ROWS = [1, 15, 17, 1023, 1024]
_FWD = {}


def _fwd_reference(case):
    """oracle.nets (float32, as the reference runs them) on the case's start weights and 1,024 seeded
    rows, once; every row count reads a prefix."""
    if case in _FWD:
        return _FWD[case]
    c = CASES[case]
    rng = np.random.default_rng(c.seed)
    s = rng.standard_normal((1024, c.S)).astype(np.float32)
    a = rng.uniform(-1, 1, (1024, c.A)).astype(np.float32)
    eps = rng.standard_normal((1024, c.A)).astype(np.float32) * 3  # (3 sigma x 0.1: some TD7 / TD3 actions clip)
    shape = {k: v for k, v in (("hidden_sizes", c.hidden_sizes), ("zs_dim", c.zs_dim)) if v is not None}
    P = {net: {k: torch.from_numpy(v) for k, v in d.items()}
         for net, d in spec.agent_params(c.alg, c.S, c.A, c.H, c.seed, **shape).items()}
    x, at, e = torch.from_numpy(s), torch.from_numpy(a), torch.from_numpy(eps)
    out = {"s": s, "a": a, "eps": eps}
    torch.set_num_threads(1)
    with torch.no_grad():
        if c.alg == "td7":
            pi = N.sale_actor(P["policy"], x, N.sale_zs(P["fixed_encoder"], x))
            out["act"] = pi
            out["det"], out["noisy"] = pi, (pi + e * 0.1).clamp(-1.0, 1.0)
            for q, enc in (("q1", "fixed_encoder"), ("q2", "fixed_encoder"), ("target_q1", "fixed_encoder_target"),
                           ("target_q2", "fixed_encoder_target")):
                zs = N.sale_zs(P[enc], x)
                out["q:" + q] = (enc, N.sale_critic(P[q], x, at, N.sale_zsa(P[enc], zs, at), zs)[:, 0])
            for enc in ("encoder", "fixed_encoder", "fixed_encoder_target"):
                zs = N.sale_zs(P[enc], x)
                out["zs:" + enc], out["zsa:" + enc] = zs, N.sale_zsa(P[enc], zs, at)
        else:
            raw = N.mlp(P["policy"], x)
            out["act"] = raw
            if c.alg == "td3":
                pi = torch.tanh(raw)
                out["det"], out["noisy"] = pi, (pi + e * 0.1).clamp(-1.0, 1.0)
            else:
                mean, log_std = raw.chunk(2, -1)
                out["det"] = torch.tanh(mean)
                out["noisy"] = torch.tanh(mean + e * torch.clamp(log_std, -20.0, 2.0).exp())
            for q in ("q1", "q2", "target_q1", "target_q2"):
                out["q:" + q] = (None, N.mlp_critic(P[q], x, at)[:, 0])
    _FWD[case] = {k: (v.numpy() if isinstance(v, torch.Tensor) else
                      (v[0], v[1].numpy()) if isinstance(v, tuple) else v) for k, v in out.items()}
    return _FWD[case]


def _close(got, ref, atol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = np.abs(got - ref)
    lim = atol + 1e-5 * np.abs(ref)
    assert (d <= lim).all(), (what, float(d.max()), float((d / lim).max()), int((d > lim).sum()))


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_entry_points_at_row_count_edges(case, n):
    """rle_act, rle_act_sample (deterministic, and with a noise tape) and rle_eval (every critic, TD7: with the
    online and the target embeddings; every encoder's zs and zsa) on n rows: one row, one short of and one past
    a 16-row block, one short of the limit, the limit."""
    c = CASES[case]
    ref = _fwd_reference(case)
    eng, rep = _engine(case)
    s, a, eps = ref["s"][:n], ref["a"][:n], ref["eps"][:n]
    _close(eng.act(s, ref["act"].shape[1]), ref["act"][:n], 1e-5, "act")
    eng.set_action_map(1.0, 0.0, 0.1)
    _close(eng.act_sample(s, 0).copy(), ref["det"][:n], 2e-6, "act_sample mode 0")
    _close(eng.act_sample(s, 2, eps).copy(), ref["noisy"][:n], 2e-6, "act_sample mode 2")
    for key, v in ref.items():
        kind, _, net = key.partition(":")
        if kind == "q":
            _close(eng.eval_q(net, s, a, v[0]), v[1][:n], 1e-5, key)
        elif kind == "zs":
            _close(eng.eval_zs(net, s), v[:n], 1e-5, key)
        elif kind == "zsa":
            _close(eng.eval_zsa(net, s, a), v[:n], 1e-5, key)


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_entry_points_reject_1025_rows(case):
    c = CASES[case]
    eng, rep = _engine(case)
    s = np.zeros((1025, c.S), np.float32)
    a = np.zeros((1025, c.A), np.float32)
    out = np.zeros((1025, 2 * c.A), np.float32)
    with pytest.raises(RuntimeError, match="rle error -1.*1024"):
        eng.act(s, c.A)
    with pytest.raises(RuntimeError, match="rle error -1.*1024"):
        eng.eval_q("q1", s, a)
    assert E.lib().rle_act_sample(eng.h, s.ctypes.data, 1025, 0, None, out.ctypes.data) == -1
    assert b"1024" in E.lib().rle_last_error()
    if c.alg == "td7":
        with pytest.raises(RuntimeError, match="rle error -1.*1024"):
            eng.eval_zs("encoder", s)
    if c.alg == "sac":
        with pytest.raises(RuntimeError, match="rle error -1"):
            eng.sac_rsample(a, a, a)


def _rsample_inputs(n, A, seed):
    """mean, log_std, eps of n rows in four kinds, cycling: plain rows; log_std below the lower clamp (-20);
    log_std above the upper clamp (2); |u| > 10 (a saturated tanh).  Outside the last kind u stays within
    +-2, where log(1 - a^2 + 1e-6) is well conditioned in float32; eps is solved from the u wanted."""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 4
    mean = rng.standard_normal((n, A))
    log_std = rng.uniform(-3.0, 1.0, (n, A))
    log_std[kind == 1] = rng.uniform(-30.0, -20.5, (int((kind == 1).sum()), A))
    log_std[kind == 2] = rng.uniform(2.5, 6.0, (int((kind == 2).sum()), A))
    u = rng.uniform(-2.0, 2.0, (n, A))
    u[kind == 3] = rng.choice([-1.0, 1.0], (int((kind == 3).sum()), A)) * rng.uniform(10.5, 14.0, (int((kind == 3).sum()), A))
    mean[kind == 1] = u[kind == 1]  # (scale e^-20: u is the mean)
    scale = np.exp(np.clip(log_std, -20.0, 2.0))
    eps = np.where((kind == 1)[:, None], rng.standard_normal((n, A)), (u - mean) / scale)
    return mean.astype(np.float32), log_std.astype(np.float32), eps.astype(np.float32)


@pytest.mark.parametrize("n", [1, 17, 1024])
def test_sac_rsample_at_row_count_edges(n):
    """rle_sac_rsample against SAC._rsample's formula (oracle.nets.gaussian_tanh) in float64: action atol
    1e-6, log_pi rtol 1e-5 / atol 1e-4.  Where the same formula in torch float32 is itself further from
    float64 (a saturated tanh: 1 - a^2 rounds to 0 and log(1e-6) stands for log(1e-6 + 1.7e-8), per
    action dimension; u - mean below the lower clamp), the bound of that element is 4 x the float32
    formula's own error."""
    case = "sac-a25"
    A = CASES[case].A
    eng, rep = _engine(case)
    mean, log_std, eps = _rsample_inputs(max(n, 4), A, 1000 + n)
    if n == 1:  # (the one row: a saturated one)
        mean, log_std, eps = mean[3:4], log_std[3:4], eps[3:4]
    t = [torch.from_numpy(x) for x in (mean, log_std, eps)]
    a32, lp32 = (x.numpy().astype(np.float64) for x in N.gaussian_tanh(*t))
    a64, lp64 = (x.numpy() for x in N.gaussian_tanh(*(x.double() for x in t)))
    act, lp = eng.sac_rsample(mean, log_std, eps)
    da, dl = np.abs(act - a64), np.abs(lp - lp64[:, 0])
    lim_a = np.maximum(1e-6, 4 * np.abs(a32 - a64))
    lim_l = np.maximum(1e-4 + 1e-5 * np.abs(lp64[:, 0]), 4 * np.abs(lp32 - lp64)[:, 0])
    print("EDGE rsample", n, "action worst", float(da.max()), "torch float32's own", float(np.abs(a32 - a64).max()),
          "log_pi worst / bound", float((dl / lim_l).max()), "rows on the 4x bound",
          int((4 * np.abs(lp32 - lp64)[:, 0] > 1e-4 + 1e-5 * np.abs(lp64[:, 0])).sum()))
    assert (da <= lim_a).all(), (float(da.max()), float((da / lim_a).max()))
    assert (dl <= lim_l).all(), (float(dl.max()), float((dl / lim_l).max()))
