"""LeakyReLU, SiLU and GELU as hidden activations, on the GPU: the nine goldens the reference wrote with them
(forward entry points, Adam moments, trajectories), the shape edges at which their kernel paths can go wrong,
the two offline modes, the Python mirror, and a guard that the ELU variant ids they share still run ELU.

Every tolerance is the project's own: forward outputs 1e-5 + 1e-5 |ref| (tests/test_parity_gpu.py); sampled
actions 2e-6 + 1e-5 |ref| (tests/test_mirror_gpu.py); info columns rel harness.LOSS_RTOL, atol 1e-4; priorities
rtol 1e-4 / atol 1e-5; Adam moments 1e-4 |ref| + 1e-4 max |ref|; parameters after n steps within 2 lr n + 1e-4
and 99% of each tensor within 1e-5; SAC log_alpha rtol 1e-5.  The edge cases run tests/test_shape_edges_gpu.py's
own test body (step-1 gradients against the float64 oracle within max(1e-5, 4 d32)).
"""

import copy
import pickle

import numpy as np
import pytest
import torch

from conftest import acts_of, load_golden

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
import more_acts  # noqa: E402
import test_engine_gpu as TE  # noqa: E402
import test_offline_gpu as TOFF  # noqa: E402
import test_offline_td3_gpu as TOFF3  # noqa: E402
import test_parity_gpu as TP  # noqa: E402
import test_shape_edges_gpu as TSEG  # noqa: E402
from harness import LOSS_RTOL, engine_from_golden, parse, shape_of  # noqa: E402
from more_acts import ACT_CASES, GOLDENS  # noqa: E402
from oracle import nets as N  # noqa: E402
from oracle import spec  # noqa: E402


# ---- forward entry points on the nine goldens --------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS)
def test_eval_matches_reference(name):
    """rle_eval Q / ZS / ZSA of the online and the target nets against the reference's forward outputs
    (tests/test_parity_gpu.py's check, unchanged)."""
    TP.test_eval_matches_reference(name)


@pytest.mark.parametrize("name", GOLDENS)
def test_act_matches_reference(name):
    """rle_act on the golden's fixed batch against the reference's policy outputs (tests/test_engine_gpu.py)."""
    TE._fwd_check(name)


def _close(got, ref, atol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = np.abs(got - ref)
    lim = atol + 1e-5 * np.abs(ref)
    assert (d <= lim).all(), (what, float(d.max()), float((d / lim).max()))


@pytest.mark.parametrize("name", GOLDENS)
def test_act_sample_matches_oracle(name):
    """rle_act_sample, deterministic (mode 0) and with a noise tape (mode 2), on 1 row (the B = 1 act chain) and
    on 17 rows (the act program, one row past a 16-row block), against oracle.nets with the golden's activations."""
    g = load_golden(name)
    alg, env, H, B, *_ = parse(g)
    S, A, hi = spec.TASKS[env]
    seed = int(g["meta"][6])
    acts = {k: N.ACTS[v] for k, v in acts_of(g).items()}
    eng, rep, _ = engine_from_golden(g)
    eng.set_action_map(1.0, 0.0, 0.1)
    s, *_ = rep.gather(np.arange(17))
    eps = np.random.default_rng(seed).standard_normal((17, A)).astype(np.float32) * 3  # (some TD7 / TD3 actions clip)
    P = {net: {k: torch.from_numpy(v) for k, v in d.items()}
         for net, d in spec.agent_params(alg, S, A, H, seed, **shape_of(g)).items()}
    x, e = torch.from_numpy(s), torch.from_numpy(eps)
    torch.set_num_threads(1)
    with torch.no_grad():
        if alg == "td7":
            pi = N.sale_actor(P["policy"], x, N.sale_zs(P["fixed_encoder"], x, acts["encoder"]), acts["actor"])
        elif alg == "td3":
            pi = torch.tanh(N.mlp(P["policy"], x, acts["actor"]))
        if alg == "sac":
            mean, log_std = N.mlp(P["policy"], x, acts["actor"]).chunk(2, -1)
            det, noisy = torch.tanh(mean), torch.tanh(mean + e * torch.clamp(log_std, -20.0, 2.0).exp())
        else:
            det, noisy = pi, (pi + e * 0.1).clamp(-1.0, 1.0)
    for n in (1, 17):
        _close(eng.act_sample(s[:n], 0).copy(), det.numpy()[:n], 2e-6, (n, "mode 0"))
        _close(eng.act_sample(s[:n], 2, eps[:n]).copy(), noisy.numpy()[:n], 2e-6, (n, "mode 2"))


# ---- trajectories on the nine goldens ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDENS)
def test_adam_moments_match_reference(name):
    """Every optimizer's exp_avg / exp_avg_sq after steps 1 and 2 (tests/test_parity_gpu.py's check, unchanged):
    the new derivatives, element-wise."""
    TP.test_adam_moments_match_reference(name)


@pytest.mark.parametrize("name", GOLDENS)
def test_trajectory_matches_reference(name):
    """Step 1 alone (single-step program), then the rest as one burst (the multi-step and remainder programs):
    indices, priorities and TD7 value bounds after step 1 and at the end, the moments after step 1, every step's
    losses, the end parameters and SAC's log_alpha."""
    g = load_golden(name)
    alg, env, H, B, Ncap, n_fill, n_steps, use_lap, seed, extra = parse(g)
    eng, rep, tp = engine_from_golden(g)

    def check(t):
        np.testing.assert_array_equal(eng.last_indices(), g["ind"][t])
        if use_lap:
            np.testing.assert_allclose(rep.get_priority(Ncap), g[f"prio_{t}"], rtol=1e-4, atol=1e-5)
            assert rep.state()[2] == pytest.approx(float(g[f"maxprio_{t}"]), rel=1e-4)
        if f"vbounds_{t}" in g:
            np.testing.assert_allclose(eng.value_bounds(), g[f"vbounds_{t}"].astype(np.float32), rtol=1e-4, atol=1e-4)

    eng.set_tapes(u=tp["u"][:n_steps], eps=tp["eps"][:n_steps], eps_pi=tp.get("eps_pi"))
    infos = [eng.step(1)[0]]
    check(0)
    TP.assert_moments(eng, g, 0)
    infos += list(eng.step(n_steps - 1))
    eng.set_tapes()
    check(n_steps - 1)
    infos = np.asarray(infos, np.float64)
    ref = g["info"]
    k = ref.shape[1]
    for t in range(n_steps):
        print("ACTS", name, "info", t, infos[t, :k].tolist(), ref[t].tolist())
    np.testing.assert_array_equal(np.isnan(infos[:, :k]), np.isnan(ref))
    np.testing.assert_allclose(infos[:, :k], ref, rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
    tol = 2 * 3e-4 * n_steps + 1e-4
    for key in g:
        if not key.startswith("out_") or key == "out_log_alpha" or ":" in key:
            continue
        net, pname = key[4:].split(".", 1)
        TE.assert_params_close(eng.get_param(net, pname, g[key].shape), g[key], tol, key, bulk=0.99)
    if "out_log_alpha" in g:
        np.testing.assert_allclose(eng.get_param("tmp", "log_alpha"), g["out_log_alpha"].reshape(-1),
                                   rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", ["td7_tiny_acts_a", "td3_tiny_acts_a", "sac_tiny_acts_a"])
def test_programs_pass_audit_and_hazard_checks(name, monkeypatch):
    """RLE_AUDIT + RLE_HAZARD while every program of the engine is built, then one step."""
    monkeypatch.setenv("RLE_AUDIT", "1")
    monkeypatch.setenv("RLE_HAZARD", "1")
    g = load_golden(name)
    eng, rep, tp = engine_from_golden(g)
    TE.run_with_tapes(eng, tp, 1, lambda t: None)
    desc = eng.describe(0)
    assert any(f" {a}]" in desc for a in ("leaky", "silu", "gelu")), desc


# ---- shape edges -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(ACT_CASES))
def test_edge_case_trains_like_the_oracle(case):
    """tests/test_shape_edges_gpu.py's run protocol and criteria, unchanged, on each edge shape with the new
    activations (tests/more_acts.py ACT_CASES)."""
    more_acts.reference(case)
    with more_acts.registered(case):
        TSEG.test_edge_case_trains_like_the_oracle(case)


# (what rle_graph_describe names of each edge's path, as tests/test_shape_edges_gpu.py PATHS: the fusions an ELU
# net of the shape keeps stay on, the in-tile prologues are off)
EDGE_PATHS = [("acts-td3-k49", r"head\+dx", True), ("acts-td3-k49", r"\+pl", False),
              ("acts-td7-odd", r"head\+dx", False), ("acts-td7-odd", TSEG._BARE % "head", True),
              ("acts-td7-b1", r"head\+dx", True), ("acts-sac-h260", TSEG._BARE % "head", True),
              ("acts-sac-h260", TSEG._BARE % "sacfwd", True), ("acts-sac-a25", r"st\+sacpre", False)]


@pytest.mark.parametrize("case,pattern,present", EDGE_PATHS,
                         ids=[f"{c}-{'has' if p else 'no'}-{i}" for i, (c, t, p) in enumerate(EDGE_PATHS)])
def test_edge_takes_the_intended_path(case, pattern, present):
    more_acts.reference(case)
    with more_acts.registered(case):
        TSEG.test_edge_takes_the_intended_path(case, pattern, present)


# ---- offline modes -----------------------------------------------------------------------------------------------

def test_offline_td7_steps_match_oracle():
    """td7_tiny_acts_a with bc_lambda 0.1 (tests/test_offline_gpu.py's per-step check): the EPI_QDOT partials of
    the policy pass under a GELU critic."""
    TOFF.SHAPES["acts_a"] = lambda: load_golden("td7_tiny_acts_a")
    try:
        TOFF._per_step("acts_a", 0.1, 8)
    finally:
        del TOFF.SHAPES["acts_a"]


def test_offline_td3_steps_match_oracle():
    """td3_tiny_acts_c with bc_alpha 2.5 (tests/test_offline_td3_gpu.py's per-step check)."""
    TOFF3.SHAPES["td3_tiny_acts_c"] = lambda: load_golden("td3_tiny_acts_c")
    try:
        eng = TOFF3._per_step("td3_tiny_acts_c", 2.5, 6)
        assert " bc" in eng.describe(0) and " bc" not in eng.describe(1)
    finally:
        del TOFF3.SHAPES["td3_tiny_acts_c"]


# ---- the mirror --------------------------------------------------------------------------------------------------

def test_mirror_keeps_the_activations_across_copies_and_rebuilds():
    """TD3 through make_nn with SiLU critics and a GELU actor: the pickle round trip, the deepcopy and the engine
    rebuilt for another batch size keep agent.acts and rle_config's codes, and the copies act bit-identically
    before and after training on the same batch."""
    from rl.agent import TD3
    from rl.nn import MLPActor, MLPCritic
    from rl.replay_memory import SimpleReplayMemory
    from test_mirror_gpu import S, _fill, _transitions

    torch.manual_seed(11)

    def mk(state_dim, action_dim, **kw):
        return (MLPActor(state_dim, action_dim, 32, action_fn="GELU"),
                MLPCritic(state_dim, action_dim, 32, action_fn=torch.nn.SiLU()),
                MLPCritic(state_dim, action_dim, 32, action_fn="SiLU"))

    want = {"act_actor": "gelu", "act_critic": "silu"}
    codes = {k: E.ACT_CODES[v] for k, v in want.items()}
    ag = TD3("Tiny-v0", make_nn=mk, batch_size=16, seed=4)
    assert ag.acts == want
    ag2 = pickle.loads(pickle.dumps(ag))
    ag3 = copy.deepcopy(ag)
    obs = np.linspace(-1, 1, S).astype(np.float32)
    rep = SimpleReplayMemory(256, "Tiny-v0")
    _fill(rep, _transitions(100, 5))
    first = ag.sample(obs, deterministic=True)
    assert np.isfinite(first).all()
    for a in (ag, ag2, ag3):
        assert a.acts == want and {k: getattr(a.engine.cfg, k) for k in want} == codes
        np.testing.assert_array_equal(a.sample(obs, deterministic=True), first)
    infos = [a.train_n(rep, 48, 3) for a in (ag, ag2, ag3)]  # (the same draws: the copies share the stream position)
    assert infos[0] == infos[1] == infos[2] and np.isfinite(infos[0][0]["train/q_fn"])
    after = ag.sample(obs, deterministic=True)
    assert not np.array_equal(after, first)
    for a in (ag, ag2, ag3):
        assert a.batch_size == 48 and a.acts == want
        assert {k: getattr(a.engine.cfg, k) for k in want} == codes
        np.testing.assert_array_equal(a.sample(obs, deterministic=True), after)


# ---- the ELU ids still run ELU -----------------------------------------------------------------------------------

def test_elu_and_default_programs_after_a_new_activation_engine():
    """The new activations run under the ELU variant ids, told apart by a second dispatch.  In one process,
    after an engine that used them: an ELU golden (td3_tiny_act, the extended instance) and the default td7_tiny
    (the TD7 instance) still reproduce their goldens."""
    g = load_golden("td3_tiny_acts_a")
    eng, rep, tp = engine_from_golden(g)
    TE.run_with_tapes(eng, tp, 2, lambda t: None)
    for name in ("td3_tiny_act", "td7_tiny"):
        TE._trajectory(name, False)
        TE._trajectory(name, True)
    infos = np.asarray(eng.step(1), np.float64)  # (the first engine is still alive and still its own)
    assert np.isfinite(infos[0, 0])
