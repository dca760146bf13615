"""Row-major dot partials of the deferred AvgL1Norm backward (RLE_FUSE_NBROWS, kernels.hip nb_rows_issue).

The weight gradients whose dZ is an AvgL1Norm backward applied on load (the critics' first layer and the
encoder's) build two scalars per batch row, 1 / m and the sign coefficient.  With the fusion on, the producing
input gradient stores its per-tile dot partials row-major and a workgroup reads a row's partials in 1-4 float4
loads; with it off (``fuse_off=nbrows``) it issues the 32 clamped loads of the batched tables.  Both sum the same
partials in the same order, so the two plans must agree bit for bit -- parameters, Adam moments, priorities,
value bounds and info rows.

Shapes: td7_tiny (both users of the variant) and td7_tiny_b100 (a batch of 100 padded to 112 rows: the rows past
the batch carry zero gradients and must contribute nothing), 6 steps each, the smallest trajectories that run
plain, policy and hard-update steps.

Clamp branch: with a layer's weights and bias at zero every row of its output has mean|x| = 0 < 1e-8, so the
norm's denominator is the clamp and the sign coefficient is 0 (sale.py:11-13).  That case is compared with
oracle.agents' step: info rows at harness.LOSS_RTOL, the Adam first moments (the step's gradients) at
test_parity_gpu's |d| <= 1e-4 |ref| + 1e-4 max|ref|.
"""

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

E = pytest.importorskip("rl._engine")
from harness import LOSS_RTOL, engine_from_golden, parse, shape_of  # noqa: E402
from oracle import spec  # noqa: E402

STEPS = 6


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(name, plan):
    g = load_golden(name)
    alg, env, H, B, Ncap, n_fill, n_steps, use_lap, seed, extra = parse(g)
    assert n_steps >= STEPS
    eng, rep, tp = engine_from_golden(g, plan=plan)
    S, A, _ = spec.TASKS[env]
    names = {net: list(p) for net, p in spec.agent_params(alg, S, A, H, seed, **shape_of(g)).items()}
    out = {"desc": "\n".join(eng.describe(w) for w in (0, 1, 3))}
    eng.set_tapes(u=tp["u"][:STEPS], eps=tp["eps"][:STEPS], eps_pi=tp.get("eps_pi"))
    for t in range(STEPS):
        out[f"info_{t}"] = np.asarray(eng.step(1)[0]).copy()
        out[f"vb_{t}"] = eng.value_bounds().copy()
    eng.set_tapes()
    out["prio"] = rep.get_priority(Ncap).copy()
    out["state"] = eng.state_export(E.STATE_ALL).copy()  # every parameter and both Adam moments
    for net, ps in names.items():
        for p in ps:
            out[f"{net}/{p}"] = np.asarray(eng.get_param(net, p)).copy()
    return out


@pytest.mark.parametrize("name", ["td7_tiny", "td7_tiny_b100"])
def test_rows_on_and_off_agree_bitwise(name):
    on = _run(name, None)
    off = _run(name, E.make_plan(fuse_off=["nbrows"]))
    # the default plan takes the new path for both users of the variant, the other plan for none
    assert on["desc"].count("adam+nbr]") >= 3 and "adam+nb]" not in on["desc"], on["desc"]
    assert off["desc"].count("adam+nb]") >= 3 and "adam+nbr]" not in off["desc"], off["desc"]
    assert set(on) == set(off)
    for k in on:
        if k == "desc":
            continue
        assert on[k].shape == off[k].shape, k
        nbad = int((_bits(on[k]) != _bits(off[k])).sum())
        assert nbad == 0, (k, nbad, on[k].size)


def test_clamped_rows_match_oracle():
    """q1 / q2's first layer and the encoder's last at zero: every row of both normed tensors is clamped."""
    from oracle import agents
    from test_oracle import build_from_golden

    import torch

    g = load_golden("td7_tiny")
    alg, orc, orep, tp, n_steps, B = build_from_golden(g)
    eng, rep, tp2 = engine_from_golden(g)
    assert "adam+nbr]" in eng.describe(1)
    zeroed = [("q1", "q01"), ("q2", "q01"), ("encoder", "zs3")]
    nets = orc.nets()
    with torch.no_grad():
        for net, layer in zeroed:
            for p in (layer + ".weight", layer + ".bias"):
                nets[net][p].zero_()
                eng.set_param(net, p, np.zeros(tuple(nets[net][p].shape), np.float32))
    n = 2  # step 1 runs clamped; Adam's first step moves the weights off zero
    eng.set_tapes(u=tp2["u"][:n], eps=tp2["eps"][:n], eps_pi=tp2.get("eps_pi"))
    keys = ["train/encoder", "train/q_fn", "train/policy"]
    for t in range(n):
        info = eng.step(1)[0]
        i1, ind = agents.run_steps(orc, alg, orep, {k: v[t:t + 1] for k, v in tp.items()}, 1, B)
        np.testing.assert_array_equal(eng.last_indices(), ind[0])
        ref = np.array([np.nan if i1[0][k] is None else i1[0][k] for k in keys])
        print("step", t, "info", info[:3].tolist(), "oracle", ref.tolist())
        np.testing.assert_allclose(info[:3], ref, rtol=LOSS_RTOL, atol=1e-4, equal_nan=True)
        for key, r in agents.moments(orc).items():
            if not key.endswith(":m"):
                continue
            net, pname = key[:-2].split(".", 1)
            got = np.asarray(eng.get_adam(net, pname, 0, r.shape), np.float64)
            r = np.asarray(r, np.float64)
            scale = max(np.abs(r).max(), 1e-30)
            d = np.abs(got - r)
            lim = 1e-4 * np.abs(r) + 1e-4 * scale
            print("  ", key, "max |d| / lim", float((d / lim).max()), "scale", scale)
            assert (d <= lim).all(), (t, key, float(d.max()), float((d / lim).max()), scale)
    eng.set_tapes()
