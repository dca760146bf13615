"""Offline TD3 (TD3+BC): the oracle's gradient step with the behaviour-cloning term (TEST INFRASTRUCTURE).

``TD3BCOracle`` restates ``oracle.agents.TD3Oracle.step`` (td3.py:206-242) with one change, the actor
objective of a policy step:

    pi    = tanh(policy(s))
    Q     = min(q1(s, pi), q2(s, pi))                 # this code base's TD3 objective, td3.py:191
    lmbda = alpha / Q.abs().mean().detach()           # no guard for mean|Q| = 0, as in the paper's code
    loss  = -lmbda * Q.mean() + mse_loss(pi, a)       # a: the batch's stored action; mse over B x A

It returns two more info keys on policy steps, ``train/bc`` (the mse) and ``train/lmbda`` (None on other
steps, as ``train/policy``); ``norm/policy`` is that of the whole loss.  ``oracle.agents.run_steps`` drives
it as it is.  With ``alpha = 0`` the step is the online one, bit for bit (tests/test_offline_td3.py guards
the restatement).
"""

from __future__ import annotations

import torch

from oracle import nets as N
from oracle.agents import TD3Oracle, _grads, _tt

INFO_KEYS = ("train/q_fn", "train/policy", "norm/policy", "train/bc", "train/lmbda")


def build_offline_td3(g, alpha):
    """test_oracle.build_from_golden with a TD3BCOracle of ``alpha`` in the oracle's place: the same nets,
    hyper-parameters, replay and tapes.  Returns (oracle, replay, tapes, n_steps, B)."""
    from conftest import acts_of, shape_of
    from oracle import spec
    from test_oracle import build_from_golden

    alg, on, rep, tp, n_steps, B = build_from_golden(g)
    assert alg == "td3"
    H, _, _, _, _, use_lap, seed = (int(x) for x in g["meta"])
    S, A, _ = spec.TASKS[str(g["meta_env"])]
    nets = spec.agent_params(alg, S, A, H, seed, **shape_of(g))
    orc = TD3BCOracle(nets, alpha=alpha, discount=on.gamma, policy_lr=on.opt_pi.lr, critic_lr=on.opt_q.lr,
                      target_policy_noise=on.noise, noise_clip=on.clip, policy_freq=on.pf, tau=on.tau,
                      use_lap=bool(use_lap), acts=acts_of(g))
    return orc, rep, tp, n_steps, B


class TD3BCOracle(TD3Oracle):
    def __init__(self, nets, alpha=2.5, **kw):
        super().__init__(nets, **kw)
        self.alpha = float(alpha)
        self.last_action_grads = None  # (policy steps) d loss / d pi(s): (the Q part, the BC part), [B, A] each

    def step(self, batch, replay, eps):
        info = {}
        s, a, s2 = _tt(batch["state"]), _tt(batch["action"]), _tt(batch["next_state"])
        r, nd = _tt(batch["reward"]), _tt(batch["done"])
        with torch.no_grad():
            noise = (_tt(eps) * self.noise).clamp(-self.clip, self.clip)
            a2 = (torch.tanh(N.mlp(self.pi, s2, self.ap)) + noise).clamp(-1.0, 1.0)
            nv = torch.min(N.mlp_critic(self.tq1, s2, a2, self.ac), N.mlp_critic(self.tq2, s2, a2, self.ac))
            y = r + self.gamma * nv * nd
        q1, q2 = N.mlp_critic(self.q1, s, a, self.ac), N.mlp_critic(self.q2, s, a, self.ac)
        if self.lap:
            d1, d2 = (q1 - y).abs(), (q2 - y).abs()

            def hub(d):
                return torch.where(d < 1.0, 0.5 * d.pow(2), 1.0 * d).mean()

            loss_q = hub(d1) + hub(d2)
            prio = torch.max(d1, d2).clamp(1.0).pow(0.4).view(-1)
            replay.update_priority(prio.detach().numpy())
        else:
            loss_q = torch.mean((y - q1) ** 2.0) * 0.5 + torch.mean((y - q2) ** 2.0) * 0.5
        g = _grads(loss_q, {**{"a" + k: v for k, v in self.q1.items()},
                            **{"b" + k: v for k, v in self.q2.items()}})
        self.opt_q.step(g)
        info["train/q_fn"] = float(loss_q.detach())
        info["train/policy"] = info["norm/policy"] = info["train/bc"] = info["train/lmbda"] = None
        if self.n_runs % self.pf == 0:
            act = torch.tanh(N.mlp(self.pi, s, self.ap))
            Q = torch.min(N.mlp_critic(self.q1, s, act, self.ac), N.mlp_critic(self.q2, s, act, self.ac))
            loss_p = -Q.mean()
            if self.alpha != 0.0:
                lmbda = self.alpha / Q.abs().mean().detach()
                bc = torch.nn.functional.mse_loss(act, a)
                q_part = -lmbda * Q.mean()
                loss_p = q_part + bc
                g_q, = torch.autograd.grad(q_part, act, retain_graph=True)
                g_bc, = torch.autograd.grad(bc, act, retain_graph=True)
                self.last_action_grads = (g_q.detach().clone(), g_bc.detach().clone())
                info["train/bc"] = float(bc.detach())
                info["train/lmbda"] = float(lmbda)
            gp = _grads(loss_p, self.pi)
            info["train/policy"] = float(loss_p.detach())
            tot = 0.0
            for gg in gp:  # nn/utils.py:13-19: sum of per-tensor L2 norms
                tot += torch.norm(gg, p=2)
            info["norm/policy"] = float(tot)
            self.opt_pi.step(gp)
            with torch.no_grad():  # td3.py:194-204 (policy term aliases itself, Q2)
                for src, dst in ((self.q1, self.tq1), (self.q2, self.tq2), (self.pi, self.pi)):
                    for k in src:
                        dst[k].copy_(self.tau * src[k] + dst[k] * (1 - self.tau))
        self.n_runs += 1
        return info
