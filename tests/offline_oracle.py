"""TD7 offline mode: the oracle's gradient step with the paper's behaviour-cloning term (TEST INFRASTRUCTURE).

``TD7BCOracle`` restates ``oracle.agents.TD7Oracle.step`` (td7.py:287-332) with one change, the actor
objective of a policy step:

    Q          = cat([q1(s, pi(s)), q2(s, pi(s))], 1)          # td7.py:259-276, the updated critics
    actor_loss = -Q.mean() + lmbda * Q.abs().mean().detach() * mse_loss(pi(s), a)

``a`` is the batch's stored action, ``mse_loss`` the mean over B x A elements.  It returns two more info
keys on policy steps, ``train/bc`` (the mse) and ``train/q_abs`` (None on other steps, as ``train/policy``).
``oracle.agents.run_steps`` drives it as it is.  With ``lmbda = 0`` the step is the online one, bit for bit
(tests/test_offline.py guards the restatement).
"""

from __future__ import annotations

import torch

from oracle.agents import TD7Oracle, _grads, _tt

INFO_KEYS = ("train/encoder", "train/q_fn", "train/policy", "train/bc", "train/q_abs")


def build_offline(g, lmbda):
    """test_oracle.build_from_golden with a TD7BCOracle of weight ``lmbda`` in the oracle's place: the same
    nets, hyper-parameters, replay and tapes.  Returns (oracle, replay, tapes, n_steps, B)."""
    from conftest import acts_of, shape_of
    from oracle import spec
    from test_oracle import build_from_golden

    alg, on, rep, tp, n_steps, B = build_from_golden(g)
    assert alg == "td7"
    H, _, _, _, _, use_lap, seed = (int(x) for x in g["meta"])
    S, A, _ = spec.TASKS[str(g["meta_env"])]
    nets = spec.agent_params(alg, S, A, H, seed, **shape_of(g))
    orc = TD7BCOracle(nets, lmbda=lmbda, discount=on.gamma, policy_lr=on.opt_pi.lr, critic_lr=on.opt_q.lr,
                      target_update_rate=on.tr, target_policy_noise=on.noise, noise_clip=on.clip,
                      policy_freq=on.pf, use_lap=bool(use_lap), acts=acts_of(g))
    return orc, rep, tp, n_steps, B


class TD7BCOracle(TD7Oracle):
    def __init__(self, nets, lmbda=0.1, **kw):
        super().__init__(nets, **kw)
        self.lmbda = float(lmbda)
        self.last_action_grads = None  # (policy steps) d loss / d pi(s): (the Q part, the BC part), [B, A] each

    def step(self, batch, replay, eps):
        self.n_runs += 1
        info = {}
        s, a, s2 = _tt(batch["state"]), _tt(batch["action"]), _tt(batch["next_state"])
        r, nd = _tt(batch["reward"]), _tt(batch["done"])
        # encoder (td7.py:246-257, 299-303)
        zs_, zsa_, actor, critic = self._fns()
        with torch.no_grad():
            zs_next = zs_(self.enc, s2)
        zsa = zsa_(self.enc, zs_(self.enc, s), a)
        loss_e = (zsa - zs_next).pow(2.0).mean()
        self.opt_enc.step(_grads(loss_e, self.enc))
        info["train/encoder"] = float(loss_e.detach())
        # critics (td7.py:175-244)
        with torch.no_grad():
            zs2 = zs_(self.fet, s2)
            noise = (_tt(eps) * self.noise).clamp(-self.clip, self.clip)
            a2 = (actor(self.pi, s2, zs2) + noise).clamp(-1.0, 1.0)
            zsa2 = zsa_(self.fet, zs2, a2)
            nq1 = critic(self.tq1, s2, a2, zsa2, zs2)
            nq2 = critic(self.tq2, s2, a2, zsa2, zs2)
            nv = torch.cat([nq1, nq2], -1).min(1, keepdim=True)[0].clamp(self.vt_min, self.vt_max)
            y = r + self.gamma * nv * nd
            self.value_max = max(self.value_max, float(y.max()))
            self.value_min = min(self.value_min, float(y.min()))
            zs = zs_(self.fe, s)
            zsa_f = zsa_(self.fe, zs, a)
        q1 = critic(self.q1, s, a, zsa_f, zs)
        q2 = critic(self.q2, s, a, zsa_f, zs)
        if self.lap:
            td = torch.cat([(q1 - y).abs(), (q2 - y).abs()], 1)
            loss_q = torch.where(td < 1.0, 0.5 * td.pow(2), 1.0 * td).sum(1).mean()
            prio = td.max(1)[0].clamp(1.0).pow(0.4).view(-1)
            replay.update_priority(prio.detach().numpy())
        else:
            loss_q = torch.mean((y - q1) ** 2.0) * 0.5 + torch.mean((y - q2) ** 2.0) * 0.5
        g = _grads(loss_q, {**{"a" + k: v for k, v in self.q1.items()},
                            **{"b" + k: v for k, v in self.q2.items()}})
        self.opt_q.step(g)
        info["train/q_fn"] = float(loss_q.detach())
        # policy (td7.py:259-276, 319-324) + the behaviour-cloning term
        info["train/policy"] = info["train/bc"] = info["train/q_abs"] = None
        if self.n_runs % self.pf == 0:
            zs = zs_(self.fe, s)
            act = actor(self.pi, s, zs)
            zsa_p = zsa_(self.fe, zs, act)
            qa = critic(self.q1, s, act, zsa_p, zs)
            qb = critic(self.q2, s, act, zsa_p, zs)
            Q = torch.cat([qa, qb], -1)
            loss_p = -Q.mean()
            if self.lmbda != 0.0:
                q_abs = Q.abs().mean().detach()
                bc = torch.nn.functional.mse_loss(act, a)
                loss_q_part = loss_p
                loss_p = loss_q_part + self.lmbda * q_abs * bc
                g_q, = torch.autograd.grad(loss_q_part, act, retain_graph=True)
                g_bc, = torch.autograd.grad(self.lmbda * q_abs * bc, act, retain_graph=True)
                self.last_action_grads = (g_q.detach().clone(), g_bc.detach().clone())
                info["train/bc"] = float(bc.detach())
                info["train/q_abs"] = float(q_abs)
            self.opt_pi.step(_grads(loss_p, self.pi))
            info["train/policy"] = float(loss_p.detach())
        # hard update (td7.py:278-285, 325-331)
        if self.n_runs % self.tr == 0:
            with torch.no_grad():
                for dst, src in ((self.tq1, self.q1), (self.tq2, self.q2),
                                 (self.fet, self.fe), (self.fe, self.enc)):
                    for k in dst:
                        dst[k].copy_(src[k])
            self.vt_max, self.vt_min = self.value_max, self.value_min
            if self.lap:
                replay.reset_max_priority()
        return info
