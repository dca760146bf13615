"""Offline SAC (AWAC, Nair et al. 2020): the oracle's gradient step with the advantage-weighted policy step
(TEST INFRASTRUCTURE).

``AWACOracle`` restates ``oracle.agents.SACOracle.step`` (sac.py:251-295) at a fixed temperature of 0 with one
change, the policy phase (after the critic update, before Polyak):

    mu, l    = pi(s);  l = clamp(l, min_log_std, max_log_std);  sigma = exp(l)
    a_pi, lp = rsample(mu, sigma, eps_pi)                   # lp only feeds the `entropy` info
    adv      = min(q1, q2)(s, a) - min(q1, q2)(s, a_pi)     # updated critics, no gradient
    w        = min(exp(adv / lmbda), 100)                   # detached
    a_c      = clamp(a, -(1 - 1e-6), 1 - 1e-6)              # fp32 constants; a: the batch's stored action
    u        = atanh(a_c)
    logp     = sum_j [-(u - mu)^2 / (2 sigma^2) - l - 0.5 log(2 pi)] - sum_j log(1 - a_c^2 + EPS)
    L        = -mean(w * logp)

Info keys: ``train/q_fn``, ``train/policy`` (= L), ``entropy`` (= -mean lp), ``train/adv`` (mean adv),
``train/weight`` (mean w).  ``oracle.agents.run_steps`` drives it as it is.  With ``lmbda = 0`` (the term switched
off) the step is the online one at ``tmp = 0``, bit for bit (tests/test_offline_sac.py guards the restatement).
``awac_grads`` is the hand-written gradient of L with respect to the raw head, the formulas the device op uses.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from oracle import nets as N
from oracle.agents import SACOracle, _grads
from oracle import agents as _agents

INFO_KEYS = ("train/q_fn", "train/policy", "entropy", "train/adv", "train/weight")
W_MAX = 100.0
# the clamp bound of the dataset action: the fp32 value of 1 - 1e-6, in every precision the oracle runs in
A_MAX = float(np.float32(1.0) - np.float32(1e-6))
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def awac_logp(mean, log_std_raw, a, lo, hi):
    """log pi(a | s) of the squashed Gaussian at the dataset action a: [B, 1]."""
    ls = torch.clamp(log_std_raw, lo, hi)
    a_c = torch.clamp(a, -A_MAX, A_MAX)
    u = torch.atanh(a_c)
    lp = -((u - mean) ** 2) / (2 * (ls.exp() ** 2)) - ls - HALF_LOG_2PI
    return lp.sum(-1, keepdim=True) - torch.log(1 - a_c.pow(2.0) + N.EPS).sum(-1, keepdim=True)


def awac_grads(mean, log_std_raw, a, w, lo, hi):
    """dL/dmean and dL/dlog_std_raw of L = -(1/B) sum_i w_i logp_i, written out (no autograd):
    -(w/B) (u - mu) / sigma^2 and -(w/B) ((u - mu)^2 / sigma^2 - 1) where the clamp passes gradient, else 0."""
    B = mean.shape[0]
    ls = torch.clamp(log_std_raw, lo, hi)
    var = ls.exp() ** 2
    u = torch.atanh(torch.clamp(a, -A_MAX, A_MAX))
    d = u - mean
    wb = w.reshape(B, 1) / B
    g_mu = -wb * d / var
    g_ls = -wb * (d * d / var - 1.0)
    g_ls = torch.where((log_std_raw >= lo) & (log_std_raw <= hi), g_ls, torch.zeros_like(g_ls))
    return g_mu, g_ls


class AWACOracle(SACOracle):
    def __init__(self, nets, A, lmbda=1.0, **kw):
        kw["tmp"] = 0.0
        super().__init__(nets, A, **kw)
        self.lmbda = float(lmbda)
        self.last = None  # (the policy phase's mean, raw log_std, dataset action, weights and raw-head gradients)

    def step(self, batch, replay, eps, eps_pi):
        _tt = _agents._tt  # (looked up per call: edge_cases.float64_oracle swaps it)
        info = {}
        s, a, s2 = _tt(batch["state"]), _tt(batch["action"]), _tt(batch["next_state"])
        r, nd = _tt(batch["reward"]), _tt(batch["done"])
        with torch.no_grad():
            a2, lp2 = self._dist(s2, eps)
            nq = torch.min(N.mlp_critic(self.tq1, s2, a2, self.ac), N.mlp_critic(self.tq2, s2, a2, self.ac))
            alpha = self.tmp
            y = r + self.gamma * (nq - alpha * lp2) * nd
        q1, q2 = N.mlp_critic(self.q1, s, a, self.ac), N.mlp_critic(self.q2, s, a, self.ac)
        loss_q = torch.mean((y - q1) ** 2.0) * 0.5 + torch.mean((y - q2) ** 2.0) * 0.5
        g = _grads(loss_q, {**{"a" + k: v for k, v in self.q1.items()},
                            **{"b" + k: v for k, v in self.q2.items()}})
        self.opt_q.step(g)
        info["train/q_fn"] = float(loss_q.detach())
        keys = list(self.pi.keys())
        if self.lmbda == 0.0:  # the term switched off: the online policy phase at tmp = 0
            act, lp = self._dist(s, eps_pi)
            qv = torch.min(N.mlp_critic(self.q1, s, act, self.ac), N.mlp_critic(self.q2, s, act, self.ac))
            policy_obj = torch.mean(-qv + lp * self.tmp)
            entropy = -(lp.mean().detach())
            gs = torch.autograd.grad(policy_obj, [self.pi[k] for k in keys])
            self.opt_pi.step(gs)
            info["train/policy"] = float(policy_obj.detach())
            info["entropy"] = float(entropy)
            self._polyak()
            self.n_runs += 1
            return info
        out = N.mlp(self.pi, s, self.ap)
        mean, log_std = out.chunk(2, -1)
        with torch.no_grad():
            a_pi, lp = N.gaussian_tanh(mean, log_std, _tt(eps_pi), self.lo, self.hi)
            q_d = torch.min(N.mlp_critic(self.q1, s, a, self.ac), N.mlp_critic(self.q2, s, a, self.ac))
            v = torch.min(N.mlp_critic(self.q1, s, a_pi, self.ac), N.mlp_critic(self.q2, s, a_pi, self.ac))
            adv = q_d - v
            w = torch.exp(adv / self.lmbda).clamp(max=W_MAX)
        logp = awac_logp(mean, log_std, a, self.lo, self.hi)
        loss_p = -(w * logp).mean()
        g_mu, g_ls = torch.autograd.grad(loss_p, [mean, log_std], retain_graph=True)
        self.last = {"mean": mean.detach().clone(), "log_std": log_std.detach().clone(), "a": a.clone(),
                     "w": w.clone(), "g_mean": g_mu.clone(), "g_log_std": g_ls.clone()}
        gs = torch.autograd.grad(loss_p, [self.pi[k] for k in keys])
        self.opt_pi.step(gs)
        info["train/policy"] = float(loss_p.detach())
        info["entropy"] = float(-(lp.mean()))
        info["train/adv"] = float(adv.mean())
        info["train/weight"] = float(w.mean())
        self._polyak()
        self.n_runs += 1
        return info
