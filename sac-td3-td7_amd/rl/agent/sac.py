"""SAC (rl/agent/sac.py:24-299) on the HIP engine."""

from __future__ import annotations

import numpy as np

from rl import _engine as E
from rl.agent.engine_agent import EngineAgent


class SAC(EngineAgent):
    """Squashed-Gaussian actor, twin critics, Polyak targets, optional auto temperature.

    Constructor arguments as the reference (sac.py:27-42) plus ``hidden``,
    ``batch_size``, ``seed`` and ``device``.  ``max_grad_norm`` is stored but, as in
    the reference, never applied (a reference script runs unchanged); the keyword-only
    ``clip_grad_norm`` is what clips: every step, the critics' optimizer (q1 + q2) and the
    policy's are each clipped to that global L2 norm in the device step, as
    ``torch.nn.utils.clip_grad_norm_`` would (the temperature is never clipped);
    ``grad_clip_stats()`` reports each optimizer's last norm and coefficient.

    ``offline=True`` trains from a fixed dataset with AWAC (Nair et al. 2020): the critic step is SAC's at a fixed
    temperature of 0, and the policy step maximises the advantage-weighted log-likelihood of the batch's stored
    action, ``L = -mean(w * log pi(a | s))`` with ``w = min(exp((Q(s, a) - Q(s, a_pi)) / lmbda), 100)`` detached
    (``Q = min(q1, q2)`` of the updated critics, ``a_pi`` the policy's own rsample).  No gradient passes through
    the critics.  The info dict is ``train/q_fn``, ``train/policy``, ``entropy``, ``train/adv`` (mean advantage)
    and ``train/weight`` (mean w).  ``offline`` forces ``tmp = 0``; ``offline=False`` ignores ``lmbda``.

    ``critic_layer_norm`` (keyword-only, default False) puts a parameter-free LayerNorm (``nn.LayerNorm(width,
    elementwise_affine=False)``, eps 1e-5) after every hidden Linear of q1, q2 and their targets, before the
    activation, in every pass of the device step (AWAC's forward-only passes included); the state_dict is
    unchanged, and ``agent.q1`` / ``agent.q2`` give host copies (``rl.nn.MLPCritic``) that carry the norm.

    ``critic_dropout`` (keyword-only, default 0.0 = off; needs ``critic_layer_norm=True``) makes every hidden block of
    the critics ``Linear -> Dropout(p) -> LayerNorm -> activation``, the DroQ critic: inverted dropout as
    ``torch.nn.Dropout(p)`` in train mode, active in every critic pass of the device step (target, online, policy),
    drawn from a Philox stream of its own, and off in ``engine.eval_q`` (inference); the host copies carry it too.

    ``n_step`` (keyword-only, default 1 = one-step targets, at most 8) trains on n-step returns: the device sampler
    walks up to ``n_step`` consecutive rows of the sampled slot's episode (continuity is read from the data:
    ``next_state[i] == state[i + 1]`` bit for bit) and the critic target becomes ``R_n + gamma^hops * notdone *
    (min Q' - alpha logpi)(s_last')``; the info dict gains ``replay/hops``, the batch's mean hops.
    ``replay.sample(B, n_step=n, discount=gamma)`` returns the same rows on the host; a host BATCH dict is refused."""

    ALG = "sac"
    ALGO = E.RLE_SAC
    OPTIM_NETS = ("policy", "q1", "q2")
    offline = False  # (class defaults: an agent pickled before the offline mode existed loads as online)
    lmbda = 1.0

    def __init__(self, env_id: str, discount_factor: float = 0.99, policy_lr: float = 3e-4,
                 critic_lr: float = 3e-4, min_log_std: float = -20.0, max_log_std: float = 2.0,
                 tau: float = 0.005, tmp: float = -1.0, use_lap: bool = False,
                 max_grad_norm: float = float("inf"), make_nn=None, *, hidden: int = 256,
                 batch_size: int = 256, seed: int | None = None, device=None, offline: bool = False,
                 lmbda: float = 1.0, clip_grad_norm: float = float("inf"), critic_layer_norm: bool = False,
                 critic_dropout: float = 0.0, n_step: int = 1, **make_nn_kwargs) -> None:
        # (n-step returns: the device sampler hands the step the n-step reward, next state and discount factor)
        self._set_n_step(n_step)
        # (parameter-free LayerNorm after every hidden Linear of the critics and their targets, in the device step)
        self._set_layer_norm(critic_layer_norm)
        # (DroQ critics: dropout on every hidden Linear's output ahead of that LayerNorm, in the device step's passes)
        self._set_dropout(critic_dropout)
        # (clip_grad_norm: global-norm clipping of the critics' and the policy's optimizer steps, applied in the
        # device step; the positional max_grad_norm stays what it is in the reference -- stored, never applied)
        self._set_clip(clip_grad_norm)
        self.offline = bool(offline)
        self.lmbda = float(lmbda)
        if self.offline:
            if tmp not in (-1.0, 0.0):
                raise ValueError("SAC(offline=True) runs at a fixed temperature of 0: leave tmp at its default or pass 0")
            if not (self.lmbda > 0.0 and np.isfinite(self.lmbda)):
                raise ValueError("SAC(offline=True): lmbda must be a finite value > 0")
            tmp = 0.0
            # (_ext: every engine this agent builds -- _rebuild, pickle, deepcopy, to() -- carries it)
            self._ext = dict(awac_lambda=self.lmbda)
        self.auto_tmp_mode = tmp < 0.0
        self.discount_factor = discount_factor
        self.min_log_std, self.max_log_std = min_log_std, max_log_std
        self.tau = tau
        self.use_lap = use_lap
        self.max_grad_norm = max_grad_norm
        cfg = dict(use_lap=use_lap, discount=discount_factor, policy_lr=policy_lr, critic_lr=critic_lr,
                   tau=tau, min_log_std=min_log_std, max_log_std=max_log_std, tmp=tmp)
        self._setup(env_id, hidden=hidden, batch_size=batch_size, seed=seed, device=device, make_nn=make_nn,
                    make_nn_kwargs=make_nn_kwargs, cfg=cfg)
        if self.auto_tmp_mode:
            self.target_entropy = -self.action_dim

    def train_ops(self, batch, replay_buffer=None, *args, **kwargs):
        if self.use_lap:
            # sac.py:199-203 calls self._lap_huber, which SAC does not define
            raise AttributeError("'SAC' object has no attribute '_lap_huber' (reference sac.py:202)")
        return super().train_ops(batch, replay_buffer, *args, **kwargs)

    def train_n(self, replay_buffer, batch_size, n_ops):
        if self.use_lap:
            raise AttributeError("'SAC' object has no attribute '_lap_huber' (reference sac.py:202)")
        return super().train_n(replay_buffer, batch_size, n_ops)

    def _info_keys(self):
        if getattr(self, "_ext", {}).get("awac_lambda", 0.0) > 0:  # (the engine's offline programs)
            keys = ("train/q_fn", "train/policy", "entropy", "train/adv", "train/weight")
        elif self.auto_tmp_mode:  # sac.py:268-290
            keys = ("train/q_fn", "tmp", "norm/tmp", "train/policy", "train/tmp", "entropy")
        else:
            keys = ("train/q_fn", "train/policy", "entropy")
        return self._with_hops(keys)

    @property
    def tmp(self):
        """exp-space temperature parameter: log_alpha (auto mode) or the fixed value."""
        if not self.auto_tmp_mode:  # sac.py:56-60: the fixed float itself
            return float(self._cfg["tmp"])
        return float(self.engine.get_param("tmp", "log_alpha")[0])

    def _inference(self, state):
        """sac.py:154-159: Normal(mean, exp(clamp(log_std))) from the device actor head."""
        import torch

        raw = torch.from_numpy(self._forward(state, 2 * self.action_dim))
        mean, log_std = raw.chunk(2, dim=-1)
        log_std = torch.clamp(log_std, self.min_log_std, self.max_log_std)
        return torch.distributions.Normal(mean, log_std.exp())

    def sample(self, state, deterministic: bool = False, **kwargs):
        """sac.py:132-152: tanh(mean) or tanh(mean + std * randn) (rsample), * scale + bias, one
        device program (rle_act_sample; engine Philox stream, or kwargs eps=[A] for parity)."""
        return self._act(state, deterministic, kwargs.get("eps"))

    @property
    def q1(self):
        """Host copy of the first critic (rl.nn.MLPCritic, LayerNorm included), from the device parameters."""
        return self._host_critic("q1")

    @property
    def q2(self):
        return self._host_critic("q2")

    def __repr__(self) -> str:
        return "SAC"
