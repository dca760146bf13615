"""TD7 (rl/agent/td7.py:31-332) on the HIP engine."""

from __future__ import annotations

import numpy as np

from rl import _engine as E
from rl.agent.engine_agent import EngineAgent


class TD7(EngineAgent):
    """SALE encoder + actor + twin critics, LAP, value clipping, fixed/target encoders.

    Same constructor arguments as the reference (td7.py:34-48) plus ``hidden``
    (hdim = zs_dim), ``batch_size`` (the captured step's B; train_ops with another
    B rebuilds the step graphs), ``seed`` (weight init + Philox stream) and ``device``.

    ``offline=True`` trains from a fixed dataset (the TD7 paper's offline mode, which the reference names
    and does not implement): on policy steps the actor objective gains the behaviour-cloning term
    ``lmbda * mean|Q|.detach() * mse(pi(s), a)`` (``a``: the batch's stored action), and the info dict
    two keys, ``train/bc`` (the mse) and ``train/q_abs`` (None on other steps).  ``offline=False``
    ignores ``lmbda``.

    ``clip_grad_norm`` (keyword-only, default inf = off) clips the encoder's and the critics' (q1 + q2)
    optimizers every step and the policy's on policy steps to that global L2 norm, as
    ``torch.nn.utils.clip_grad_norm_`` would; ``grad_clip_stats()`` reports each one's last norm and coefficient.
    """

    ALG = "td7"
    ALGO = E.RLE_TD7
    OPTIM_NETS = ("encoder", "policy", "q1", "q2")
    NULLABLE = ("train/policy", "train/bc", "train/q_abs")
    offline = False  # (class defaults: an agent pickled before the offline mode existed loads as online)
    lmbda = 0.1

    def __init__(self, env_id: str, discount_factor: float = 0.99, policy_lr: float = 3e-4,
                 critic_lr: float = 3e-4, target_update_rate: int = 250, exploration_noise: float = 0.1,
                 target_policy_noise: float = 0.2, noise_clip: float = 0.5, policy_freq: int = 2,
                 use_lap: bool = False, make_nn=None, *, hidden: int = 256, batch_size: int = 256,
                 seed: int | None = None, device=None, offline: bool = False, lmbda: float = 0.1,
                 clip_grad_norm: float = float("inf"), n_step: int = 1, **make_nn_kwargs) -> None:
        # (n_step > 1 raises: the encoder learns the one-step model zsa(s, a) -> zs(s') from the same next-state rows)
        self._set_n_step(n_step)
        self._set_clip(clip_grad_norm)  # (global-norm clipping of the encoder's, critics' and policy's optimizer steps)
        self.discount_factor = discount_factor
        self.target_update_rate = target_update_rate
        self.target_policy_noise = target_policy_noise
        self.exploration_noise = exploration_noise
        self.noise_clip = noise_clip
        self.policy_freq = policy_freq
        self.use_lap = use_lap
        cfg = dict(use_lap=use_lap, discount=discount_factor, policy_lr=policy_lr, critic_lr=critic_lr,
                   target_policy_noise=target_policy_noise, noise_clip=noise_clip, policy_freq=policy_freq,
                   target_update_rate=target_update_rate)
        self.offline = bool(offline)
        self.lmbda = float(lmbda)
        if self.offline:  # (in _cfg: every engine this agent builds -- _rebuild, pickle, deepcopy, to() -- carries it)
            cfg["bc_lambda"] = self.lmbda
        self._setup(env_id, hidden=hidden, batch_size=batch_size, seed=seed, device=device, make_nn=make_nn,
                    make_nn_kwargs=make_nn_kwargs, cfg=cfg)

    def _info_keys(self):
        keys = ("train/encoder", "train/q_fn", "train/policy")  # td7.py:302,314,317
        bc = getattr(self, "_cfg", {}).get("bc_lambda", 0.0) > 0  # (the engine's offline programs: two more columns)
        return keys + ("train/bc", "train/q_abs") if bc else keys

    @property
    def value_max(self):
        return float(self.engine.value_bounds()[0])

    @property
    def value_min(self):
        return float(self.engine.value_bounds()[1])

    @property
    def value_target_max(self):
        return float(self.engine.value_bounds()[2])

    @property
    def value_target_min(self):
        return float(self.engine.value_bounds()[3])

    def sample(self, state, deterministic: bool = False, **kwargs):
        """td7.py:141-156: clip(tanh(policy(s)) + exploration_noise * randn, -1, 1) * scale + bias, one
        device program (rle_act_sample).  The noise comes from the engine's Philox stream (the
        reference uses torch's global generator); kwargs eps=[A] supplies it instead (parity)."""
        return self._act(state, deterministic, kwargs.get("eps"))

    def __repr__(self) -> str:
        return "TD7"
