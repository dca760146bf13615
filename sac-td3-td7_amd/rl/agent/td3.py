"""TD3 (rl/agent/td3.py:30-245) on the HIP engine."""

from __future__ import annotations

import numpy as np

from rl import _engine as E
from rl.agent.engine_agent import EngineAgent


class TD3(EngineAgent):
    """MLP actor + twin critics with target policy smoothing and delayed Polyak updates.

    Constructor arguments as the reference (td3.py:33-47) plus ``hidden``,
    ``batch_size``, ``seed`` and ``device`` (see TD7).

    ``offline=True`` trains from a fixed dataset with TD3+BC (Fujimoto & Gu 2021): on policy steps the actor
    objective is ``-lmbda * mean(Q) + mse(pi(s), a)`` with ``lmbda = alpha / mean|Q|.detach()`` (``a``: the
    batch's stored action; ``Q = min(q1, q2)`` as this code base's TD3 objective), and the info dict gains two
    keys, ``train/bc`` (the mse) and ``train/lmbda`` (None on other steps).  The recipe's state normalisation is
    the replay's ``normalize_states()`` and the agent's ``set_obs_norm``.  ``offline=False`` ignores ``alpha``.

    ``clip_grad_norm`` (keyword-only, default inf = off) clips the critics' optimizer (q1 + q2) every step and the
    policy's on policy steps to that global L2 norm, as ``torch.nn.utils.clip_grad_norm_`` would; ``norm/policy``
    stays the norm before clipping, and ``grad_clip_stats()`` reports each optimizer's last norm and coefficient.

    ``critic_layer_norm`` (keyword-only, default False) puts a parameter-free LayerNorm (``nn.LayerNorm(width,
    elementwise_affine=False)``, eps 1e-5) after every hidden Linear of q1, q2 and their targets, before the
    activation -- the critic of ReBRAC / RLPD -- in every pass of the device step; the state_dict is unchanged, and
    ``agent.q1`` / ``agent.q2`` give host copies (``rl.nn.MLPCritic``) that carry the norm.

    ``critic_dropout`` (keyword-only, default 0.0 = off; needs ``critic_layer_norm=True``) makes every hidden block of
    the critics ``Linear -> Dropout(p) -> LayerNorm -> activation``, the DroQ critic: inverted dropout as
    ``torch.nn.Dropout(p)`` in train mode, active in every critic pass of the device step (target, online, policy),
    drawn from a Philox stream of its own, and off in ``engine.eval_q`` (inference); the host copies carry it too.

    ``n_step`` (keyword-only, default 1 = one-step targets, at most 8) trains on n-step returns: the device sampler
    walks up to ``n_step`` consecutive rows of the sampled slot's episode (continuity is read from the data:
    ``next_state[i] == state[i + 1]`` bit for bit) and the critic target becomes ``R_n + gamma^hops * notdone *
    Q'(s_last')``; the info dict gains ``replay/hops``, the batch's mean hops.  ``replay.sample(B, n_step=n,
    discount=gamma)`` returns the same rows on the host; a host BATCH dict is refused.
    """

    ALG = "td3"
    ALGO = E.RLE_TD3
    OPTIM_NETS = ("policy", "q1", "q2")
    NULLABLE = ("train/policy", "norm/policy", "train/bc", "train/lmbda")
    offline = False  # (class defaults: an agent pickled before the offline mode existed loads as online)
    alpha = 2.5

    def __init__(self, env_id: str, discount_factor: float = 0.99, policy_lr: float = 3e-4,
                 critic_lr: float = 3e-4, exploration_noise: float = 0.1, target_policy_noise: float = 0.2,
                 noise_clip: float = 0.5, policy_freq: int = 2, tau: float = 0.005, use_lap: bool = False,
                 make_nn=None, *, hidden: int = 256, batch_size: int = 256, seed: int | None = None,
                 device=None, offline: bool = False, alpha: float = 2.5,
                 clip_grad_norm: float = float("inf"), critic_layer_norm: bool = False,
                 critic_dropout: float = 0.0, n_step: int = 1, **make_nn_kwargs) -> None:
        # (n-step returns: the device sampler hands the step the n-step reward, next state and discount factor)
        self._set_n_step(n_step)
        # (parameter-free LayerNorm after every hidden Linear of the critics and their targets, in the device step)
        self._set_layer_norm(critic_layer_norm)
        # (DroQ critics: dropout on every hidden Linear's output ahead of that LayerNorm, in the device step's passes)
        self._set_dropout(critic_dropout)
        self._set_clip(clip_grad_norm)  # (global-norm clipping of the critics' and the policy's optimizer steps)
        self.offline = bool(offline)
        self.alpha = float(alpha)
        if self.offline:  # (_ext: every engine this agent builds -- _rebuild, pickle, deepcopy, to() -- carries it)
            self._ext = dict(bc_alpha=self.alpha)
        self.discount_factor = discount_factor
        self.target_policy_noise = target_policy_noise
        self.exploration_noise = exploration_noise
        self.noise_clip = noise_clip
        self.policy_freq = policy_freq
        self.use_lap = use_lap
        self.tau = tau
        cfg = dict(use_lap=use_lap, discount=discount_factor, policy_lr=policy_lr, critic_lr=critic_lr,
                   tau=tau, target_policy_noise=target_policy_noise, noise_clip=noise_clip,
                   policy_freq=policy_freq)
        self._setup(env_id, hidden=hidden, batch_size=batch_size, seed=seed, device=device, make_nn=make_nn,
                    make_nn_kwargs=make_nn_kwargs, cfg=cfg)

    def _info_keys(self):
        keys = ("train/q_fn", "train/policy", "norm/policy")  # td3.py:226-235
        bc = getattr(self, "_ext", {}).get("bc_alpha", 0.0) > 0  # (the engine's offline programs: two more columns)
        return self._with_hops(keys + ("train/bc", "train/lmbda") if bc else keys)

    def sample(self, state, deterministic: bool = False, **kwargs):
        """td3.py:114-135: clip(tanh(policy(s)) + exploration_noise * randn, -1, 1) * scale + bias, one
        device program (rle_act_sample).  The noise comes from the engine's Philox stream (the
        reference uses torch's global generator); kwargs eps=[A] supplies it instead (parity)."""
        return self._act(state, deterministic, kwargs.get("eps"))

    @property
    def q1(self):
        """Host copy of the first critic (rl.nn.MLPCritic, LayerNorm included), from the device parameters."""
        return self._host_critic("q1")

    @property
    def q2(self):
        return self._host_critic("q2")

    def __repr__(self) -> str:
        return "TD3"
