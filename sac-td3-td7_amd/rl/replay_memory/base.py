"""Replay memories held in HBM (rl/replay_memory/base.py:9-26 interface).

The reference keeps float64 NumPy rings on the host and casts gathered rows to
float32 tensors in ``sample`` (lap.py:55-60).  Here the ring lives on the GPU as
float32 structure-of-arrays (``rle_replay_*`` in include/rle.h), which is the
same data after that cast.  Host appends are staged and flushed in one batched
copy before any device use, so the per-env-step cost is a host memcpy.
"""

from __future__ import annotations

from typing import Any

import numpy as np

from rl import _engine as E
from rl.replay_memory import snapshot as S
from rl.utils.envs import get_action_bias_scale, get_state_action_dims


def _device_index(device) -> int:
    """GPU index of a device spelling (None, k, "cuda", "cuda:k", "hip:k"); "cpu" is -1."""
    if device is None:
        return 0
    if isinstance(device, int):
        return device
    s = str(device)
    if s == "cpu":
        return -1
    if s.startswith("cuda") or s.startswith("hip"):
        return int(s.split(":")[1]) if ":" in s else 0
    raise ValueError(f"unsupported device {device!r}")


class DeviceBatch(dict):
    """The BATCH dict (annotation.py:23-30) plus the indices and replay it was drawn from.

    Engine-backed ``train_ops`` trains on rows ``ind`` of ``replay`` on the device;
    the tensors in the dict are the host copy the reference would have built.
    """

    def __init__(self, data, ind: np.ndarray, replay: "BaseReplayMemory"):
        super().__init__(data)
        self.ind = ind
        self.replay = replay


class BaseReplayMemory:
    """Device ring of (state, action, reward, next_state, notdone) rows."""

    LAP = False
    STAGE = 4096  # host rows staged before one batched H2D append
    # dataset state normalisation (normalize_states): plain attributes, so they travel with pickle, deepcopy and
    # to() through _host_attrs (class defaults: a replay pickled before they existed loads as not normalised)
    states_normalized = False
    state_mean = None
    state_scale = None

    def __init__(self, replay_buffer_size: int, env_id: str | None = None, *, state_dim: int | None = None,
                 action_dim: int | None = None, device: int = 0, **kwargs) -> None:
        self.replay_buffer_size = int(replay_buffer_size)
        if env_id is not None:
            state_dim, action_dim = get_state_action_dims(env_id)
            self.action_bias, self.action_scale = get_action_bias_scale(env_id)
        else:
            if state_dim is None or action_dim is None:
                raise ValueError("need env_id or state_dim/action_dim")
            self.action_bias = np.zeros(action_dim, np.float32)
            self.action_scale = np.ones(action_dim, np.float32)
        self.env_id = env_id
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        self.device = int(device)
        self.dev = E.Replay(self.replay_buffer_size, self.state_dim, self.action_dim, self.LAP, self.device)
        self._stage: list[tuple] = []
        self._ind = None
        self._ind_src = None  # engine whose last step drew the current indices

    # ---- appends ---------------------------------------------------------
    def _normalise(self, action):
        # lap.py:35 / simple.py:32, in the operands' own NumPy dtypes like the reference
        return np.asarray(action) / self.action_scale - self.action_bias

    def append(self, transition: list[Any]) -> None:
        """lap.py:31-43: one transition [obs, action, reward, next_obs, float_done]."""
        assert len(transition) == 5
        obs, action, reward, next_obs, float_done = transition
        self._stage.append((obs, self._normalise(action), reward, next_obs, float_done))
        if len(self._stage) >= self.STAGE:
            self.flush()

    def append_batch(self, obs, action, reward, next_obs, float_done) -> None:
        """Vectorised append of n transitions (row order = append order)."""
        self.flush()
        a = self._normalise(np.asarray(action).reshape(-1, self.action_dim))
        self.dev.append(np.asarray(obs).reshape(-1, self.state_dim), a, np.asarray(reward).reshape(-1),
                        np.asarray(next_obs).reshape(-1, self.state_dim), np.asarray(float_done).reshape(-1))

    def flush(self) -> None:
        if not self._stage:
            return
        st, a, r, s2, d = zip(*self._stage)
        self._stage = []
        n = len(r)
        self.dev.append(np.asarray(st, np.float64).reshape(n, self.state_dim).astype(np.float32),
                        np.asarray(a, np.float64).reshape(n, self.action_dim).astype(np.float32),
                        np.asarray(r, np.float64).reshape(n).astype(np.float32),
                        np.asarray(s2, np.float64).reshape(n, self.state_dim).astype(np.float32),
                        np.asarray(d, np.float64).reshape(n).astype(np.float32))

    # ---- state -----------------------------------------------------------
    @property
    def ptr(self) -> int:
        self.flush()
        return self.dev.state()[0]

    @property
    def size(self) -> int:
        self.flush()
        return self.dev.state()[1]

    def __len__(self) -> int:
        """lap.py:75-76: the write pointer (not the size) — kept as in the reference."""
        return self.ptr

    @property
    def ind(self):
        """Indices of the last batch: from sample(), or from the engine's last fused step."""
        if self._ind_src is not None:
            self._ind = self._ind_src.last_indices()
            self._ind_src = None
        return self._ind

    @ind.setter
    def ind(self, value):
        self._ind = None if value is None else np.asarray(value, np.int64)
        self._ind_src = None

    def _mark_engine_indices(self, eng) -> None:
        self._ind_src = eng

    # ---- dataset state normalisation ---------------------------------------
    def normalize_states(self, eps: float = 1e-3):
        """The TD3+BC recipe, on the device: per-feature mean and population std of ``state`` over the filled
        rows (rle_replay_state_stats), then ``state`` and ``next_state`` <- ``(x - mean) / (std + eps)``
        (rle_replay_normalize_states).  Returns ``(mean, std + eps)`` as fp32 arrays -- what
        ``agent.set_obs_norm`` takes.  A replay is normalised once: a second call raises RuntimeError."""
        if self.states_normalized:
            raise RuntimeError("normalize_states: this replay's states are already normalised")
        self.flush()
        mean, std = self.dev.state_stats()
        scale = std + np.float32(eps)
        self.dev.normalize_states(mean, scale)
        self.states_normalized = True
        self.state_mean, self.state_scale = mean, scale
        return mean, scale

    # ---- sampling --------------------------------------------------------
    def sample(self, batch_size: int, use_torch: bool = True, *, n_step: int = 1, discount: float = 0.99):
        """lap.py:45-64 / simple.py:45-62: u = torch.rand(B) from torch's global generator,
        device index search, row gather.  ``n_step`` > 1: the n-step host batch of the sampled slots
        (rle_replay_gather_nstep with ``discount``): reward holds the n-step return, next_state the last hop's, done
        ``discount^(hops-1)`` times the last hop's not-done mask, and ``hops`` the rows' hop counts; ``ind`` stays
        the sampled slots, which is what an ``n_step`` agent's ``train_ops`` recomputes the rows from."""
        import torch

        n_step = E.check_n_step(-1, n_step)
        self.flush()
        u = torch.rand(batch_size).numpy()
        ind = self.dev.sample_indices(u)
        hops = None
        if n_step > 1:
            s, a, r, s2, d, hops = self.dev.gather_nstep(ind, n_step, discount)
        else:
            s, a, r, s2, d = self.dev.gather(ind)
        data = dict(state=s, action=a, reward=r[:, None], next_state=s2, done=d[:, None])
        if use_torch:
            data = {k: torch.from_numpy(v) for k, v in data.items()}
        self.ind = ind
        batch = DeviceBatch(data, ind, self)
        if hops is not None:
            batch.hops = hops
        return batch

    # ---- save / restore / copy / move --------------------------------------
    # The reference's replays are NumPy arrays (lap.py:18-29, simple.py:15-27): pickle, deepcopy and a
    # checkpoint of them need no code.  Here the ring is in HBM behind a handle, so each is spelled out
    # on the device pack kernels (rle_replay_export / _import / _copy).
    def _meta(self) -> dict:
        ptr, size, maxp = self.dev.state()
        return S.make_meta(capacity=self.replay_buffer_size, state_dim=self.state_dim, action_dim=self.action_dim,
                           lap=self.LAP, ptr=ptr, size=size, max_priority=maxp, env_id=self.env_id,
                           action_bias=self.action_bias, action_scale=self.action_scale)

    def _check_meta(self, meta) -> dict:
        return S.validate_meta(meta, capacity=self.replay_buffer_size, state_dim=self.state_dim,
                               action_dim=self.action_dim, lap=self.LAP)

    def state_dict(self) -> dict:
        """Everything sampling and appending depend on, as host data: ``meta`` (capacity, dims, lap, ptr,
        size, max_priority, env_id, action map, format version), the arrays ``state``, ``action``,
        ``reward``, ``next_state``, ``notdone`` (and ``priority`` for LAP) as rows ``[0, size)`` in slot
        order, and the last indices ``ind``.  Staged appends are flushed first."""
        self.flush()
        meta = self._meta()
        rows = self.dev.export_rows(0, meta["size"], priority=self.LAP)
        sd = {"meta": meta}
        sd.update(zip(S.field_names(self.LAP), rows))
        ind = self.ind
        sd["ind"] = None if ind is None else np.array(ind, np.int64)
        return sd

    def load_state_dict(self, sd: dict) -> "BaseReplayMemory":
        """Restore a ``state_dict`` of a replay of the same capacity, dims and LAP-ness (ValueError
        otherwise).  Engines bound to this replay redraw their prefetched batch."""
        meta = self._check_meta(sd["meta"])
        arrays = {k: np.ascontiguousarray(sd[k], np.float32) for k in S.field_names(self.LAP) if k in sd}
        S.validate_arrays(meta, arrays)
        self._stage = []
        self.dev.import_rows(0, arrays["state"], arrays["action"], arrays["reward"], arrays["next_state"],
                             arrays["notdone"], arrays.get("priority"))
        self.dev.set_state(meta["ptr"], meta["size"], meta["max_priority"])
        self.ind = sd.get("ind")
        return self

    def _host_attrs(self) -> dict:
        return {k: v for k, v in self.__dict__.items() if k not in ("dev", "_stage", "_ind", "_ind_src")}

    def _fresh(self, attrs: dict, device: int) -> None:
        """An empty ring of this replay's settings on GPU ``device`` (no ``__init__``: the settings come
        from a state or a snapshot, not from an environment table)."""
        self.__dict__.update(attrs)
        self.device = int(device)
        self._stage, self._ind, self._ind_src = [], None, None
        self.dev = E.Replay(self.replay_buffer_size, self.state_dim, self.action_dim, self.LAP, self.device)

    def __getstate__(self) -> dict:
        """Pickle goes through ``state_dict``: the whole replay is held in host memory (3.1 GB for 1M
        Humanoid rows).  ``save`` / ``load`` stream it in chunks instead."""
        return {"attrs": self._host_attrs(), "state": self.state_dict()}

    def __setstate__(self, d: dict) -> None:
        self._fresh(d["attrs"], d["attrs"].get("device", 0))
        self.load_state_dict(d["state"])

    def __deepcopy__(self, memo) -> "BaseReplayMemory":
        """A new ring on the same GPU filled by one device-to-device copy (no host round trip)."""
        import copy

        self.flush()
        new = type(self).__new__(type(self))
        memo[id(self)] = new
        new._fresh(copy.deepcopy(self._host_attrs(), memo), self.device)
        new.dev.copy_from(self.dev)
        new.ind = self.ind
        return new

    def to(self, device) -> "BaseReplayMemory":
        """Move the ring to GPU k (``"cuda:k"``, ``"hip:k"`` or k, as ``EngineAgent.to``; "cpu" and the
        current device are no-ops).  An agent that trains from this replay moves on its own:
        ``agent.to(device)``."""
        k = _device_index(device)
        if k < 0 or k == self.device:
            return self
        self.flush()
        ind = self.ind  # (read from the engine that drew it before its replay goes away)
        new = E.Replay(self.replay_buffer_size, self.state_dim, self.action_dim, self.LAP, k)
        new.copy_from(self.dev)
        self.dev.close()
        self.dev, self.device = new, k
        self.ind = ind
        return self

    def save(self, path) -> None:
        """Write the replay as a snapshot directory (rl/replay_memory/snapshot.py): ``meta.json`` and one
        ``.npy`` per array, streamed ``REPLAY_IO_ROWS`` rows at a time, so host memory stays bounded by
        one chunk whatever the replay's size."""
        self.flush()
        meta = self._meta()
        names = S.field_names(self.LAP)
        with S.SnapshotWriter(path, meta, self.ind) as w:
            for first in range(0, meta["size"], E.REPLAY_IO_ROWS):
                c = min(E.REPLAY_IO_ROWS, meta["size"] - first)
                w.write(dict(zip(names, self.dev.export_rows(first, c, priority=self.LAP))))

    @classmethod
    def load(cls, path, device=0) -> "BaseReplayMemory":
        """Read a snapshot directory written by ``save`` into a new replay on GPU ``device``."""
        meta, ind, chunks = S.read_snapshot(path, E.REPLAY_IO_ROWS, lap=cls.LAP)
        new = cls.__new__(cls)
        new._fresh({"replay_buffer_size": meta["capacity"], "env_id": meta["env_id"],
                    "state_dim": meta["state_dim"], "action_dim": meta["action_dim"],
                    "action_bias": np.asarray(meta["action_bias"], np.float32),
                    "action_scale": np.asarray(meta["action_scale"], np.float32)}, max(_device_index(device), 0))
        for first, c in chunks:
            new.dev.import_rows(first, c["state"], c["action"], c["reward"], c["next_state"], c["notdone"],
                                c.get("priority"))
        new.dev.set_state(meta["ptr"], meta["size"], meta["max_priority"])
        new.ind = ind
        return new
