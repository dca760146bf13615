"""Shared machinery of the engine-backed TD7 / TD3 / SAC agents.

Each agent owns one ``rle_engine`` (include/rle.h): all networks, target copies,
Adam moments and step counters live in HBM and a gradient step is one replay of
a captured HIP graph.  The Python side keeps the reference's interface
(rl/agent/abc.py:16-55, rl/sampler.py:14-19): construction arguments,
``train_ops(batch, replay_buffer)`` returning the same info dict, ``sample``,
``to``, ``load_state_dict``, pickling (``save``/``load``/``deepcopy``).

There is no CPU path: constructing an agent without the HIP library raises.
"""

from __future__ import annotations

import copy
import math

import numpy as np

from rl import _engine as E
from rl.agent.abc import Agent
from rl.agent.state_blob import blob_to_dict, covers, dict_to_blob
from rl.nn.layout import AGENT_COPIES, AGENT_NETS, init_agent, layers
from rl.replay_memory.base import BaseReplayMemory, DeviceBatch, _device_index
from rl.sampler import Sampler
from rl.utils.envs import get_action_bias_scale, get_state_action_dims


class EngineAgent(Agent, Sampler):
    ALG = ""          # "td7" | "td3" | "sac"
    ALGO = -1         # RLE_TD7 / RLE_TD3 / RLE_SAC
    OPTIM_NETS: tuple = ()
    NULLABLE: tuple = ()  # info keys the reference sets to None on non-policy steps
    # (class defaults: agents pickled before these existed load without them)
    _ext: dict = {}   # rle_config_ext settings (make_config_ext), re-applied by every _new_engine
    obs_norm = None   # (mean, scale) fed to the act path by sample(), set_obs_norm
    # global gradient-norm threshold of every optimizer of a step (rle_set_grad_clip); inf: off
    clip_grad_norm: float = math.inf
    # parameter-free LayerNorm after every hidden Linear of the critics (rle_set_layer_norm; TD3 / SAC)
    critic_layer_norm: bool = False
    # dropout probability on every hidden Linear's output of the critics, ahead of the LayerNorm
    # (rle_set_critic_dropout; TD3 / SAC, needs critic_layer_norm); 0.0: off
    critic_dropout: float = 0.0
    # n of the n-step returns the device sampler gathers (rle_set_n_step; TD3 / SAC); 1: one-step targets
    n_step: int = 1

    def _setup(self, env_id, *, hidden, batch_size, seed, device, make_nn, make_nn_kwargs, cfg):
        custom = None
        shape = {}  # net shapes beyond the defaults: zs_dim (SALE), hidden_sizes (make_mlp)
        acts = {}  # hidden activations of the make_nn nets (make_config act_*)
        if make_nn is not None:  # td7.py:56-61 / td3.py:53-56 / sac.py:47-50 (rl.nn.modules nets only)
            from rl.nn.modules import nets_and_settings_from_make_nn

            S, A = get_state_action_dims(env_id)
            hidden, shape, custom, acts, ln, drop = nets_and_settings_from_make_nn(self.ALG, make_nn, S, A,
                                                                                    make_nn_kwargs)
            if self.critic_layer_norm and not ln:
                raise ValueError("critic_layer_norm=True, but make_nn's critics carry no LayerNorm "
                                 "(rl.nn.MLPCritic(..., layer_norm=True))")
            if ln:  # (the hook's nets decide; False stays the class default)
                self.critic_layer_norm = True
            if self.critic_dropout and drop != self.critic_dropout:
                raise ValueError(f"critic_dropout={self.critic_dropout}, but make_nn's critics carry dropout {drop} "
                                 "(rl.nn.MLPCritic(..., layer_norm=True, dropout=p))")
            if drop:  # (the hook's nets decide; 0.0 stays the class default)
                self.critic_dropout = float(drop)
            make_nn_kwargs = {}
        if self.critic_dropout and not self.critic_layer_norm:
            raise ValueError("critic_dropout needs critic_layer_norm=True: the dropout lives in the critics' "
                             "LayerNorm blocks (dropout without LayerNorm is not run)")
        hdim = make_nn_kwargs.pop("hdim", None)
        zs = make_nn_kwargs.pop("zs_dim", None)
        hs = make_nn_kwargs.pop("hidden_sizes", None)
        if make_nn_kwargs:
            raise TypeError(f"unsupported arguments {sorted(make_nn_kwargs)}")
        if self.ALG == "td7":
            if hs is not None:
                raise TypeError("hidden_sizes is a make_mlp argument (TD3 / SAC); TD7 takes hdim / zs_dim")
            if hdim is not None:
                hidden = hdim
            if zs is not None and int(zs) != int(hidden):
                shape["zs_dim"] = int(zs)
        else:
            if hdim is not None or zs is not None:
                raise TypeError("hdim / zs_dim are SALE arguments (TD7); TD3 / SAC take hidden_sizes")
            if hs is not None:
                from rl.nn.modules import _sizes

                hs = _sizes(hs)
                shape["hidden_sizes"] = [int(h) for h in hs]
                hidden = hs[-1]
        if shape.get("hidden_sizes") == [int(hidden)] * 2:
            shape = {}  # (the default shape)
        self.shape = shape
        self.acts = acts
        self.env_id = env_id
        self.state_dim, self.action_dim = get_state_action_dims(env_id)
        self.action_bias, self.action_scale = get_action_bias_scale(env_id)
        self.hidden = int(hidden)
        if seed is None:
            import torch

            seed = torch.initial_seed() & 0x7FFFFFFF
        self.seed = int(seed)
        self._cfg = dict(cfg)
        self._device = max(_device_index(device), 0)
        self.device = device if device is not None else "cuda:0"
        self._replay = None
        self.engine = self._new_engine(int(batch_size))
        if custom is not None:  # the hook's nets, and their construction-time copies (td7.py:62-66)
            nets = dict(custom)
            for name, src in AGENT_COPIES[self.ALG].items():
                nets[name] = {k: v.copy() for k, v in custom[src].items()}
        else:
            nets = init_agent(self.ALG, self.state_dim, self.action_dim, self.hidden, self.seed, **self.shape)
        self._import({"params": nets})

    # ---- engine lifecycle ----------------------------------------------------
    def _new_engine(self, batch):
        c = E.make_config(self.ALGO, self.state_dim, self.action_dim, self.hidden, batch, seed=self.seed,
                          device=self._device, **self._cfg, **self.shape, **getattr(self, "acts", {}))
        ext = getattr(self, "_ext", None)
        eng = E.Engine(c, ext=E.make_config_ext(**ext) if ext else None)
        clip = float(getattr(self, "clip_grad_norm", math.inf))
        if clip != math.inf:  # (an agent pickled before the attribute existed, or left at inf: the unclipped step)
            eng.set_grad_clip(clip)
        if getattr(self, "critic_layer_norm", False):  # (class default False: an older pickle loads without it)
            eng.set_layer_norm(True)
        drop = float(getattr(self, "critic_dropout", 0.0))
        if drop > 0.0:  # (class default 0.0: an older pickle loads without it)
            eng.set_critic_dropout(drop)
        n = int(getattr(self, "n_step", 1))
        if n > 1:  # (class default 1: an older pickle loads without it)
            eng.set_n_step(n)
        return eng

    def _set_n_step(self, n_step):
        """The constructors' keyword, checked as rle_set_n_step checks it (before the engine exists; 1 stays the
        class default: nothing new in the pickle)."""
        n = E.check_n_step(self.ALGO, n_step)
        if n > 1:
            self.n_step = n

    def _with_hops(self, keys):
        """The info row's keys with the n-step column after the agent's own (TD3 / SAC _info_keys)."""
        return keys + ("replay/hops",) if getattr(self, "n_step", 1) > 1 else keys

    def _set_dropout(self, critic_dropout):
        """The TD3 / SAC constructors' keyword, checked as rle_set_critic_dropout checks it (before the engine
        exists; 0.0 stays the class default: nothing new in the pickle)."""
        p = float(critic_dropout)
        if not 0.0 <= p < 1.0:
            raise ValueError("critic_dropout must be in [0, 1) (0: no dropout)")
        if p > 0.0:
            self.critic_dropout = p

    def _set_layer_norm(self, critic_layer_norm):
        """The TD3 / SAC constructors' keyword (False stays the class default: nothing new in the pickle)."""
        if critic_layer_norm:
            self.critic_layer_norm = True

    def _host_critic(self, name):
        """A host-side rl.nn.MLPCritic with critic `name`'s current parameters (TD3 / SAC): the module the
        reference keeps as agent.q1 / agent.q2, LayerNorm and dropout included, rebuilt from the device on each
        access (in train mode, as a new module is; .eval() gives what rle_eval computes)."""
        import torch

        from rl.nn.modules import MLPCritic

        fn = {"relu": "ReLU", "elu": "ELU", "identity": "Identity", "leaky_relu": "LeakyReLU", "silu": "SiLU",
              "gelu": "GELU"}[getattr(self, "acts", {}).get("act_critic", "relu")]
        sizes = self.shape.get("hidden_sizes", [self.hidden] * 2)
        m = MLPCritic(self.state_dim, self.action_dim, sizes, action_fn=fn, layer_norm=self.critic_layer_norm,
                      dropout=getattr(self, "critic_dropout", 0.0))
        sd = {k: torch.from_numpy(np.array(v, np.float32)) for k, v in self.state_dict()[name].items()}
        m.load_state_dict(sd)
        return m

    def _set_clip(self, clip_grad_norm):
        """The constructors' keyword, checked as rle_set_grad_clip checks it (before the engine exists)."""
        c = float(clip_grad_norm)
        if not c >= 0.0:
            raise ValueError("clip_grad_norm must be >= 0 (0 or inf: no clipping)")
        if c != math.inf:  # (inf stays the class default: nothing new in the instance dict or its pickle)
            self.clip_grad_norm = c

    def grad_clip_stats(self) -> dict:
        """{optimizer: (total gradient norm, clip coefficient)} of the last update of each of this agent's
        optimizers ("critics", "policy", TD7's "encoder"); NaN before an optimizer's first step, or unclipped."""
        st = self.engine.grad_clip_stats()
        return {k: v for k, v in st.items() if k != "encoder" or self.ALG == "td7"}

    def set_obs_norm(self, mean, scale=None):
        """``sample()`` feeds ``(obs - mean) / scale`` to the act path (fp32, on the host): the observation
        side of a replay's ``normalize_states()``, whose return value this takes.  ``None`` clears it.
        Pickled with the agent; nothing on the device act path changes."""
        if mean is None:
            self.obs_norm = None
            return
        m = np.ascontiguousarray(mean, np.float32).reshape(self.state_dim)
        s = np.ascontiguousarray(scale, np.float32).reshape(self.state_dim)
        if not (np.isfinite(m).all() and np.isfinite(s).all() and (s != 0).all()):
            raise ValueError("set_obs_norm: mean must be finite, scale finite and non-zero")
        self.obs_norm = (m.copy(), s.copy())

    @property
    def batch_size(self) -> int:
        return self.engine.cfg.batch

    def _rebuild(self, batch=None, device=None):
        """A fresh engine with this one's whole state.  On the same GPU the state goes device to
        device (rle_copy_state); to another GPU through one exported blob."""
        batch = self.batch_size if batch is None else batch
        old = self.engine
        if device is None or device == self._device:
            self.engine = self._new_engine(batch)
            self.engine.copy_state_from(old)
            old.close()
        else:
            st = self._export()
            self._device = device
            old.close()
            self.engine = self._new_engine(batch)
            self._import(st)
        self._replay = None

    def _prepare(self, replay: BaseReplayMemory, batch: int):
        if not isinstance(replay, BaseReplayMemory):
            raise TypeError("engine agents train from rl.replay_memory device replays")
        if self._cfg.get("use_lap") and not replay.LAP:
            raise AssertionError("use_lap=True needs a LAPReplayMemory (td7.py:307-309)")
        if replay.device != self._device:
            raise ValueError(f"replay on device {replay.device}, agent on {self._device}")
        # (graphs capture the bound ring: another replay, or the same one after replay.to() gave it a new
        # ring, means a fresh engine)
        moved = self._replay is replay and self.engine.replay is not replay.dev
        if batch != self.batch_size or (self._replay is not None and self._replay is not replay) or moved:
            self._rebuild(batch)
        if self._replay is not replay:
            self.engine.bind(replay.dev)
            self._replay = replay
        replay.flush()

    # ---- parameters / state ---------------------------------------------------
    def _param_names(self):
        out = []
        for net, kind in AGENT_NETS[self.ALG].items():
            o = 2 * self.action_dim if (self.ALG == "sac" and net == "policy") else None
            names = []
            for prefix, fin, fout in layers(kind, self.state_dim, self.action_dim, self.hidden, o, **self.shape):
                names += [(prefix + ".weight", (fout, fin)), (prefix + ".bias", (fout,))]
            out.append((net, names))
            for copy, src in AGENT_COPIES[self.ALG].items():
                if src == net:
                    out.append((copy, names))
        return out

    def _export(self, what=E.STATE_ALL, reuse=False):
        """The engine's state as the nested dict the agents pickle.  Every parameter and Adam moment
        comes from ONE exported blob (rle_state_export: one pack launch, one copy), cut by its table
        of contents; the arrays are views of that blob.  ``what`` = STATE_PARAMS: the networks only.
        ``reuse``: the blob is the engine's reusable host array, valid until the next such export (for a
        pickler, which serialises the arrays at once: no 24 MB array is allocated and freed per save)."""
        e = self.engine
        names = self._param_names()
        shapes = {(net, n): shp for net, ns in names for n, shp in ns}
        blob = e.state_export(what, e.state_buffer(what) if reuse else None)
        cut = blob_to_dict(e.state_toc(what), blob, shapes)
        params = {net: {n: cut["params"][net][n] for n, _ in ns} for net, ns in names}
        if self.ALG == "sac":
            params["tmp"] = cut["params"]["tmp"]
        if what == E.STATE_PARAMS:
            return {"params": params}
        adam = {net: {n: cut["adam"][net][n] for n, _ in ns} for net, ns in names if net in self.OPTIM_NETS}
        if self.ALG == "sac":
            adam["tmp"] = cut["adam"]["tmp"]
        return {"params": params, "adam": adam, "counters": e.counters(), "vbounds": e.value_bounds(),
                "act_counter": e.act_counter()}

    def _import(self, st):
        """The reverse.  A dict with every network (and every moment, when it has "adam") goes in as
        one blob (rle_state_import); a partial one (load_params of some nets) tensor by tensor."""
        e = self.engine
        what = E.STATE_ALL if "adam" in st else E.STATE_PARAMS
        toc = e.state_toc(what)
        if covers(toc, st):
            with E.state_scratch(e.state_size(what)) as buf:
                e.state_import(dict_to_blob(toc, st, buf), what)
        else:
            for net, d in st["params"].items():
                for n, v in d.items():
                    e.set_param(net, n, np.asarray(v, np.float32))
            for net, d in st.get("adam", {}).items():
                for n, (m, v) in d.items():
                    e.set_adam(net, n, 0, m)
                    e.set_adam(net, n, 1, v)
        if "counters" in st:
            e.set_counters(st["counters"])
        if "vbounds" in st:
            e.set_value_bounds(st["vbounds"])
        if "act_counter" in st:
            e.set_act_counter(st["act_counter"])

    def state_dict(self):
        """{net: {param name: ndarray}} in the reference's state_dict naming."""
        return self._export(E.STATE_PARAMS)["params"]

    def load_params(self, params):
        self._import({"params": params})

    def __getstate__(self):
        d = {k: v for k, v in self.__dict__.items() if k not in ("engine", "_replay")}
        # (the arrays are views of the engine's reusable export array: serialise them before the next
        # __getstate__ of this agent, as pickle does)
        d["_engine_state"] = self._export(reuse=True)
        d["_batch"] = self.batch_size
        return d

    def __setstate__(self, d):
        st = d.pop("_engine_state")
        batch = d.pop("_batch")
        self.__dict__.update(d)
        self._replay = None
        self.engine = self._new_engine(batch)
        self._import(st)

    def __deepcopy__(self, memo):
        """copy.deepcopy(agent) (run_w_checkpoint.py:72): the host attributes, and a new engine whose
        state comes device to device (rle_copy_state) -- what pickle.loads(pickle.dumps(agent)) gives,
        without the host trip.  Like a pickle, the copy is bound to no replay."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in ("engine", "_replay", "_host_ring"):  # (the ring of host batches is rebuilt on demand)
                new.__dict__[k] = copy.deepcopy(v, memo)
        new._replay = None
        new.engine = new._new_engine(self.batch_size)
        new.engine.copy_state_from(self.engine)
        return new

    def to(self, device):
        """td7.py:101-112: move to a device.  'cpu' is accepted as a no-op (pickling exports
        the HBM state; there is no CPU execution path); cuda:k moves the engine to GPU k."""
        k = _device_index(device)
        if k >= 0 and k != self._device:
            self._rebuild(device=k)
        self.device = device
        return self

    def load_state_dict(self, agent: "EngineAgent"):
        """td7.py:114-125 / td3.py:94-100 / sac.py:101-107: copy every network (not the
        optimiser state, counters or SAC temperature)."""
        if type(agent) is not type(self):
            raise TypeError("load_state_dict needs an agent of the same class")
        self.engine.copy_nets_from(agent.engine)  # (rle_copy_nets: device to device, a peer copy across GPUs)
        return self

    @property
    def n_runs(self) -> int:
        return int(self.engine.counters()[3])

    # ---- training ----------------------------------------------------------
    def _info(self, row):
        out = {}
        for k, v in zip(self._info_keys(), row):
            v = float(v)
            out[k] = None if (k in self.NULLABLE and math.isnan(v)) else v
        return out

    def train_ops(self, batch, replay_buffer=None, *args, **kwargs):
        """One gradient step on ``batch`` (td7.py:287-332 / td3.py:206-242 / sac.py:251-295).

        ``batch`` must come from ``replay_buffer.sample(B)`` of a device replay: the step
        reads rows ``batch.ind`` in HBM (the host tensors in the dict are not re-uploaded).
        Target-policy / rsample noise comes from the engine's Philox stream."""
        if not isinstance(batch, DeviceBatch):
            return self._train_host_batch(batch, replay_buffer)
        rep = replay_buffer if replay_buffer is not None else batch.replay
        if batch.replay is not rep:
            raise ValueError("batch was drawn from a different replay than replay_buffer")
        ind = np.ascontiguousarray(batch.ind, np.int64).reshape(1, -1)
        self._prepare(rep, ind.shape[1])
        self.engine.set_tapes(ind=ind)
        try:
            row = self.engine.step(1)[0]
        finally:
            self.engine.set_tapes()
        return self._info(row)

    def _train_host_batch(self, batch, replay_buffer):
        """train_ops on any BATCH dict (annotation.py:23-30: state, action, reward, next_state,
        done as arrays or tensors; action in the replay's stored form, done the not-done mask):
        the rows go into a B-row device ring bound to the engine, the step runs on rows 0..B-1,
        and a LAP replay_buffer gets the new priorities through its own update_priority (and its
        reset_max_priority at TD7 hard updates), as td7.py:236-240, 325-331 would call them."""

        if getattr(self, "n_step", 1) > 1:
            raise ValueError("train_ops on a host BATCH dict with n_step > 1: its B-row scratch ring has no episode "
                             "order (train from a device replay's sample(), or train_n)")
        missing = [k for k in ("state", "action", "reward", "next_state", "done") if k not in batch]
        if missing:
            raise ValueError(f"BATCH (annotation.py:23-30) without {missing}")

        def arr(k, shape):
            v = batch[k]
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            return np.ascontiguousarray(np.asarray(v, np.float32).reshape(shape))

        B = int(np.asarray(batch["reward"].shape[0] if hasattr(batch["reward"], "shape") else len(batch["reward"])))
        s, a = arr("state", (B, self.state_dim)), arr("action", (B, self.action_dim))
        r, s2, d = arr("reward", (B,)), arr("next_state", (B, self.state_dim)), arr("done", (B,))
        lap = bool(self._cfg.get("use_lap")) and self.ALG != "sac"
        # td7.py:310 / td3.py:221 assert a LAP replay before update_priority (here before the step,
        # which runs as one device program: the reference would have stepped the encoder first)
        assert not lap or (replay_buffer is not None and getattr(replay_buffer, "LAP", hasattr(replay_buffer, "update_priority"))), \
            "a LAP agent's train_ops needs the LAPReplayMemory its priorities go to (td7.py:310)"
        ring = getattr(self, "_host_ring", None)
        if ring is None or ring.capacity != B or getattr(ring, "device", None) != self._device:
            ring = self._host_ring = E.Replay(B, self.state_dim, self.action_dim, lap, self._device)
            ring.device = self._device
        ring.append(s, a, r, s2, d)  # (capacity B: the write pointer returns to row 0)
        # (graphs capture the bound replay: another replay or batch size means a fresh engine)
        if B != self.batch_size or (self._replay is not None and self._replay is not ring):
            self._rebuild(B)
        if self._replay is not ring:
            self.engine.bind(ring)
            self._replay = ring
        hard_before = self.engine.counters()[3]
        self.engine.set_tapes(ind=np.arange(B, dtype=np.int64)[None])
        try:
            row = self.engine.step(1)[0]
        finally:
            self.engine.set_tapes()
        if lap:
            import torch

            replay_buffer.update_priority(torch.from_numpy(ring.get_priority(B).copy()))
            tur = int(self._cfg.get("target_update_rate", 250))
            if self.ALG == "td7" and (hard_before + 1) % tur == 0 and hasattr(replay_buffer, "reset_max_priority"):
                replay_buffer.reset_max_priority()
        return self._info(row)

    def train_n(self, replay_buffer: BaseReplayMemory, batch_size: int, n_ops: int):
        """n_ops x (sample + train_ops) fused on the device (run_train_ops, run.py:87-96)."""
        self._prepare(replay_buffer, batch_size)
        rows = self.engine.step(n_ops) if n_ops > 0 else []
        if n_ops > 0:
            replay_buffer._mark_engine_indices(self.engine)
        return [self._info(r) for r in rows]

    # ---- acting --------------------------------------------------------------
    def _act(self, state, deterministic, eps=None):
        """Agent.sample as one device program (rle_act_sample): forward, exploration noise
        (the engine's Philox stream, or the tape `eps` [A]), clip and the action map, written
        into pinned memory by the last kernel.  Returns the first row as the reference does."""
        eng = self.engine
        # the reference reads action_scale / action_bias / exploration_noise on every call
        # (td7.py:151-155): re-send the map whenever any of them changed
        amap = (np.asarray(self.action_scale, np.float32).tobytes(), np.asarray(self.action_bias, np.float32).tobytes(),
                float(getattr(self, "exploration_noise", 0.1)))
        if getattr(eng, "_act_map", None) != amap:
            eng.set_action_map(self.action_scale, self.action_bias, amap[2])
            eng._act_map = amap
        if hasattr(state, "detach"):
            state = state.detach().cpu().numpy()
        if self.obs_norm is not None:
            state = (np.asarray(state, np.float32) - self.obs_norm[0]) / self.obs_norm[1]
        if eps is not None:
            return eng.act_sample(state, 2, eps)[0].copy()
        return eng.act_sample(state, 0 if deterministic else 1)[0].copy()

    def _forward(self, state, width):
        if hasattr(state, "detach"):
            state = state.detach().cpu().numpy()
        x = np.asarray(state, np.float32)
        if x.ndim == 1:
            x = x[None]
        return self.engine.act(x, width)
