"""ctypes binding of ``librle.so`` (C ABI in ``include/rle.h``).

This is the only bridge between the Python mirror of the reference interface
and the HIP engine.  There is no CPU fallback: if the library is missing or
fails to load, every engine-backed object raises.
"""

from __future__ import annotations

import contextlib
import ctypes
import os
import threading

import numpy as np

RLE_TD7, RLE_TD3, RLE_SAC = 0, 1, 2
RLE_EVAL_Q, RLE_EVAL_ZS, RLE_EVAL_ZSA = 0, 1, 2
INFO_MAX = 8
MAX_N_STEP = 8  # RLE_MAX_N_STEP
REPLAY_IO_ROWS = 8192  # rle_replay_io_rows(): rows per staging chunk of replay export / import

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RLE_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "librle.so")  # RLE_LIB: experiment builds

_lib = None

_f32p = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_longlong)
_vp = ctypes.c_void_p
_cs = ctypes.c_char_p
_int = ctypes.c_int
_ll = ctypes.c_longlong


class Config(ctypes.Structure):
    """Mirror of ``rle_config`` (include/rle.h)."""

    _fields_ = [
        ("algo", _int), ("state_dim", _int), ("action_dim", _int), ("hidden", _int),
        ("batch", _int), ("use_lap", _int), ("discount", ctypes.c_float),
        ("policy_lr", ctypes.c_float), ("critic_lr", ctypes.c_float), ("tau", ctypes.c_float),
        ("target_policy_noise", ctypes.c_float), ("noise_clip", ctypes.c_float),
        ("policy_freq", _int), ("target_update_rate", _int), ("min_log_std", ctypes.c_float),
        ("max_log_std", ctypes.c_float), ("tmp", ctypes.c_float), ("seed", ctypes.c_ulonglong),
        ("device", _int), ("zs_dim", _int), ("n_hidden", _int), ("hidden_sizes", _int * 8),
        ("act_actor", _int), ("act_critic", _int), ("act_encoder", _int),
        ("bc_lambda", ctypes.c_float),
    ]


class ConfigExt(ctypes.Structure):
    """Mirror of ``rle_config_ext`` (include/rle.h): settings added after ``rle_config`` was frozen.
    ``size`` is what this mirror knows of the struct; the library reads every field past it as 0."""

    _fields_ = [("size", _int), ("bc_alpha", ctypes.c_float), ("awac_lambda", ctypes.c_float)]


def make_config_ext(bc_alpha=0.0, awac_lambda=0.0) -> ConfigExt:
    """``bc_alpha`` (TD3): 0 online; > 0 the offline (TD3+BC) policy step's alpha (rle_config_ext bc_alpha).
    ``awac_lambda`` (SAC at a fixed temperature of 0): 0 online; > 0 the offline (AWAC) policy step's lambda
    (rle_config_ext awac_lambda)."""
    return ConfigExt(ctypes.sizeof(ConfigExt), float(bc_alpha), float(awac_lambda))


# rle_config act_* codes (include/rle.h RLE_ACT_*): 0 = the reference default of that net
ACT_CODES = {"default": 0, "relu": 1, "elu": 2, "identity": 3, "leaky_relu": 4, "silu": 5, "gelu": 6}


class Plan(ctypes.Structure):
    """Mirror of ``rle_plan`` (include/rle.h): the schedule / tile-plan / fusion choices that
    decide the step's fp32 summation order.  No environment variable changes it."""

    _fields_ = [
        ("level_cap", _int), ("steps_per_graph", _int), ("pre_tn", _int), ("pl_tn", _int), ("tn_min", _int),
        ("flat_div", _int), ("balance", _int), ("tiny_w", _int), ("uni_w", _int), ("tiny_wg", _int),
        ("sched_cap", _int), ("fuse_off", ctypes.c_uint), ("fuse_on", ctypes.c_uint), ("rb", _int),
        ("pl_w", _int), ("lap_w", _int), ("head_w", _int), ("adam_w", _int), ("wide", _int), ("lpt", _int),
        ("dispatch", _int), ("dpf", _int), ("xcd", _int),
    ]


# RLE_FUSE_* bits of rle_plan.fuse_off
FUSE = {"prelayer": 1 << 0, "pre": 1 << 1, "qdot": 1 << 2, "headdx": 1 << 3, "nbdefer": 1 << 4, "sacfwd": 1 << 5,
        "sacbwd": 1 << 6, "fold": 1 << 7, "pipolyak": 1 << 8, "endsplit": 1 << 9, "priosample": 1 << 10,
        "twostage": 1 << 11, "sacpre": 1 << 12, "normfin": 1 << 13, "nbrows": 1 << 14}


def make_plan(fuse_off=(), fuse_on=(), **kw) -> Plan:
    """rle_plan_default() with the given fields changed; fuse_off / fuse_on: names of FUSE to switch off
    / on (fuse_on: the opt-in fusions, FUSE_OPT_IN)."""
    p = Plan()
    _check(lib().rle_plan_default(ctypes.byref(p)))
    for k, v in kw.items():
        if k not in dict(Plan._fields_):
            raise ValueError(f"unknown plan field {k!r}")
        setattr(p, k, int(v))
    def bits(names):
        b = 0
        for name in ([names] if isinstance(names, str) else names):
            b |= FUSE[name]
        return b

    p.fuse_off, p.fuse_on = bits(fuse_off), bits(fuse_on)
    return p


def parse_plan(text: str) -> Plan:
    """'level_cap=512,steps_per_graph=4,fuse_off=headdx+qdot' -> Plan (bench.py --plan, tools)."""
    kw, off, on = {}, (), ()
    for item in filter(None, (t.strip() for t in (text or "").split(","))):
        k, _, v = item.partition("=")
        if k == "fuse_off":
            off = tuple(filter(None, v.split("+")))
        elif k == "fuse_on":
            on = tuple(filter(None, v.split("+")))
        else:
            kw[k] = int(v)
    return make_plan(off, on, **kw)


def plan_dict(p: Plan) -> dict:
    d = {k: getattr(p, k) for k, _ in Plan._fields_}
    d["fuse_off"] = [n for n, b in FUSE.items() if p.fuse_off & b]
    d["fuse_on"] = [n for n, b in FUSE.items() if p.fuse_on & b]
    return d


STATE_PARAMS, STATE_ADAM_M, STATE_ADAM_V, STATE_ALL = 1, 2, 4, 7  # RLE_STATE_* masks of rle_state_*

_scratch = np.empty(0, np.float32)
_scratch_lock = threading.Lock()


@contextlib.contextmanager
def state_scratch(n):
    """A process-wide fp32 host array of n elements for assembling a packed state that is imported at
    once (unpickling makes a new engine per agent: an array per engine would be allocated and freed, tens
    of MB, on every load).  Grown on demand, never shrunk; held under a lock while in use."""
    global _scratch
    with _scratch_lock:
        if _scratch.size < n:
            _scratch = np.empty(n, np.float32)
        yield _scratch[:n]


class StateEntry(ctypes.Structure):
    """Mirror of ``rle_state_entry`` (include/rle.h): one tensor of a packed agent state."""

    _fields_ = [("net", ctypes.c_char * 32), ("name", ctypes.c_char * 32), ("arena", _int), ("reserved", _int),
                ("offset", _ll), ("numel", _ll)]


# name -> (restype, argtypes)
SIGNATURES = {
    "rle_last_error": (_cs, []),
    "rle_replay_create": (_int, [_int, _ll, _int, _int, _int, ctypes.POINTER(_vp)]),
    "rle_replay_destroy": (_int, [_vp]),
    "rle_replay_append": (_int, [_vp, _f32p, _f32p, _f32p, _f32p, _f32p, _ll]),
    "rle_replay_state": (_int, [_vp, _i64p, _i64p, _f32p]),
    "rle_replay_fill_random": (_int, [_vp, _ll, ctypes.c_ulonglong]),
    "rle_replay_get_priority": (_int, [_vp, _f32p, _ll]),
    "rle_replay_set_priority": (_int, [_vp, _f32p, _ll, ctypes.c_float]),
    "rle_replay_sample_indices": (_int, [_vp, _int, _f32p, _i64p]),
    "rle_replay_update_priority": (_int, [_vp, _int, _i64p, _f32p]),
    "rle_replay_reset_max_priority": (_int, [_vp]),
    "rle_replay_gather": (_int, [_vp, _int, _i64p, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "rle_replay_gather_nstep": (_int, [_vp, _int, _i64p, _int, ctypes.c_float, _f32p, _f32p, _f32p, _f32p, _f32p,
                                       ctypes.POINTER(ctypes.c_int)]),
    "rle_replay_io_rows": (_int, []),
    "rle_replay_export": (_int, [_vp, _ll, _ll, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "rle_replay_import": (_int, [_vp, _ll, _ll, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "rle_replay_set_state": (_int, [_vp, _ll, _ll, ctypes.c_float]),
    "rle_replay_copy": (_int, [_vp, _vp]),
    "rle_replay_state_stats": (_int, [_vp, _f32p, _f32p]),
    "rle_replay_normalize_states": (_int, [_vp, _f32p, _f32p]),
    "rle_create": (_int, [ctypes.POINTER(Config), ctypes.POINTER(_vp)]),
    "rle_create_ext": (_int, [ctypes.POINTER(Config), ctypes.POINTER(ConfigExt), ctypes.POINTER(_vp)]),
    "rle_destroy": (_int, [_vp]),
    "rle_plan_default": (_int, [ctypes.POINTER(Plan)]),
    "rle_set_plan": (_int, [_vp, ctypes.POINTER(Plan)]),
    "rle_get_plan": (_int, [_vp, ctypes.POINTER(Plan)]),
    "rle_set_grad_clip": (_int, [_vp, ctypes.c_float]),
    "rle_get_grad_clip": (_int, [_vp, _f32p]),
    "rle_grad_clip_stats": (_int, [_vp, _f32p]),
    "rle_set_layer_norm": (_int, [_vp, _int]),
    "rle_get_layer_norm": (_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "rle_set_critic_dropout": (_int, [_vp, ctypes.c_float]),
    "rle_get_critic_dropout": (_int, [_vp, _f32p]),
    "rle_dropout_mask": (_int, [_vp, _ll, _int, _int, _int, _f32p]),
    "rle_set_n_step": (_int, [_vp, _int]),
    "rle_get_n_step": (_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "rle_bind_replay": (_int, [_vp, _vp]),
    "rle_param_numel": (_int, [_vp, _cs, _cs, _i64p]),
    "rle_get_param": (_int, [_vp, _cs, _cs, _f32p, _ll]),
    "rle_set_param": (_int, [_vp, _cs, _cs, _f32p, _ll]),
    "rle_get_adam": (_int, [_vp, _cs, _cs, _int, _f32p, _ll]),
    "rle_set_adam": (_int, [_vp, _cs, _cs, _int, _f32p, _ll]),
    "rle_state_toc": (_int, [_vp, _int, ctypes.POINTER(StateEntry), _int, ctypes.POINTER(_int)]),
    "rle_state_export": (_int, [_vp, _int, _f32p, _ll]),
    "rle_state_import": (_int, [_vp, _int, _f32p, _ll]),
    "rle_copy_nets": (_int, [_vp, _vp]),
    "rle_get_counters": (_int, [_vp, _i64p]),
    "rle_set_counters": (_int, [_vp, _i64p]),
    "rle_get_act_counter": (_int, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "rle_set_act_counter": (_int, [_vp, ctypes.c_uint64]),
    "rle_get_value_bounds": (_int, [_vp, _f32p]),
    "rle_set_value_bounds": (_int, [_vp, _f32p]),
    "rle_step": (_int, [_vp, _int, _f32p]),
    "rle_step_timed": (_int, [_vp, _int, _f32p]),
    "rle_step_async": (_int, [_vp, _int]),
    "rle_set_tapes": (_int, [_vp, _int, _f32p, _f32p, _f32p, _i64p]),
    "rle_last_indices": (_int, [_vp, _i64p]),
    "rle_act": (_int, [_vp, _f32p, _int, _f32p]),
    # (raw addresses: the per-env-step path skips ctypes pointer conversions)
    "rle_act_sample": (_int, [_vp, _vp, _int, _int, _vp, _vp]),
    "rle_set_action_map": (_int, [_vp, _f32p, _f32p, ctypes.c_float]),
    "rle_launch_count": (_int, [_vp, ctypes.POINTER(ctypes.c_longlong)]),
    "rle_graph_stats": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "rle_graph_describe": (_int, [_vp, _int, ctypes.c_char_p, _int]),
    "rle_graph_trace": (_int, [_vp, _int, ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]),
    "rle_trace_stride": (_int, []),
    "rle_aql_wait_plan": (_int, [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
    "rle_aql_selftest": (_int, []),
    "rle_level_plan": (_int, [ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), _int, _int,
                              ctypes.c_ulonglong, ctypes.c_ulonglong, _int, _int, ctypes.POINTER(ctypes.c_uint), _int,
                              ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "rle_schedule_plan": (_int, [ctypes.POINTER(_int)] * 4 + [_int] + [ctypes.POINTER(_int)] * 4 + [_int, _vp, _int]
                          + [ctypes.POINTER(_int)] * 3),
    "rle_hazard_scan": (_int, [ctypes.POINTER(ctypes.c_ulonglong)] * 2 + [ctypes.POINTER(_int)] * 2 + [_int,
                        ctypes.POINTER(_int), _int, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "rle_eval": (_int, [_vp, _int, _cs, _cs, _f32p, _f32p, _int, _f32p]),
    "rle_sac_rsample": (_int, [_vp, _f32p, _f32p, _f32p, _int, _f32p, _f32p]),
    "rle_get_info": (_int, [_vp, _int, _f32p]),
    "rle_copy_state": (_int, [_vp, _vp]),
    "rle_synchronize": (_int, [_vp]),
}


def lib():
    """Load librle.so (fails loudly: no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"HIP engine library not built: {LIB_PATH} (run __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        msg = lib().rle_last_error().decode(errors="replace")
        raise RuntimeError(f"rle error {rc}: {msg}")


def _fp(a):
    return None if a is None else a.ctypes.data_as(_f32p)


def _ip(a):
    return None if a is None else a.ctypes.data_as(_i64p)


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if shape is None else a.reshape(shape)


class Replay:
    """Device replay ring (HBM) with optional LAP priorities."""

    def __init__(self, capacity, state_dim, action_dim, lap, device=0):
        self.h = _vp()
        self.S, self.A, self.capacity, self.lap = state_dim, action_dim, capacity, bool(lap)
        _check(lib().rle_replay_create(device, capacity, state_dim, action_dim, int(lap), ctypes.byref(self.h)))

    def close(self):
        if self.h:
            _check(lib().rle_replay_destroy(self.h))
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, state, action, reward, next_state, notdone):
        n = len(reward)
        s = _f32(state, (n, self.S))
        a = _f32(action, (n, self.A))
        r = _f32(reward, (n,))
        s2 = _f32(next_state, (n, self.S))
        d = _f32(notdone, (n,))
        _check(lib().rle_replay_append(self.h, _fp(s), _fp(a), _fp(r), _fp(s2), _fp(d), n))

    def state(self):
        p, s, m = _ll(), _ll(), ctypes.c_float()
        _check(lib().rle_replay_state(self.h, ctypes.byref(p), ctypes.byref(s), ctypes.byref(m)))
        return p.value, s.value, m.value

    def fill_random(self, count, seed):
        _check(lib().rle_replay_fill_random(self.h, count, seed))

    def get_priority(self, n=None):
        n = self.capacity if n is None else n
        out = np.empty(n, np.float32)
        _check(lib().rle_replay_get_priority(self.h, _fp(out), n))
        return out

    def set_priority(self, p, max_priority):
        p = _f32(p)
        _check(lib().rle_replay_set_priority(self.h, _fp(p), p.size, float(max_priority)))

    def sample_indices(self, u):
        u = _f32(u)
        out = np.empty(u.size, np.int64)
        _check(lib().rle_replay_sample_indices(self.h, u.size, _fp(u), _ip(out)))
        return out

    def update_priority(self, ind, p):
        ind = np.ascontiguousarray(ind, np.int64)
        p = _f32(p)
        _check(lib().rle_replay_update_priority(self.h, ind.size, _ip(ind), _fp(p)))

    def reset_max_priority(self):
        _check(lib().rle_replay_reset_max_priority(self.h))

    def gather(self, ind):
        ind = np.ascontiguousarray(ind, np.int64)
        n = ind.size
        s = np.empty((n, self.S), np.float32)
        a = np.empty((n, self.A), np.float32)
        r = np.empty(n, np.float32)
        s2 = np.empty((n, self.S), np.float32)
        d = np.empty(n, np.float32)
        _check(lib().rle_replay_gather(self.h, n, _ip(ind), _fp(s), _fp(a), _fp(r), _fp(s2), _fp(d)))
        return s, a, r, s2, d

    def gather_nstep(self, ind, n_step, discount):
        """The n-step batch of rle.h's law for slots `ind` (each < size), computed by the step's own sampler
        (rle_replay_gather_nstep): (state, action, R, next_state of the last hop, gamma^(hops-1) * notdone of the
        last hop, hops).  n_step = 1 is gather() and hops 1."""
        ind = np.ascontiguousarray(ind, np.int64)
        n = ind.size
        s = np.empty((n, self.S), np.float32)
        a = np.empty((n, self.A), np.float32)
        r = np.empty(n, np.float32)
        s2 = np.empty((n, self.S), np.float32)
        d = np.empty(n, np.float32)
        hops = np.empty(n, np.int32)
        _check(lib().rle_replay_gather_nstep(self.h, n, _ip(ind), int(n_step), ctypes.c_float(discount), _fp(s),
                                             _fp(a), _fp(r), _fp(s2), _fp(d),
                                             hops.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return s, a, r, s2, d, hops

    def export_rows(self, first, count, priority=False):
        """Slots first .. first+count-1 as unpadded fp32 arrays (rle_replay_export):
        (state, action, reward, next_state, notdone), plus priority when asked (LAP replays)."""
        first, n = int(first), int(count)
        s = np.empty((n, self.S), np.float32)
        a = np.empty((n, self.A), np.float32)
        r = np.empty(n, np.float32)
        s2 = np.empty((n, self.S), np.float32)
        d = np.empty(n, np.float32)
        p = np.empty(n, np.float32) if priority else None
        _check(lib().rle_replay_export(self.h, first, n, _fp(s), _fp(a), _fp(r), _fp(s2), _fp(d), _fp(p)))
        return (s, a, r, s2, d, p) if priority else (s, a, r, s2, d)

    def import_rows(self, first, state, action, reward, next_state, notdone, priority=None):
        """Host rows -> slots first .. (rle_replay_import); ptr, size and the LAP sums follow in set_state."""
        n = len(reward)
        s = _f32(state, (n, self.S))
        a = _f32(action, (n, self.A))
        r = _f32(reward, (n,))
        s2 = _f32(next_state, (n, self.S))
        d = _f32(notdone, (n,))
        p = None if priority is None else _f32(priority, (n,))
        _check(lib().rle_replay_import(self.h, int(first), n, _fp(s), _fp(a), _fp(r), _fp(s2), _fp(d), _fp(p)))

    def set_state(self, ptr, size, max_priority):
        _check(lib().rle_replay_set_state(self.h, int(ptr), int(size), float(max_priority)))

    def state_stats(self):
        """Per-feature (mean, population std) of ``state`` over the filled rows (rle_replay_state_stats: fp64
        accumulation on the device, results in fp32)."""
        m, s = np.empty(self.S, np.float32), np.empty(self.S, np.float32)
        _check(lib().rle_replay_state_stats(self.h, _fp(m), _fp(s)))
        return m, s

    def normalize_states(self, shift, scale):
        """state, next_state of the filled rows <- (x - shift) / scale on the device
        (rle_replay_normalize_states)."""
        shift, scale = _f32(shift, (self.S,)), _f32(scale, (self.S,))
        _check(lib().rle_replay_normalize_states(self.h, _fp(shift), _fp(scale)))

    def copy_from(self, other: "Replay"):
        """This ring := other (rle_replay_copy: device to device, also across two GPUs)."""
        _check(lib().rle_replay_copy(self.h, other.h))


class Engine:
    """One agent's device state + captured step graphs."""

    def __init__(self, cfg: Config, plan: Plan | None = None, ext: ConfigExt | None = None):
        self.cfg = cfg
        self.ext = ext
        self.h = _vp()
        if ext is None:
            _check(lib().rle_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        else:
            _check(lib().rle_create_ext(ctypes.byref(cfg), ctypes.byref(ext), ctypes.byref(self.h)))
        self.replay = None
        self._act_out = {}
        if plan is not None:
            self.set_plan(plan)

    def set_plan(self, plan: Plan):
        """Before the first step (the step programs are built with it)."""
        _check(lib().rle_set_plan(self.h, ctypes.byref(plan)))

    def plan(self) -> dict:
        """The plan in effect (defaults resolved)."""
        p = Plan()
        _check(lib().rle_get_plan(self.h, ctypes.byref(p)))
        return plan_dict(p)

    def set_grad_clip(self, max_norm: float):
        """Clip every optimizer of the step to this global L2 norm (0 or inf: off).  Before the first step."""
        _check(lib().rle_set_grad_clip(self.h, ctypes.c_float(max_norm)))

    def grad_clip(self) -> float:
        """The clipping threshold in effect (0.0: off)."""
        v = np.zeros(1, np.float32)
        _check(lib().rle_get_grad_clip(self.h, _fp(v)))
        return float(v[0])

    def grad_clip_stats(self) -> dict:
        """{optimizer: (total norm, clip coefficient)} of each optimizer's last update (NaN: none yet, or off)."""
        v = np.zeros(6, np.float32)
        _check(lib().rle_grad_clip_stats(self.h, _fp(v)))
        return {k: (float(v[2 * i]), float(v[2 * i + 1])) for i, k in enumerate(("critics", "policy", "encoder"))}

    def set_layer_norm(self, critic: bool = True):
        """Parameter-free LayerNorm (eps 1e-5) after every hidden Linear of the critics and their targets, before
        the activation (TD3 / SAC).  Before the first step."""
        _check(lib().rle_set_layer_norm(self.h, ctypes.c_int(1 if critic else 0)))

    def layer_norm(self) -> bool:
        """Whether the critics carry LayerNorm (rle_get_layer_norm)."""
        v = ctypes.c_int(0)
        _check(lib().rle_get_layer_norm(self.h, ctypes.byref(v)))
        return bool(v.value)

    def set_n_step(self, n: int):
        """n-step returns (rle_set_n_step): the step's sampler gathers the n-step reward, the last hop's next_state
        and gamma^(hops-1) * notdone for every sampled slot.  1 <= n <= MAX_N_STEP, 1 off.  TD3 / SAC.  Before the
        first step."""
        _check(lib().rle_set_n_step(self.h, ctypes.c_int(int(n))))

    def n_step(self) -> int:
        """The engine's n of its n-step returns (rle_get_n_step; 1: off)."""
        v = ctypes.c_int(0)
        _check(lib().rle_get_n_step(self.h, ctypes.byref(v)))
        return int(v.value)

    def set_critic_dropout(self, p: float):
        """Inverted dropout (torch.nn.Dropout(p) in train mode) on every hidden Linear's output of the critics and
        their targets, ahead of the LayerNorm, in every critic pass of a gradient step; off in eval_q.  0 <= p < 1,
        0 off.  Needs set_layer_norm(True).  Before the first step."""
        _check(lib().rle_set_critic_dropout(self.h, ctypes.c_float(p)))

    def critic_dropout(self) -> float:
        """The critics' dropout probability (rle_get_critic_dropout; 0: off)."""
        v = np.zeros(1, np.float32)
        _check(lib().rle_get_critic_dropout(self.h, _fp(v)))
        return float(v[0])

    def dropout_mask(self, step: int, site: int, rows: int, width: int) -> np.ndarray:
        """The device's dropout mask of `site` = (pass * 2 + twin) * 8 + layer at RNG step `step`: float32
        [rows, width], 0 where dropped, 1 / (1 - p) where kept (rle_dropout_mask)."""
        out = np.empty((rows, width), np.float32)
        step = int(step) & 0xFFFFFFFFFFFFFFFF
        _check(lib().rle_dropout_mask(self.h, ctypes.c_longlong(step - (1 << 64) if step >> 63 else step),
                                      ctypes.c_int(site), ctypes.c_int(rows), ctypes.c_int(width), _fp(out)))
        return out

    def close(self):
        if self.h:
            _check(lib().rle_destroy(self.h))
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, replay: Replay):
        _check(lib().rle_bind_replay(self.h, replay.h))
        self.replay = replay

    def numel(self, net, name):
        n = _ll()
        _check(lib().rle_param_numel(self.h, net.encode(), name.encode(), ctypes.byref(n)))
        return n.value

    def get_param(self, net, name, shape=None):
        n = self.numel(net, name)
        out = np.empty(n, np.float32)
        _check(lib().rle_get_param(self.h, net.encode(), name.encode(), _fp(out), n))
        return out if shape is None else out.reshape(shape)

    def set_param(self, net, name, value):
        v = _f32(value).ravel()
        _check(lib().rle_set_param(self.h, net.encode(), name.encode(), _fp(v), v.size))

    def get_adam(self, net, name, which, shape=None):
        n = self.numel(net, name)
        out = np.empty(n, np.float32)
        _check(lib().rle_get_adam(self.h, net.encode(), name.encode(), which, _fp(out), n))
        return out if shape is None else out.reshape(shape)

    def set_adam(self, net, name, which, value):
        v = _f32(value).ravel()
        _check(lib().rle_set_adam(self.h, net.encode(), name.encode(), which, _fp(v), v.size))

    def state_toc(self, what=STATE_ALL):
        """Table of contents of the packed state of mask ``what`` (rle_state_toc): a list of
        (net, name, arena, offset, numel), arena 0 params / 1 Adam m / 2 Adam v, offsets in floats."""
        tocs = self.__dict__.setdefault("_state_tocs", {})
        if what not in tocs:
            n = _int()
            _check(lib().rle_state_toc(self.h, what, None, 0, ctypes.byref(n)))
            ent = (StateEntry * n.value)()
            _check(lib().rle_state_toc(self.h, what, ent, n.value, ctypes.byref(n)))
            tocs[what] = [(e.net.decode(), e.name.decode(), e.arena, e.offset, e.numel) for e in ent]
        return tocs[what]

    def state_size(self, what=STATE_ALL):
        toc = self.state_toc(what)
        return toc[-1][3] + toc[-1][4]

    def state_buffer(self, what=STATE_ALL):
        """This engine's reusable host array for a packed state of ``what`` (allocated once, for the full
        mask): for callers that consume a state at once, as pickling does -- the next user overwrites it."""
        buf = self.__dict__.get("_state_buf")
        if buf is None:
            buf = self._state_buf = np.empty(self.state_size(STATE_ALL), np.float32)
        return buf[:self.state_size(what)]

    def state_export(self, what=STATE_ALL, out=None):
        """The packed state of ``what`` as one fp32 array (rle_state_export: one device pass); into ``out``
        when given (e.g. state_buffer(what)), else into a new array."""
        n = self.state_size(what)
        if out is None:
            out = np.empty(n, np.float32)
        if out.dtype != np.float32 or out.shape != (n,) or not out.flags.c_contiguous:
            raise ValueError(f"state_export: out must be a contiguous float32 array of {n} elements")
        _check(lib().rle_state_export(self.h, what, _fp(out), n))
        return out

    def state_import(self, blob, what=STATE_ALL):
        blob = _f32(blob).ravel()
        _check(lib().rle_state_import(self.h, what, _fp(blob), blob.size))

    def copy_nets_from(self, other: "Engine"):
        """Every network's parameters of ``other`` (rle_copy_nets: device to device, also across two GPUs)."""
        _check(lib().rle_copy_nets(self.h, other.h))

    def counters(self):
        out = np.zeros(6, np.int64)
        _check(lib().rle_get_counters(self.h, _ip(out)))
        return out

    def act_counter(self):
        v = ctypes.c_uint64(0)
        _check(lib().rle_get_act_counter(self.h, ctypes.byref(v)))
        return int(v.value)

    def set_act_counter(self, v):
        _check(lib().rle_set_act_counter(self.h, int(v)))

    def set_counters(self, c):
        c = np.ascontiguousarray(c, np.int64)
        _check(lib().rle_set_counters(self.h, _ip(c)))

    def value_bounds(self):
        out = np.zeros(4, np.float32)
        _check(lib().rle_get_value_bounds(self.h, _fp(out)))
        return out

    def set_value_bounds(self, v):
        v = _f32(v)
        _check(lib().rle_set_value_bounds(self.h, _fp(v)))

    def step(self, n, want_info=True):
        info = np.empty((max(n, 1), INFO_MAX), np.float32) if want_info else None
        _check(lib().rle_step(self.h, n, _fp(info)))
        return info[:n] if want_info else None

    def step_timed(self, n):
        """n steps, no info readback; returns GPU ms from HIP events on the engine stream."""
        ms = ctypes.c_float()
        _check(lib().rle_step_timed(self.h, n, ctypes.byref(ms)))
        return ms.value

    def step_async(self, n):
        """Enqueue n steps on the engine's stream; no host sync, no info readback."""
        _check(lib().rle_step_async(self.h, n))

    def set_tapes(self, u=None, eps=None, eps_pi=None, ind=None):
        if u is None and ind is None:
            _check(lib().rle_set_tapes(self.h, 0, None, None, None, None))
            return
        n = (u if u is not None else ind).shape[0]
        _check(lib().rle_set_tapes(
            self.h, n, _fp(None if u is None else _f32(u)), _fp(None if eps is None else _f32(eps)),
            _fp(None if eps_pi is None else _f32(eps_pi)),
            _ip(None if ind is None else np.ascontiguousarray(ind, np.int64))))

    def last_indices(self):
        out = np.empty(self.cfg.batch, np.int64)
        _check(lib().rle_last_indices(self.h, _ip(out)))
        return out

    def act(self, obs, width):
        obs = _f32(obs)
        if obs.ndim == 1:
            obs = obs[None]
        if obs.ndim != 2 or obs.shape[1] != self.cfg.state_dim:
            raise ValueError(f"act: observation shape {obs.shape}, expected (n, {self.cfg.state_dim})")
        n = obs.shape[0]
        out = np.empty((n, width), np.float32)
        _check(lib().rle_act(self.h, _fp(obs), n, _fp(out)))
        return out

    def set_action_map(self, scale, bias, exploration_noise=0.1):
        """Environment action map of act_sample: a * scale + bias, and the TD7 / TD3
        exploration noise std (rle_set_action_map)."""
        scale = _f32(np.broadcast_to(np.asarray(scale, np.float32), (self.cfg.action_dim,)))
        bias = _f32(np.broadcast_to(np.asarray(bias, np.float32), (self.cfg.action_dim,)))
        _check(lib().rle_set_action_map(self.h, _fp(scale), _fp(bias), float(exploration_noise)))

    def act_sample(self, obs, mode, eps=None):
        """Agent.sample on the device (rle_act_sample): obs [S] or [n][S] -> environment
        actions [n][A].  mode 0 deterministic, 1 Philox exploration noise, 2 noise tape eps."""
        x = obs if (type(obs) is np.ndarray and obs.dtype == np.float32 and obs.flags.c_contiguous) else _f32(obs)
        # the kernel reads n rows of state_dim floats from this address: shapes are checked here,
        # as the reference's first Linear would reject them
        if x.ndim not in (1, 2) or x.shape[-1] != self.cfg.state_dim:
            raise ValueError(f"act_sample: observation shape {x.shape}, expected ({self.cfg.state_dim},) "
                             f"or (n, {self.cfg.state_dim})")
        n = 1 if x.ndim == 1 else x.shape[0]
        if not 1 <= n <= 1024:
            raise ValueError(f"act_sample: {n} observations (1..1024)")
        out = self._act_out.get(n)
        if out is None:
            out = self._act_out[n] = np.empty((n, self.cfg.action_dim), np.float32)
        e = 0
        if mode == 2:
            eps = _f32(eps).reshape(n, self.cfg.action_dim)
            e = eps.ctypes.data
        rc = lib().rle_act_sample(self.h, x.ctypes.data, n, mode, e, out.ctypes.data)
        if rc:
            _check(rc)
        return out

    def eval_q(self, net, s, a, enc="fixed_encoder"):
        """estimate_q_value of critic `net` on (s, a) -> [n] (TD7: embeddings of encoder `enc`)."""
        s = _f32(s)
        n = s.shape[0]
        a = _f32(a, (n, self.cfg.action_dim))
        out = np.empty(n, np.float32)
        enc_b = enc.encode() if (enc and self.cfg.algo == RLE_TD7) else None
        _check(lib().rle_eval(self.h, RLE_EVAL_Q, net.encode(), enc_b, _fp(s), _fp(a), n, _fp(out)))
        return out

    def eval_zs(self, enc, s):
        """encode_state of encoder `enc` (TD7) -> [n][zs_dim]."""
        s = _f32(s)
        n = s.shape[0]
        out = np.empty((n, self.cfg.zs_dim or self.cfg.hidden), np.float32)
        _check(lib().rle_eval(self.h, RLE_EVAL_ZS, enc.encode(), None, _fp(s), None, n, _fp(out)))
        return out

    def eval_zsa(self, enc, s, a):
        """encode_state_action(encode_state(s), a) of encoder `enc` (TD7) -> [n][zs_dim]."""
        s = _f32(s)
        n = s.shape[0]
        a = _f32(a, (n, self.cfg.action_dim))
        out = np.empty((n, self.cfg.zs_dim or self.cfg.hidden), np.float32)
        _check(lib().rle_eval(self.h, RLE_EVAL_ZSA, enc.encode(), None, _fp(s), _fp(a), n, _fp(out)))
        return out

    def sac_rsample(self, mean, log_std, eps):
        """SAC._rsample through the device op: (tanh action [n][A], log_pi [n])."""
        mean = _f32(mean)
        n, A = mean.shape
        log_std, eps = _f32(log_std, (n, A)), _f32(eps, (n, A))
        act = np.empty((n, A), np.float32)
        lp = np.empty(n, np.float32)
        _check(lib().rle_sac_rsample(self.h, _fp(mean), _fp(log_std), _fp(eps), n, _fp(act), _fp(lp)))
        return act, lp

    def get_info(self, n):
        """Info rows of the last step / step_async call."""
        out = np.empty((max(n, 1), INFO_MAX), np.float32)
        _check(lib().rle_get_info(self.h, n, _fp(out)))
        return out[:n]

    def launch_count(self):
        n = ctypes.c_longlong()
        _check(lib().rle_launch_count(self.h, ctypes.byref(n)))
        return n.value

    def graph_stats(self):
        a, b = _int(), _int()
        _check(lib().rle_graph_stats(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def describe(self, which=0):
        buf = ctypes.create_string_buffer(1 << 16)
        _check(lib().rle_graph_describe(self.h, which, buf, len(buf)))
        return buf.value.decode()

    def trace(self, which=0):
        """Per-workgroup phase timestamps of the last replay of graph `which` (RLE_TRACE=1):
        (workgroups, 4) -- or 16 columns from a -DRLE_TRACE_FINE build."""
        n = ctypes.c_longlong()
        _check(lib().rle_graph_trace(self.h, which, None, 0, ctypes.byref(n)))
        stride = lib().rle_trace_stride()
        if n.value == 0:
            return np.zeros((0, stride), np.uint64)
        out = np.zeros((n.value, stride), np.uint64)
        _check(lib().rle_graph_trace(self.h, which, out.ctypes.data, out.size, ctypes.byref(n)))
        return out

    def copy_state_from(self, other: "Engine"):
        _check(lib().rle_copy_state(self.h, other.h))

    def synchronize(self):
        _check(lib().rle_synchronize(self.h))


def check_n_step(algo, n_step) -> int:
    """The n of n-step returns as rle_set_n_step checks it, before an engine exists: an int in 1 .. MAX_N_STEP
    (1: off), and 1 on TD7, whose encoder learns the one-step model zsa(s, a) -> zs(s') from the same next-state
    rows.  Returns it as an int; anything else is a ValueError."""
    if isinstance(n_step, bool) or int(n_step) != n_step:
        raise ValueError(f"n_step {n_step!r}: an integer in 1 .. {MAX_N_STEP}")
    n = int(n_step)
    if not 1 <= n <= MAX_N_STEP:
        raise ValueError(f"n_step {n}: must be in 1 .. {MAX_N_STEP} (1: one-step targets)")
    if n > 1 and algo == RLE_TD7:
        raise ValueError("n_step > 1 is TD3 / SAC only: TD7's encoder learns the one-step model zsa(s, a) -> zs(s') "
                         "from the same next-state rows")
    return n


def make_config(algo, state_dim, action_dim, hidden, batch, use_lap=False, discount=0.99,
                policy_lr=3e-4, critic_lr=3e-4, tau=0.005, target_policy_noise=0.2,
                noise_clip=0.5, policy_freq=2, target_update_rate=250, min_log_std=-20.0,
                max_log_std=2.0, tmp=-1.0, seed=0, device=0, zs_dim=0, hidden_sizes=None,
                act_actor="default", act_critic="default", act_encoder="default", bc_lambda=0.0) -> Config:
    """``hidden``: TD7 hdim, TD3 / SAC the width of both hidden layers; ``zs_dim`` (TD7, 0 = hidden) and
    ``hidden_sizes`` (TD3 / SAC: make_mlp's list, 2..6 layers) give the other net shapes (include/rle.h).
    ``act_*``: hidden activations, "relu" / "elu" (alpha 1) / "identity" / "leaky_relu" (slope 0.01) / "silu" /
    "gelu" (the exact erf form) or "default"; any other name is a ValueError.
    ``bc_lambda`` (TD7): 0 online; > 0 the offline mode's behaviour-cloning weight (rle_config bc_lambda)."""
    hs = list(hidden_sizes) if hidden_sizes is not None else []
    if hs and not 2 <= len(hs) <= 6:
        raise ValueError(f"hidden_sizes {hs}: 2..6 hidden layers")
    acts = []
    for a in (act_actor, act_critic, act_encoder):
        if a not in ACT_CODES:
            raise ValueError(f"activation {a!r}: one of {sorted(ACT_CODES)}")
        acts.append(ACT_CODES[a])
    return Config(algo, state_dim, action_dim, hs[-1] if hs else hidden, batch, int(use_lap), discount,
                  policy_lr, critic_lr, tau, target_policy_noise, noise_clip, policy_freq, target_update_rate,
                  min_log_std, max_log_std, tmp, seed, device, zs_dim, len(hs),
                  (_int * 8)(*(hs + [0] * (8 - len(hs)))), *acts, float(bc_lambda))
