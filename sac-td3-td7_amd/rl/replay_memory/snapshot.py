"""Replay snapshots on disk: a directory of ``meta.json`` plus one ``.npy`` file per array.

The reference's replays are NumPy arrays that pickle as they are (lap.py:18-29, simple.py:15-27).
A device replay of 1M Humanoid transitions is 3.1 GB, so ``BaseReplayMemory.save`` streams it
instead: ``meta.json`` holds the settings (capacity, dims, ptr, size, max_priority, ...), and
``state.npy``, ``action.npy``, ``reward.npy``, ``next_state.npy``, ``notdone.npy`` (and
``priority.npy`` for LAP) hold rows ``[0, size)`` in slot order, written and read through
``numpy.lib.format.open_memmap`` one chunk at a time.  ``ind.npy`` (optional) keeps the indices
of the last batch.

Nothing here touches the engine: the writer takes NumPy chunks, the reader yields them.
"""

from __future__ import annotations

import json
import os

import numpy as np
from numpy.lib.format import open_memmap

FORMAT = 1
META = "meta.json"
FIELDS = ("state", "action", "reward", "next_state", "notdone")
_META_KEYS = ("format", "capacity", "state_dim", "action_dim", "lap", "ptr", "size", "max_priority",
              "env_id", "action_bias", "action_scale")


def field_names(lap: bool) -> tuple:
    """Array names of a snapshot, in the order of the packed rows."""
    return FIELDS + (("priority",) if lap else ())


def field_shape(name: str, rows: int, state_dim: int, action_dim: int) -> tuple:
    if name in ("state", "next_state"):
        return (rows, state_dim)
    if name == "action":
        return (rows, action_dim)
    return (rows,)


def make_meta(*, capacity, state_dim, action_dim, lap, ptr, size, max_priority, env_id=None,
              action_bias=None, action_scale=None) -> dict:
    """The settings of a replay as JSON scalars and lists."""
    vec = lambda v, fill: [float(x) for x in (np.full(action_dim, fill) if v is None else np.asarray(v).reshape(-1))]
    return {"format": FORMAT, "capacity": int(capacity), "state_dim": int(state_dim), "action_dim": int(action_dim),
            "lap": bool(lap), "ptr": int(ptr), "size": int(size), "max_priority": float(max_priority),
            "env_id": None if env_id is None else str(env_id),
            "action_bias": vec(action_bias, 0.0), "action_scale": vec(action_scale, 1.0)}


def validate_meta(meta: dict, *, capacity=None, state_dim=None, action_dim=None, lap=None) -> dict:
    """Checks a snapshot's settings (and, where given, that they fit a replay of that capacity,
    those dims and that LAP-ness).  Every failure is a ValueError that names the field."""
    if not isinstance(meta, dict):
        raise ValueError("meta: not a mapping")
    for k in _META_KEYS:
        if k not in meta:
            raise ValueError(f"meta: field {k!r} is missing")
    if meta["format"] != FORMAT:
        raise ValueError(f"format: snapshot format version {meta['format']!r}, this reader knows {FORMAT}")
    for k in ("capacity", "state_dim", "action_dim", "ptr", "size"):
        if not isinstance(meta[k], int) or isinstance(meta[k], bool) or meta[k] < 0:
            raise ValueError(f"{k}: {meta[k]!r} is not a non-negative integer")
    if not isinstance(meta["lap"], bool):
        raise ValueError(f"lap: {meta['lap']!r} is not a boolean")
    if meta["capacity"] < 1 or meta["state_dim"] < 1 or meta["action_dim"] < 1:
        raise ValueError("capacity / state_dim / action_dim: must be positive")
    if meta["size"] > meta["capacity"]:
        raise ValueError(f"size: {meta['size']} rows in a replay of capacity {meta['capacity']}")
    if meta["ptr"] >= meta["capacity"]:
        raise ValueError(f"ptr: {meta['ptr']} is outside a ring of capacity {meta['capacity']}")
    mp = meta["max_priority"]
    if not isinstance(mp, (int, float)) or isinstance(mp, bool) or not np.isfinite(mp) or mp <= 0:
        raise ValueError(f"max_priority: {mp!r} is not a finite positive number")
    for k in ("action_bias", "action_scale"):
        if not isinstance(meta[k], list) or len(meta[k]) != meta["action_dim"]:
            raise ValueError(f"{k}: needs {meta['action_dim']} numbers")
    for k, want in (("capacity", capacity), ("state_dim", state_dim), ("action_dim", action_dim), ("lap", lap)):
        if want is not None and meta[k] != want:
            raise ValueError(f"{k}: snapshot has {meta[k]!r}, the replay {want!r}")
    return meta


def validate_arrays(meta: dict, arrays: dict) -> None:
    """Every array of the snapshot present, float32 and of shape [size][dim] / [size]."""
    for name in field_names(meta["lap"]):
        if name not in arrays:
            raise ValueError(f"{name}: array is missing")
        a = arrays[name]
        want = field_shape(name, meta["size"], meta["state_dim"], meta["action_dim"])
        if tuple(a.shape) != want:
            raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {want}")
        if a.dtype != np.float32:
            raise ValueError(f"{name}: dtype {a.dtype}, expected float32")
    if not meta["lap"] and "priority" in arrays and arrays["priority"] is not None:
        raise ValueError("priority: array given for a replay without LAP")


class SnapshotWriter:
    """Writes a snapshot directory chunk by chunk: ``write(chunk)`` appends the rows of a dict of
    arrays (every field of the snapshot, equal row counts); ``close`` checks that exactly ``size``
    rows arrived and writes ``meta.json`` last, so an interrupted save never looks complete."""

    def __init__(self, path, meta: dict, ind=None):
        self.path = os.fspath(path)
        self.meta = validate_meta(dict(meta))
        self.names = field_names(self.meta["lap"])
        os.makedirs(self.path, exist_ok=True)
        stale = os.path.join(self.path, META)
        if os.path.exists(stale):
            os.remove(stale)
        n, S, A = self.meta["size"], self.meta["state_dim"], self.meta["action_dim"]
        self.maps = {}
        for k in self.names:
            f = os.path.join(self.path, k + ".npy")
            if n == 0:  # (an empty file cannot be memory-mapped)
                np.save(f, np.empty(field_shape(k, 0, S, A), np.float32))
            else:
                self.maps[k] = open_memmap(f, mode="w+", dtype=np.float32, shape=field_shape(k, n, S, A))
        ind_path = os.path.join(self.path, "ind.npy")
        if ind is not None:
            np.save(ind_path, np.asarray(ind, np.int64))
        elif os.path.exists(ind_path):
            os.remove(ind_path)
        self.rows = 0

    def write(self, chunk: dict) -> None:
        c = len(chunk["reward"])
        if c == 0:
            return
        if self.rows + c > self.meta["size"]:
            raise ValueError(f"size: chunk of {c} rows at row {self.rows} exceeds {self.meta['size']}")
        for k in self.names:
            if k not in chunk:
                raise ValueError(f"{k}: array is missing from the chunk")
            a = np.asarray(chunk[k], np.float32)
            want = field_shape(k, c, self.meta["state_dim"], self.meta["action_dim"])
            if a.shape != want:
                raise ValueError(f"{k}: chunk shape {a.shape}, expected {want}")
            self.maps[k][self.rows:self.rows + c] = a
        self.rows += c

    def close(self) -> None:
        if self.rows != self.meta["size"]:
            raise ValueError(f"size: {self.rows} rows written, meta says {self.meta['size']}")
        for m in self.maps.values():
            m.flush()
        self.maps = {}
        with open(os.path.join(self.path, META), "w") as fh:
            json.dump(self.meta, fh, indent=1)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.maps = {}


def write_snapshot(path, meta: dict, chunks, ind=None) -> None:
    """``chunks``: an iterable of dicts of arrays, in slot order."""
    with SnapshotWriter(path, meta, ind) as w:
        for c in chunks:
            w.write(c)


class SnapshotReader:
    """Opens a snapshot directory: ``meta`` validated (optionally against a replay's capacity, dims
    and LAP-ness), every ``.npy`` memory-mapped and checked; ``chunks(rows)`` yields
    ``(first_row, {name: ndarray})`` with at most ``rows`` rows each, copied out of the maps."""

    def __init__(self, path, **expect):
        self.path = os.fspath(path)
        mp = os.path.join(self.path, META)
        if not os.path.isfile(mp):
            raise ValueError(f"meta: {mp} does not exist (not a replay snapshot, or an interrupted save)")
        with open(mp) as fh:
            try:
                meta = json.load(fh)
            except json.JSONDecodeError as e:
                raise ValueError(f"meta: {mp} is not JSON ({e})") from e
        self.meta = validate_meta(meta, **expect)
        self.maps = {}
        for k in field_names(self.meta["lap"]):
            f = os.path.join(self.path, k + ".npy")
            if not os.path.isfile(f):
                raise ValueError(f"{k}: {f} does not exist")
            try:
                self.maps[k] = np.load(f, mmap_mode="r" if self.meta["size"] else None, allow_pickle=False)
            except (ValueError, EOFError, OSError) as e:  # (a truncated file: header or data cut short)
                raise ValueError(f"{k}: {f} is truncated or not an .npy file ({e})") from e
        validate_arrays(self.meta, self.maps)
        ind_path = os.path.join(self.path, "ind.npy")
        self.ind = np.load(ind_path, allow_pickle=False).astype(np.int64) if os.path.isfile(ind_path) else None

    def chunks(self, rows: int):
        n = self.meta["size"]
        for first in range(0, n, int(rows)):
            c = min(int(rows), n - first)
            yield first, {k: np.ascontiguousarray(m[first:first + c]) for k, m in self.maps.items()}


def read_snapshot(path, rows: int, **expect):
    """(meta, ind, iterator of (first_row, chunk)) of a snapshot directory."""
    r = SnapshotReader(path, **expect)
    return r.meta, r.ind, r.chunks(rows)
