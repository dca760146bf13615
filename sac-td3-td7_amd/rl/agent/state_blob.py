"""Packed agent state <-> the nested dict an engine agent pickles.  No GPU needed.

``rle_state_export`` (include/rle.h) returns every parameter and Adam moment of an engine as ONE
fp32 array, described by a table of contents: a list of ``(net, name, arena, offset, numel)`` with
arena 0 params / 1 Adam m / 2 Adam v and offsets in floats.  The agents keep the dict they always
pickled::

    {"params": {net: {name: array}}, "adam": {net: {name: (m, v)}}}

so pickles written through the per-tensor path still load.  The functions here cut that dict out of
a blob and assemble a blob from it.
"""

from __future__ import annotations

import numpy as np

PARAMS, ADAM_M, ADAM_V = 0, 1, 2


def toc_size(toc) -> int:
    """Floats of the packed state a table of contents describes (entries are contiguous)."""
    return max((off + n for _, _, _, off, n in toc), default=0)


def blob_to_dict(toc, blob, shapes=None):
    """Views of ``blob`` per tensor.  ``shapes``: {(net, name): shape} (default: flat arrays).
    Nets and names keep the TOC's order; an arena the TOC does not list gives no key."""
    blob = np.asarray(blob, np.float32).reshape(-1)
    if blob.size != toc_size(toc):
        raise ValueError(f"packed state of {blob.size} floats, the table of contents describes {toc_size(toc)}")
    shapes = shapes or {}
    cut = {PARAMS: {}, ADAM_M: {}, ADAM_V: {}}
    for net, name, arena, off, n in toc:
        cut[arena].setdefault(net, {})[name] = blob[off:off + n].reshape(shapes.get((net, name), (n,)))
    out = {}
    if cut[PARAMS]:
        out["params"] = cut[PARAMS]
    if cut[ADAM_M] or cut[ADAM_V]:
        if {(k, n) for k, d in cut[ADAM_M].items() for n in d} != {(k, n) for k, d in cut[ADAM_V].items() for n in d}:
            raise ValueError("the table of contents lists Adam m and v of different tensors")
        out["adam"] = {net: {name: (m, cut[ADAM_V][net][name]) for name, m in d.items()}
                       for net, d in cut[ADAM_M].items()}
    return out


def covers(toc, st) -> bool:
    """True when ``st`` holds exactly the tensors of ``toc`` (so one blob can carry it)."""
    want = {PARAMS: set(), ADAM_M: set()}
    for net, name, arena, _, _ in toc:
        want[min(arena, ADAM_M)].add((net, name))
    have_p = {(net, name) for net, d in st.get("params", {}).items() for name in d}
    have_a = {(net, name) for net, d in st.get("adam", {}).items() for name in d}
    return have_p == want[PARAMS] and have_a == want[ADAM_M]


def dict_to_blob(toc, st, out=None):
    """One fp32 array laid out by ``toc`` from ``st`` (into ``out`` when given); a tensor of another
    size raises ValueError."""
    blob = np.empty(toc_size(toc), np.float32) if out is None else out
    if blob.dtype != np.float32 or blob.shape != (toc_size(toc),):
        raise ValueError(f"out must be a float32 array of {toc_size(toc)} elements")
    for net, name, arena, off, n in toc:
        v = st["params"][net][name] if arena == PARAMS else st["adam"][net][name][arena - 1]
        v = np.asarray(v, np.float32)
        if v.size != n:
            raise ValueError(f"size mismatch for {net}.{name}: {v.size} values, expected {n}")
        blob[off:off + n] = v.reshape(-1)
    return blob
