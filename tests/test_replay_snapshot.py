"""Replay snapshots without a GPU: the directory writer / reader / validator (rl/replay_memory/snapshot.py)
and the argument checks of the replay export / import ABI, which come before any HIP call."""

import ctypes
import json
import os

import numpy as np
import pytest

from rl import _engine as E
from rl.replay_memory import snapshot as SN

S, A = 11, 3


def _meta(size, lap, cap=100, ptr=None):
    return SN.make_meta(capacity=cap, state_dim=S, action_dim=A, lap=lap, ptr=size % cap if ptr is None else ptr,
                        size=size, max_priority=np.float32(1.7), env_id="Tiny-v0",
                        action_bias=np.zeros(A, np.float32), action_scale=np.full(A, 0.5, np.float32))


def _arrays(size, lap, seed=0):
    rng = np.random.default_rng(seed)
    a = {k: rng.standard_normal(SN.field_shape(k, size, S, A)).astype(np.float32) for k in SN.field_names(lap)}
    if lap:
        a["priority"] = np.abs(a["priority"]) + 1
    return a


def _chunks(arrays, sizes):
    first = 0
    for c in sizes:
        yield {k: v[first:first + c] for k, v in arrays.items()}
        first += c


@pytest.mark.parametrize("lap", [True, False])
@pytest.mark.parametrize("size,sizes,rows", [(37, (5, 0, 17, 1, 14), 8), (64, (64,), 64), (9, (4, 5), 100), (0, (), 8)])
def test_writer_reader_roundtrip(tmp_path, lap, size, sizes, rows):
    arrays = _arrays(size, lap)
    meta = _meta(size, lap)
    ind = np.array([3, 1, 4, 1, 5], np.int64) if size else None
    SN.write_snapshot(tmp_path / "snap", meta, _chunks(arrays, sizes), ind)
    assert sorted(os.listdir(tmp_path / "snap")) == sorted(
        ["meta.json"] + [k + ".npy" for k in SN.field_names(lap)] + (["ind.npy"] if size else []))
    got_meta, got_ind, chunks = SN.read_snapshot(tmp_path / "snap", rows, capacity=100, state_dim=S, action_dim=A,
                                                 lap=lap)
    assert got_meta == meta
    assert np.float32(got_meta["max_priority"]) == np.float32(1.7)
    if size:
        np.testing.assert_array_equal(got_ind, ind)
    else:
        assert got_ind is None
    seen = 0
    for first, c in chunks:
        assert first == seen and set(c) == set(SN.field_names(lap))
        n = len(c["reward"])
        assert 0 < n <= rows
        for k, v in c.items():
            assert v.dtype == np.float32 and v.flags.c_contiguous
            np.testing.assert_array_equal(v, arrays[k][first:first + n])
        seen += n
    assert seen == size


def test_meta_json_holds_only_scalars_and_lists(tmp_path):
    SN.write_snapshot(tmp_path / "s", _meta(12, True), _chunks(_arrays(12, True), (12,)))
    meta = json.load(open(tmp_path / "s" / "meta.json"))
    assert set(meta) == {"format", "capacity", "state_dim", "action_dim", "lap", "ptr", "size", "max_priority",
                         "env_id", "action_bias", "action_scale"}
    for k, v in meta.items():
        if isinstance(v, list):
            assert all(type(x) in (int, float) for x in v), k
        else:
            assert v is None or type(v) in (int, float, bool, str), k
    assert meta["format"] == SN.FORMAT and meta["size"] == 12 and meta["lap"] is True


def test_writer_refuses_wrong_row_counts_and_shapes(tmp_path):
    arrays = _arrays(10, False)
    with pytest.raises(ValueError, match="size"):
        SN.write_snapshot(tmp_path / "short", _meta(10, False), _chunks(arrays, (4,)))
    assert not os.path.exists(tmp_path / "short" / "meta.json")  # an incomplete save never looks complete
    with pytest.raises(ValueError, match="size"):
        SN.write_snapshot(tmp_path / "long", _meta(10, False), _chunks(_arrays(14, False), (7, 7)))
    bad = dict(arrays, action=np.zeros((10, A + 1), np.float32))
    with pytest.raises(ValueError, match="action"):
        SN.write_snapshot(tmp_path / "shape", _meta(10, False), [bad])


def test_validation_errors_name_the_field(tmp_path):
    path = tmp_path / "s"
    SN.write_snapshot(path, _meta(20, True), _chunks(_arrays(20, True), (20,)))
    ok = dict(capacity=100, state_dim=S, action_dim=A, lap=True)
    SN.SnapshotReader(path, **ok)
    for field, value in (("state_dim", S + 1), ("action_dim", A + 2), ("capacity", 101), ("lap", False)):
        with pytest.raises(ValueError, match=field):
            SN.SnapshotReader(path, **dict(ok, **{field: value}))
    # a truncated array
    f = path / "next_state.npy"
    data = f.read_bytes()
    f.write_bytes(data[:len(data) - 40])
    with pytest.raises(ValueError, match="next_state"):
        SN.SnapshotReader(path, **ok)
    f.write_bytes(data[:30])  # (inside the header)
    with pytest.raises(ValueError, match="next_state"):
        SN.SnapshotReader(path, **ok)
    f.write_bytes(data)
    # an array of another width
    np.save(path / "action.npy", np.zeros((20, A + 1), np.float32))
    with pytest.raises(ValueError, match="action"):
        SN.SnapshotReader(path, **ok)
    np.save(path / "action.npy", np.zeros((20, A), np.float32))
    os.remove(path / "priority.npy")
    with pytest.raises(ValueError, match="priority"):
        SN.SnapshotReader(path, **ok)
    np.save(path / "priority.npy", np.ones(20, np.float32))
    SN.SnapshotReader(path, **ok)
    # an unknown format version, and settings that contradict each other
    meta = json.load(open(path / "meta.json"))
    for field, value in (("format", SN.FORMAT + 1), ("size", 101), ("ptr", 100), ("max_priority", 0.0),
                         ("max_priority", float("nan")), ("action_scale", [1.0])):
        json.dump(dict(meta, **{field: value}), open(path / "meta.json", "w"))
        with pytest.raises(ValueError, match=field):
            SN.SnapshotReader(path, **ok)
    os.remove(path / "meta.json")
    with pytest.raises(ValueError, match="meta"):
        SN.SnapshotReader(path, **ok)


def test_state_dict_validation_without_a_ring():
    meta = _meta(6, True)
    arrays = _arrays(6, True)
    SN.validate_arrays(meta, arrays)
    with pytest.raises(ValueError, match="reward"):
        SN.validate_arrays(meta, dict(arrays, reward=arrays["reward"][:5]))
    with pytest.raises(ValueError, match="state"):
        SN.validate_arrays(meta, dict(arrays, state=arrays["state"].astype(np.float64)))
    with pytest.raises(ValueError, match="priority"):
        SN.validate_arrays(_meta(6, False), arrays)


def test_replay_io_abi_checks_arguments_before_any_hip_call():
    """rle_replay_export / _import / _set_state / _copy with a null handle return RLE_EINVAL with a message
    (no GPU is touched), as rle_replay_create does for bad sizes."""
    lib = E.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float))
    assert lib.rle_replay_export(None, 0, 1, p, None, None, None, None, None) == -1
    assert b"export" in lib.rle_last_error()
    assert lib.rle_replay_import(None, 0, 1, p, None, None, None, None, None) == -1
    assert b"import" in lib.rle_last_error()
    assert lib.rle_replay_set_state(None, 0, 0, 1.0) == -1
    assert b"set_state" in lib.rle_last_error()
    assert lib.rle_replay_copy(None, None) == -1
    assert b"copy" in lib.rle_last_error()


def test_replay_io_rows_is_the_module_constant():
    assert E.lib().rle_replay_io_rows() == E.REPLAY_IO_ROWS
    assert E.REPLAY_IO_ROWS in (8192, 16384)
