"""The packed agent state on the host (no GPU): the table-of-contents record of include/rle.h against its
ctypes mirror, and the blob <-> dict slicing of rl/agent/state_blob.py on a hand-made table of contents."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from rl import _engine as E
from rl.agent.state_blob import blob_to_dict, covers, dict_to_blob, toc_size


def test_state_entry_matches_the_header_layout(tmp_path):
    """rl/_engine.py StateEntry mirrors rle_state_entry field by field: a C program compiled against
    include/rle.h prints the struct's size and every field's offset (gcc on the host, no GPU)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lines = ['printf("size %zu\\n", sizeof(rle_state_entry));']
    for f, *_ in E.StateEntry._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rle_state_entry, {f}));')
    for name in ("RLE_STATE_PARAMS", "RLE_STATE_ADAM_M", "RLE_STATE_ADAM_V", "RLE_STATE_ALL"):
        lines.append(f'printf("{name} %d\\n", {name});')
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rle.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                    text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(E.StateEntry) == 88
    for f, *_ in E.StateEntry._fields_:
        assert int(got[f]) == getattr(E.StateEntry, f).offset, f
    assert (int(got["RLE_STATE_PARAMS"]), int(got["RLE_STATE_ADAM_M"]), int(got["RLE_STATE_ADAM_V"]),
            int(got["RLE_STATE_ALL"])) == (E.STATE_PARAMS, E.STATE_ADAM_M, E.STATE_ADAM_V, E.STATE_ALL)


# A SAC-like table of contents by hand: params of two nets and the temperature, then m and v of the one net
# with an optimiser and of the temperature.  (net, name, arena, offset, numel)
TOC = [
    ("policy", "mlp.0.weight", 0, 0, 6), ("policy", "mlp.0.bias", 0, 6, 2),
    ("target_q1", "mlp.0.weight", 0, 8, 3), ("target_q1", "mlp.0.bias", 0, 11, 1),
    ("tmp", "log_alpha", 0, 12, 1),
    ("policy", "mlp.0.weight", 1, 13, 6), ("policy", "mlp.0.bias", 1, 19, 2), ("tmp", "log_alpha", 1, 21, 1),
    ("policy", "mlp.0.weight", 2, 22, 6), ("policy", "mlp.0.bias", 2, 28, 2), ("tmp", "log_alpha", 2, 30, 1),
]
SHAPES = {("policy", "mlp.0.weight"): (2, 3), ("policy", "mlp.0.bias"): (2,),
          ("target_q1", "mlp.0.weight"): (1, 3), ("target_q1", "mlp.0.bias"): (1,)}


def test_blob_to_dict_cuts_by_offset_in_toc_order():
    assert toc_size(TOC) == 31 and toc_size([]) == 0
    blob = np.arange(31, dtype=np.float32)
    d = blob_to_dict(TOC, blob, SHAPES)
    assert list(d) == ["params", "adam"]
    assert list(d["params"]) == ["policy", "target_q1", "tmp"] and list(d["adam"]) == ["policy", "tmp"]
    assert list(d["params"]["policy"]) == ["mlp.0.weight", "mlp.0.bias"]
    np.testing.assert_array_equal(d["params"]["policy"]["mlp.0.weight"], [[0, 1, 2], [3, 4, 5]])
    np.testing.assert_array_equal(d["params"]["policy"]["mlp.0.bias"], [6, 7])
    np.testing.assert_array_equal(d["params"]["target_q1"]["mlp.0.weight"], [[8, 9, 10]])
    # the SAC scalar: one float, shape (1,), as rle_get_param returns it
    assert d["params"]["tmp"]["log_alpha"].shape == (1,) and d["params"]["tmp"]["log_alpha"][0] == 12
    m, v = d["adam"]["policy"]["mlp.0.weight"]
    np.testing.assert_array_equal(m, np.arange(13, 19).reshape(2, 3))
    np.testing.assert_array_equal(v, np.arange(22, 28).reshape(2, 3))
    m, v = d["adam"]["tmp"]["log_alpha"]
    assert (m.shape, float(m[0]), v.shape, float(v[0])) == ((1,), 21.0, (1,), 30.0)
    assert all(a.dtype == np.float32 for net in d["params"].values() for a in net.values())
    # views of the one blob, no copies
    assert np.shares_memory(d["params"]["policy"]["mlp.0.weight"], blob) and np.shares_memory(v, blob)
    with pytest.raises(ValueError, match="31"):
        blob_to_dict(TOC, blob[:30], SHAPES)


def test_params_only_toc_gives_no_adam_key():
    ptoc = [t for t in TOC if t[2] == 0]
    d = blob_to_dict(ptoc, np.arange(13, dtype=np.float32))
    assert list(d) == ["params"] and d["params"]["policy"]["mlp.0.weight"].shape == (6,)


def test_dict_to_blob_is_the_inverse_and_checks_sizes():
    blob = np.random.default_rng(0).standard_normal(31).astype(np.float32)
    d = blob_to_dict(TOC, blob, SHAPES)
    assert covers(TOC, d)
    np.testing.assert_array_equal(dict_to_blob(TOC, d), blob)
    # any array-like of the right size, in any key order, lands at its TOC offset
    shuffled = {"adam": {k: dict(reversed(list(v.items()))) for k, v in reversed(list(d["adam"].items()))},
                "params": {k: {n: a.astype(np.float64).tolist() for n, a in v.items()}
                           for k, v in reversed(list(d["params"].items()))}}
    np.testing.assert_array_equal(dict_to_blob(TOC, shuffled), blob)
    ptoc = [t for t in TOC if t[2] == 0]
    np.testing.assert_array_equal(dict_to_blob(ptoc, {"params": d["params"]}), blob[:13])
    # into a caller's array -- also the one the views were cut from (an agent re-importing its own export)
    out = np.zeros(31, np.float32)
    assert dict_to_blob(TOC, d, out) is out and np.array_equal(out, blob)
    assert dict_to_blob(TOC, d, blob) is blob and np.array_equal(out, blob)
    with pytest.raises(ValueError, match="31"):
        dict_to_blob(TOC, d, np.zeros(30, np.float32))
    bad ={"params": dict(d["params"], policy=dict(d["params"]["policy"], **{"mlp.0.bias": np.zeros(3)})),
           "adam": d["adam"]}
    with pytest.raises(ValueError, match="policy.mlp.0.bias"):
        dict_to_blob(TOC, bad)


def test_covers_tells_whole_states_from_partial_ones():
    d = blob_to_dict(TOC, np.zeros(31, np.float32), SHAPES)
    ptoc = [t for t in TOC if t[2] == 0]
    assert covers(TOC, d) and covers(ptoc, {"params": d["params"]})
    assert not covers(TOC, {"params": d["params"]})                      # no moments for a full TOC
    assert not covers(ptoc, d)                                           # moments a params TOC does not list
    assert not covers(ptoc, {"params": {"policy": d["params"]["policy"]}})   # load_params of one net
    no_tmp = {k: v for k, v in d["params"].items() if k != "tmp"}
    assert not covers(ptoc, {"params": no_tmp})                          # freshly initialised nets, no temperature
    extra = dict(d["params"], q9={"w": np.zeros(1)})
    assert not covers(ptoc, {"params": extra})
