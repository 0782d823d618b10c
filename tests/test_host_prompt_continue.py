"""CPU tests of the prompt-continuation attention's host side (ABI v20, paro_attn_prompt): the version, and argument validation that
returns PARO_ERR_INVALID with a message before any launch."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from paroquant_amd import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_abi_version_is_20(lib):
    from paroquant_amd import _native
    assert _native.PARO_ABI_VERSION == 20 and lib.paro_abi_version() == 20
    assert "paro_attn_prompt" in _native.EXPORTS and hasattr(lib, "paro_attn_prompt")


@pytest.mark.parametrize("case, kw, text", [
    ("head_dim 256", dict(head_dim=256), b"head_dim"),
    ("head_dim 96", dict(head_dim=96), b"head_dim"),
    ("past max_positions", dict(pos0=60, rows=5), b"max_positions"),
    ("negative pos0", dict(pos0=-1), b"max_positions"),
    ("rows 0", dict(rows=0), b"rows"),
    ("rows -3", dict(rows=-3), b"rows"),
    ("ratio 12 / 5", dict(n_heads=12, n_kv_heads=5), b"multiple"),
    ("no kv heads", dict(n_kv_heads=0), b"multiple"),
    ("max_positions 60", dict(max_positions=60, pos0=0, rows=8), b"multiple of 8"),
    ("fp32", dict(act_dtype=0), b"act_dtype"),
])
def test_attn_prompt_validation_without_gpu(lib, case, kw, text):
    from paroquant_amd import _native as nat
    one = ctypes.c_void_p(1)
    a = dict(rows=4, pos0=8, n_heads=8, n_kv_heads=2, head_dim=128, max_positions=64, act_dtype=nat.DTYPE_F16)
    a.update(kw)
    rc = lib.paro_attn_prompt(one, one, one, one, a["rows"], a["pos0"], a["n_heads"], a["n_kv_heads"], a["head_dim"], a["max_positions"],
                              a["act_dtype"], None)
    assert rc == -1, case
    assert text in lib.paro_last_error(), (case, lib.paro_last_error())


def test_attn_prompt_rejects_null_pointers(lib):
    one = ctypes.c_void_p(1)
    assert lib.paro_attn_prompt(one, None, one, one, 4, 0, 8, 2, 64, 64, 1, None) == -1
    assert b"null" in lib.paro_last_error()
