"""glfsx_post_ragged_device's C-ABI: the symbol, its signature and what it
answers before any device work.  CPU-only."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RAGGED = 16 << 20


def _decl():
    txt = open(os.path.join(ROOT, "include", "glfsx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"int\s+glfsx_post_ragged_device\s*\(([^)]*)\)\s*;", txt)
    assert m, "glfsx_post_ragged_device is not declared in include/glfsx.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbol_and_signature():
    from glfs_amd import _native as N
    assert _decl() == [
        "const uint8_t salt[32]", "const uint8_t *cid_key", "const void *d_data",
        "const uint64_t *d_offsets", "const uint64_t *d_lengths", "uint64_t n",
        "uint64_t max_len", "void *d_ctext", "void *d_refs", "void *stream"]
    res, args = N.SIGNATURES["glfsx_post_ragged_device"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(N.lib, "glfsx_post_ragged_device")


def test_answers_before_device_work():
    """n == 0 is done; a null array is an argument error; a max_len above
    16 MiB is unsupported -- all three decided before a device is looked for,
    so they hold with and without one."""
    from glfs_amd import _native as N
    f = N.lib.glfsx_post_ragged_device
    salt = bytes(32)
    p = 4096  # never dereferenced: every call below returns before a launch
    assert f(salt, None, None, None, None, 0, 0, None, None, None) == 0
    assert f(salt, None, p, p, p, 0, MAX_RAGGED + 1, None, p, None) == 0
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        d, o, ln, r = args
        assert f(salt, None, d, o, ln, 1, 1024, None, r, None) == N.GLFSX_E_ARG, args
    assert f(salt, None, p, p, p, 1, MAX_RAGGED + 1, None, p, None) == N.GLFSX_E_UNSUPPORTED
    assert "16777217" in N.last_error()


def test_no_device_is_a_device_error():
    from glfs_amd import _native as N
    if N.device_count() > 0:
        pytest.skip("GPU present")
    p = 4096
    rc = N.lib.glfsx_post_ragged_device(bytes(32), None, p, p, p, 1, 1024, None, p, None)
    assert rc == N.GLFSX_E_DEVICE
    assert "no HIP device" in N.last_error()
