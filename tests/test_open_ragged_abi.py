"""The ragged open's entry points without a GPU: glfsx_open_ragged_device and
glfsx_open_blobs are declared, bound and exported; the device form checks its
arguments in the documented order before it touches the device; a well-formed
call fails with GLFSX_E_DEVICE when there is none; the Python mirror has
open_blobs and verify_tree, and the older signatures are as they were."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "glfsx.h")
NAMES = ("glfsx_open_ragged_device", "glfsx_open_blobs")
MAX_RAGGED = 16 << 20


def test_declared_bound_and_exported():
    from glfs_amd import _native as N
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (glfsx_[a-z0-9_]+)", out))
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name + " is not declared in include/glfsx.h"
        assert name in N.SIGNATURES
        restype, argtypes = N.SIGNATURES[name]
        assert restype is ctypes.c_int
        assert len(argtypes) == len(m.group(1).split(",")), name
        assert name in exported
    # the declarations are the issue's: parameter names in order
    dev = re.search(r"glfsx_open_ragged_device\s*\(([^)]*)\)", txt).group(1)
    assert re.findall(r"(\w+)\s*(?:,|$)", dev) == [
        "salt", "cid_key", "d_ctext", "d_offsets", "d_lengths", "n", "max_len", "d_refs",
        "d_ptext", "d_status", "stream"]
    host = re.search(r"glfsx_open_blobs\s*\(([^)]*)\)", txt).group(1)
    assert re.findall(r"(\w+)\s*(?:,|$)", host) == [
        "salt", "cid_key", "ctext", "offsets", "lengths", "n", "refs", "ptext", "status_out",
        "n_bad"]


def _call(N, ctext=0x1000, offs=0x2000, lens=0x3000, n=1, max_len=4096, refs=0x4000,
          ptext=None, status=0x5000):
    """glfsx_open_ragged_device with made-up device addresses: every call
    here returns before anything is dereferenced."""
    return N.lib.glfsx_open_ragged_device(bytes(32), None, ctext, offs, lens, n, max_len, refs,
                                          ptext, status, None)


def test_argument_checks_come_first_and_in_order():
    """Null pointers, then alignment, then the length limit, then n == 0 --
    each decided before the device is looked for, so the codes are the same
    with and without a GPU."""
    from glfs_amd import _native as N
    # 1. a null d_ctext, d_refs or d_status: GLFSX_E_ARG, whatever else is wrong
    for kw in ({"ctext": None}, {"refs": None}, {"status": None}):
        assert _call(N, **kw) == N.GLFSX_E_ARG, kw
        assert "null" in N.last_error()
        assert _call(N, max_len=MAX_RAGGED + 1, n=0, **kw) == N.GLFSX_E_ARG, kw
    assert _call(N, ctext=None, refs=0x4001) == N.GLFSX_E_ARG
    assert "null" in N.last_error()
    # 2. misaligned d_refs / d_status: GLFSX_E_ARG before the length limit
    for kw in ({"refs": 0x4001}, {"refs": 0x4002}, {"status": 0x5002}, {"status": 0x5003}):
        assert _call(N, max_len=MAX_RAGGED + 1, n=0, **kw) == N.GLFSX_E_ARG, kw
        assert "aligned" in N.last_error()
    # 3. max_len above 16 MiB: GLFSX_E_UNSUPPORTED, even for n == 0
    assert _call(N, max_len=MAX_RAGGED + 1) == N.GLFSX_E_UNSUPPORTED
    assert _call(N, max_len=MAX_RAGGED + 1, n=0) == N.GLFSX_E_UNSUPPORTED
    assert "ragged open" in N.last_error()
    # 4. n == 0: nothing to do, whatever the arrays are
    assert _call(N, n=0) == 0
    assert _call(N, n=0, max_len=MAX_RAGGED, offs=None, lens=None) == 0
    # the host form: nothing to do for n == 0; a length above the limit is
    # refused before the device is looked for
    bad = ctypes.c_uint64(7)
    assert N.lib.glfsx_open_blobs(None, None, None, None, None, 0, None, None, None,
                                  ctypes.byref(bad)) == 0
    assert bad.value == 0
    one = (ctypes.c_uint64 * 1)
    assert N.lib.glfsx_open_blobs(None, None, b"x", one(0), one(MAX_RAGGED + 1), 1, bytes(64),
                                  None, None, None) == N.GLFSX_E_UNSUPPORTED
    assert N.lib.glfsx_open_blobs(None, None, None, one(0), one(1), 1, bytes(64),
                                  None, None, None) == N.GLFSX_E_ARG


def test_well_formed_calls_need_a_device():
    from glfs_amd import _native as N
    if N.device_count() > 0:
        pytest.skip("GPU present")
    assert _call(N) == N.GLFSX_E_DEVICE
    assert "no HIP device" in N.last_error()
    one = (ctypes.c_uint64 * 1)
    st, bad = (ctypes.c_uint32 * 1)(), ctypes.c_uint64()
    assert N.lib.glfsx_open_blobs(bytes(32), None, b"x" * 64, one(0), one(64), 1, bytes(64),
                                  ctypes.create_string_buffer(64), st,
                                  ctypes.byref(bad)) == N.GLFSX_E_DEVICE
    assert "no HIP device" in N.last_error()


def test_mirror_has_the_new_calls_and_keeps_the_old():
    from glfs_amd import bigblob, glfs

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert params(bigblob.open_blobs) == [("ctexts", E), ("refs", E), ("salt", E),
                                          ("cid_key", None), ("want_ptext", True)]
    assert params(glfs.Machine.verify_tree) == [("self", E), ("store", E), ("ref", E),
                                                ("cid_key", None)]
    assert bigblob.open_blobs([], [], None) == ([], [])  # nothing to do, no device
    # as they were
    assert params(bigblob.open_level) == [("ctexts", E), ("refs", E), ("block_size", E),
                                          ("salt", E), ("cid_key", None), ("want_ptext", True)]
    assert params(glfs.Machine.verify) == [("self", E), ("store", E), ("ref", E)]
    assert params(glfs.Machine.sync) == [("self", E), ("dst", E), ("src", E), ("x", E)]
    assert params(bigblob.Machine.verify) == [("self", E), ("store", E), ("root", E),
                                              ("salt", None), ("cid_key", None)]
    assert params(bigblob.ErrCorrupt.__init__) == [("self", E), ("index", E), ("cid", E),
                                                   ("status", E), ("level", None)]
