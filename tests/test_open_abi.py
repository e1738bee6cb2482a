"""The verified read's C-ABI and Python surface without a device: the three
entry points are declared, bound and exported, their argument checks come
before the device is touched, and the mirror's old signatures still hold.
CPU-only."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "glfsx.h")
NAMES = {"glfsx_open_batch_device", "glfsx_open_batch", "glfsx_set_open_route"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_symbols_in_header_binding_and_library():
    from glfs_amd import _native
    declared = set(re.findall(r"\b(glfsx_[a-z0-9_]+)\s*\(", _header()))
    assert NAMES <= declared
    assert NAMES <= set(_native.SIGNATURES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert NAMES <= set(re.findall(r"\bT (glfsx_[a-z0-9_]+)", out))


def test_error_code_and_status_bits():
    from glfs_amd import _native
    txt = _header()
    assert re.search(r"\bGLFSX_E_CORRUPT\s*=\s*-9\b", txt)
    assert re.search(r"#define\s+GLFSX_BAD_CID\s+1u\b", txt)
    assert re.search(r"#define\s+GLFSX_BAD_DEK\s+2u\b", txt)
    assert _native.GLFSX_E_CORRUPT == -9
    assert (_native.GLFSX_BAD_CID, _native.GLFSX_BAD_DEK) == (1, 2)


def test_argument_checks_come_before_the_device():
    from glfs_amd import _native as N
    no_device = N.device_count() == 0
    salt, ct, refs, pt = bytes(32), bytes(128), bytes(128), ctypes.create_string_buffer(128)
    st = (ctypes.c_uint32 * 2)()
    nbad = ctypes.c_uint64(7)
    L = N.lib
    assert L.glfsx_open_batch(salt, None, ct, 128, 64, None, pt, st, nbad) == N.GLFSX_E_ARG
    assert L.glfsx_open_batch(salt, None, ct, 128, 100, refs, pt, st, nbad) == \
        N.GLFSX_E_UNSUPPORTED
    nbad.value = 7
    assert L.glfsx_open_batch(salt, None, ct, 0, 64, refs, pt, st, nbad) == 0
    assert nbad.value == 0
    # the device form: the same order of checks; odd addresses for refs / status
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    assert L.glfsx_open_batch_device(salt, None, a, 128, 64, None, a, a, None) == N.GLFSX_E_ARG
    assert L.glfsx_open_batch_device(salt, None, a, 128, 64, a + 1, a, a, None) == N.GLFSX_E_ARG
    assert L.glfsx_open_batch_device(salt, None, a, 128, 64, a, a, a + 2, None) == N.GLFSX_E_ARG
    assert L.glfsx_open_batch_device(salt, None, a, 128, 100, a, a, a, None) == \
        N.GLFSX_E_UNSUPPORTED
    assert L.glfsx_open_batch_device(salt, None, a, 0, 64, a, a, a, None) == 0
    if no_device:   # a well-formed call gets as far as the device, and no further
        assert L.glfsx_open_batch(salt, None, ct, 128, 64, refs, pt, st, nbad) == \
            N.GLFSX_E_DEVICE
        assert "no HIP device" in N.last_error()
        assert L.glfsx_open_batch_device(salt, None, a, 128, 64, a, a, a, None) == \
            N.GLFSX_E_DEVICE
        assert "no HIP device" in N.last_error()


def test_set_open_route_hook():
    from glfs_amd import _native as N
    first = N.set_open_route(1)
    try:
        assert first in (0, 1, 2)
        assert N.set_open_route(2) == 1
        assert N.set_open_route(3) == 2      # ignored ...
        assert N.set_open_route(-1) == 2     # ... and so is this
        assert N.set_open_route(0) == 2
        assert N.set_open_route(0) == 0
    finally:
        N.set_open_route(first)
    assert N.set_open_route(first) == first


def test_err_corrupt_fields():
    from glfs_amd import _native as N, bigblob
    cid = bytes(range(32))
    e = bigblob.ErrCorrupt(5, cid, 3, level=2)
    assert isinstance(e, N.GlfsxError) and e.code == N.GLFSX_E_CORRUPT
    assert (e.index, e.cid, e.status, e.level) == (5, cid, 3, 2)
    assert cid.hex() in str(e)
    assert bigblob.ErrCorrupt(0, cid, 1).level is None


def test_old_signatures_still_accepted():
    from glfs_amd import bigblob, glfs
    for fn, old in ((bigblob.read_all, ["store", "root"]), (bigblob._tree_levels, ["get", "root"]),
                    (bigblob.Machine.sync, ["self", "dst", "src", "x", "fn"])):
        ps = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in ps[:len(old)]] == old
        # everything new is optional: the old calls mean what they meant
        assert all(p.default is not inspect.Parameter.empty for p in ps[len(old):])
    # nothing to walk: a one-block root needs no device for its levels
    root = bigblob.Root(bigblob.Ref(bytes(32), bytes(32)), 10, 1024)
    assert bigblob._tree_levels(lambda cid: b"", root) == [[root.ref]]
    assert bigblob.read_all(None, bigblob.Root(root.ref, 0, 1024)) == b""
    assert callable(bigblob.Machine.verify) and callable(glfs.Machine.verify)
    assert callable(bigblob.open_level)
