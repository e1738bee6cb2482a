"""The one-block verified read's C-ABI (glfsx_open) and the checked read
interface of the Python mirror without a device: the entry point is declared,
bound and exported, its argument checks come before the device is touched in
the documented order, and every new parameter of the mirror is optional.
CPU-only."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "glfsx.h")
NAMES = {"glfsx_open"}
MAX_MSG = 256 * 256 * 64 * 1024       # kMaxMsgLen (glfs_amd/csrc/kernels.h)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_symbol_in_header_binding_and_library():
    from glfs_amd import _native
    declared = set(re.findall(r"\b(glfsx_[a-z0-9_]+)\s*\(", _header()))
    assert NAMES <= declared
    assert NAMES <= set(_native.SIGNATURES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert NAMES <= set(re.findall(r"\bT (glfsx_[a-z0-9_]+)", out))
    # the prototype as the issue states it
    assert re.search(
        r"int\s+glfsx_open\(const uint8_t \*salt, const uint8_t \*cid_key, "
        r"const uint8_t ref\[64\],\s*const void \*ctext, uint64_t n, void \*ptext, "
        r"uint32_t \*status_out\);", _header())
    res, args = _native.SIGNATURES["glfsx_open"]
    assert res is ctypes.c_int and len(args) == 7


def test_argument_checks_come_before_the_device_in_order():
    from glfs_amd import _native as N
    L = N.lib
    salt, ref, ct = bytes(32), bytes(64), bytes(128)
    pt = ctypes.create_string_buffer(128)
    st = ctypes.c_uint32(0x5A5A5A5A)
    # 1. a NULL ref, or bytes announced with no ctext: GLFSX_E_ARG
    assert L.glfsx_open(salt, None, None, ct, 128, pt, ctypes.byref(st)) == N.GLFSX_E_ARG
    assert L.glfsx_open(salt, None, ref, None, 128, pt, ctypes.byref(st)) == N.GLFSX_E_ARG
    # ... and they come first: both wrong at once is still an argument error
    assert L.glfsx_open(salt, None, None, ct, MAX_MSG + 1, pt, None) == N.GLFSX_E_ARG
    assert L.glfsx_open(None, None, ref, None, MAX_MSG + 1, None, None) == N.GLFSX_E_ARG
    # 2. above the kernels' limit: GLFSX_E_UNSUPPORTED (the bytes are not read)
    assert L.glfsx_open(salt, None, ref, ct, MAX_MSG + 1, pt, ctypes.byref(st)) == \
        N.GLFSX_E_UNSUPPORTED
    assert L.glfsx_open(None, None, ref, ct, 1 << 63, None, None) == N.GLFSX_E_UNSUPPORTED
    assert st.value == 0x5A5A5A5A          # a refused call writes no status
    assert pt.raw == bytes(128)


def test_no_device():
    from glfs_amd import _native as N
    if N.device_count():
        return                              # the GPU suite covers the rest
    L = N.lib
    salt, ref, ct = bytes(32), bytes(64), bytes(128)
    pt = ctypes.create_string_buffer(128)
    st = ctypes.c_uint32(0)
    for n, c in ((128, ct), (0, None), (0, ct), (65537, bytes(65537))):
        # a well-formed call gets as far as the device, and no further; n == 0
        # is a real message, not a no-op
        assert L.glfsx_open(salt, None, ref, c, n, pt if n <= 128 else None,
                            ctypes.byref(st)) == N.GLFSX_E_DEVICE
        assert "no HIP device" in N.last_error()
    assert L.glfsx_open(None, None, ref, ct, 128, None, None) == N.GLFSX_E_DEVICE
    from glfs_amd import bigblob
    try:
        bigblob.open_block(ct, bigblob.Ref(bytes(32), bytes(32)), salt)
    except N.DeviceError:
        pass
    else:
        raise AssertionError("open_block without a device must raise DeviceError")


def test_old_signatures_still_accepted_and_new_parameters_optional():
    from glfs_amd import bigblob, glfs, tree
    M, G = bigblob.Machine, glfs.Machine
    old = [
        (M.get_f, ["self", "store", "ref"]),
        (M.get_piece, ["self", "store", "root", "bf", "level", "block_index"]),
        (M.read_at, ["self", "store", "x", "offset", "n"]),
        (M.new_reader, ["self", "store", "root"]),
        (M.traverse, ["self", "store", "root", "enter", "exit"]),
        (M.populate, ["self", "store", "root", "dst"]),
        (bigblob.Reader.__init__, ["self", "machine", "store", "root"]),
        (G.get_typed, ["self", "store", "ty", "x"]),
        (G.get_blob, ["self", "store", "x"]),
        (G.get_blob_bytes, ["self", "store", "x", "max_size"]),
        (G.get_at_path, ["self", "store", "ref", "subpath"]),
        (G.get_tree_slice, ["self", "store", "ref"]),
        (tree.get_tree_slice, ["store", "ref"]),
        (tree.lookup_path, ["store", "ent", "subpath"]),
        (tree.get_at_path, ["store", "ref", "subpath"]),
    ]
    for fn, names in old:
        ps = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in ps[:len(names)]] == names, fn
        # everything behind the old parameters is optional
        assert all(p.default is not inspect.Parameter.empty
                   or p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD) for p in ps[len(names):]), fn
    for fn in (M.get_f, M.get_piece, M.read_at, M.new_reader, M.traverse, M.populate,
               bigblob.Reader.__init__, tree.get_tree_slice, tree.lookup_path, tree.get_at_path):
        ps = inspect.signature(fn).parameters
        assert ps["salt"].default is None and ps["cid_key"].default is None, fn
    ps = inspect.signature(bigblob.open_block).parameters
    assert list(ps) == ["ctext", "ref", "salt", "cid_key", "want_ptext"]
    assert ps["cid_key"].default is None and ps["want_ptext"].default is True
    assert inspect.signature(glfs.with_verify).parameters["cid_key"].default is None


def test_verification_is_off_by_default():
    from glfs_amd import bigblob, glfs
    m = glfs.Machine()
    assert m.verify_reads is False and m.cid_key is None and m._read_kw("blob") == {}
    key = bytes(range(32))
    v = glfs.Machine(glfs.with_verify(key))
    assert v.verify_reads is True and v.cid_key == key
    assert glfs.Machine(glfs.with_verify()).cid_key is None
    # the reference's own option stays dead (machine.go:41-48)
    assert glfs.Machine(glfs.with_salt(b"\x01" * 32)).salt == bytes(32)
    # an unchecked Reader carries no keys; a root of no levels needs no device
    r = bigblob.Machine().new_reader(None, bigblob.Root(bigblob.Ref(bytes(32), bytes(32)), 0, 64))
    assert (r.salt, r.cid_key) == (None, None) and r.read() == b""
    assert bigblob.Machine()._level_salts(None) == (None, None)


def test_err_corrupt_carries_the_level():
    from glfs_amd import bigblob
    e = bigblob.ErrCorrupt(0, bytes(range(32)), 2)
    assert e.level is None
    e2 = e.at_level(3)
    assert (e2.level, e2.cid, e2.status, e2.index) == (3, e.cid, 2, 0)
    assert "level 3" in str(e2) and e.cid.hex() in str(e2)
