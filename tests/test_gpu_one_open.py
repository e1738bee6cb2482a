"""glfsx_open -- the verified read of one block from host memory: k_one_open
(one launch, CID and DEK trees side by side) up to 64 KiB, device staging
above -- against the oracle: expected refs and ctext are O.post of
O.fill_splitmix data, never the library's own write path.  Every case runs
under route 1 (every size through device staging) and route 2 (the one-shot
kernel up to 64 KiB), and the two must agree."""
import ctypes
import functools
import threading

import pytest

from test_gpu_small_decrypt_matrix import (MED, ONE, ONE_FAMILIES, ONE_OPEN, aux_key,
                                           aux_kernel_table, aux_reset, aux_take, one_expect)

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SALT = bytes(range(1, 33))
CID_KEY = bytes(range(101, 133))
OTHER = bytes(range(201, 233))
POISON = 0x5A5A5A5A                   # the status word is not pre-zeroed
GUARD = bytes([0xA5]) * 64            # behind the plaintext: stays as it is
# every boundary of block (64), chunk (1024), wave (16 chunks of four lanes)
# and QUADS instantiation (16 KiB), and trees with an odd pass-through
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 4096, 4097, 16383, 16384,
           16385, 32775, 65535, 65536]
STAGED = [65537, 131073, MiB, 2 * MiB + 5]
DAMAGE = [1, 64, 1025, 4096, 16385, 65536]


@functools.lru_cache(maxsize=None)
def _msg(n, keyed=False, seed=0):
    """(data, ref, ctext) of an n-byte message from the oracle, computed once."""
    from oracle import oracle as O
    data = O.fill_splitmix(n, 7 * n + 1 + seed)
    ref, ct = O.post(SALT, data, CID_KEY if keyed else None)
    return data, ref, ct


def _flip(b, at, bit=0):
    x = bytearray(b)
    x[at] ^= 1 << bit
    return bytes(x)


def _call(N, ct, ref, salt, cid_key, want=True, inplace=False, off=0):
    """One glfsx_open; returns (rc, status, plaintext or None, guard, error text).
    off: the caller's ctext, plaintext and ref start that many bytes into
    16-byte aligned buffers."""
    n = len(ct)
    cbuf = ctypes.create_string_buffer(off + n + 64)
    ctypes.memmove(ctypes.addressof(cbuf) + off, ct + GUARD, n + 64)
    rbuf = ctypes.create_string_buffer(off + 64)
    ctypes.memmove(ctypes.addressof(rbuf) + off, ref, 64)
    pbuf = cbuf if inplace else ctypes.create_string_buffer(off + n + 64)
    if not inplace:
        ctypes.memmove(ctypes.addressof(pbuf) + n + off, GUARD, 64)
    st = ctypes.c_uint32(POISON)
    rc = N.lib.glfsx_open(salt, cid_key, ctypes.addressof(rbuf) + off,
                          ctypes.addressof(cbuf) + off, n,
                          ctypes.addressof(pbuf) + off if want else None, ctypes.byref(st))
    err = N.last_error() if rc else ""
    raw = pbuf.raw
    return rc, st.value, (raw[off:off + n] if want else None), raw[off + n:off + n + 64], err


def _both(N, *a, **kw):
    """The call under route 1 and under route 2: identical results.  Route 2
    up to 64 KiB is one k_one_open_v launch, which the aux log must show."""
    out = []
    try:
        for route in (1, 2):
            N.set_open_route(route)
            aux_reset(N)
            out.append(_call(N, *a, **kw))
            log = aux_take(N, families=ONE_FAMILIES)
            n, salted = len(a[0]), a[2] is not None
            assert log == ([one_expect(ONE_OPEN, 1, n, salted)] if route == 2 and n <= 65536
                           else []), (route, n, salted, log)
    finally:
        N.set_open_route(0)
    assert out[0][:4] == out[1][:4], "the staged route and the one-shot kernel disagree"
    return out[1]


def _bad(N, res, ref, status):
    rc, st, _, guard, err = res
    assert rc == N.GLFSX_E_CORRUPT and st == status
    assert ref[:32].hex() in err
    assert guard == GUARD


# ------------------------------------------------------------------ clean input
@pytest.mark.parametrize("n", LENGTHS + STAGED)
def test_clean(gpu, O, n):
    for keyed in (False, True):
        data, ref, ct = _msg(n, keyed)
        for salt in (SALT, None):
            # (route 2, n <= 64 KiB: _both has seen k_one_open_v<16 up to 16 KiB
            # else 64, salted or not> in the aux log)
            rc, st, pt, guard, _ = _both(gpu, ct, ref, salt, CID_KEY if keyed else None)
            assert (rc, st) == (0, 0), (n, keyed, salt is not None)   # the poison is gone
            assert pt == data
            assert guard == GUARD                                      # nothing past the end


def test_auto_route_is_the_one_shot_kernel(gpu, O):
    """Route 0 up to 64 KiB: launches of the coalescing poster, not staging."""
    out = (ctypes.c_uint64 * 3)()
    gpu.set_open_route(0)
    gpu.lib.glfsx_one_stats(1, out)
    for n in (0, 4096, 65536):
        data, ref, ct = _msg(n)
        rc, st, pt, _, _ = _call(gpu, ct, ref, SALT, None)
        assert (rc, st, pt) == (0, 0, data)
    gpu.lib.glfsx_one_stats(1, out)
    assert (out[0], out[1]) == (3, 3)
    data, ref, ct = _msg(65537)
    assert _call(gpu, ct, ref, SALT, None)[:3] == (0, 0, data)
    gpu.lib.glfsx_one_stats(0, out)
    assert out[0] == 0                  # above 64 KiB: the staged route


# ---------------------------------------------------------------------- damage
@pytest.mark.parametrize("n", DAMAGE)
def test_damaged_ctext(gpu, O, n):
    """A bit flipped in the first, a middle-chunk and the last ctext byte:
    neither the CID nor the DEK matches."""
    data, ref, ct = _msg(n)
    for at in sorted({0, (n // 2048) * 1024 + min(n - 1, 517) if n > 1024 else n // 2, n - 1}):
        res = _both(gpu, _flip(ct, at, at % 8), ref, SALT, None)
        _bad(gpu, res, ref, 3)
        assert res[2] != data and len(res[2]) == n   # written all the same


@pytest.mark.parametrize("n", DAMAGE)
def test_damaged_ref_and_wrong_keys(gpu, O, n):
    data, ref, ct = _msg(n)
    kdata, kref, kct = _msg(n, True)
    # the ref's CID: status 1 exactly, the plaintext still the data
    bad = _flip(ref, 9, 3)
    res = _both(gpu, ct, bad, SALT, None)
    _bad(gpu, res, bad, 1)
    assert res[2] == data
    # the ref's DEK: status 2 exactly (the ciphertext is the one posted)
    bad = _flip(ref, 32 + 21, 6)
    _bad(gpu, _both(gpu, ct, bad, SALT, None), bad, 2)
    # ... and without a salt nobody looks at the DEK
    rc, st, _, _, _ = _both(gpu, ct, bad, None, None)
    assert (rc, st) == (0, 0)
    # the wrong salt: 2, the plaintext still the data
    res = _both(gpu, ct, ref, OTHER, None)
    _bad(gpu, res, ref, 2)
    assert res[2] == data
    # the wrong CID key, a key where none was used, none where one was: 1
    for c, r, key, want in ((kct, kref, OTHER, kdata), (ct, ref, CID_KEY, data),
                            (kct, kref, None, kdata)):
        res = _both(gpu, c, r, SALT, key)
        _bad(gpu, res, r, 1)
        assert res[2] == want
    # CID only, damaged bytes: bit 1 is never set without a salt
    _bad(gpu, _both(gpu, _flip(ct, n - 1), ref, None, None), ref, 1)


# ------------------------------------------------------------ the call's forms
@pytest.mark.parametrize("n", [0, 17, 4097, 65536, 65537])
def test_status_only_in_place_and_odd_addresses(gpu, O, n):
    data, ref, ct = _msg(n, True)
    # ptext == NULL: the status alone
    for salt in (SALT, None):
        rc, st, pt, guard, _ = _both(gpu, ct, ref, salt, CID_KEY, want=False)
        assert (rc, st, pt, guard) == (0, 0, None, GUARD)
    if n:
        _bad(gpu, _both(gpu, _flip(ct, n // 2), ref, SALT, CID_KEY, want=False), ref, 3)
    # ptext == ctext
    rc, st, pt, guard, _ = _both(gpu, ct, ref, SALT, CID_KEY, inplace=True)
    assert (rc, st, pt, guard) == (0, 0, data, GUARD)
    # ctext, ptext and ref at odd addresses
    for off in (1, 7):
        rc, st, pt, guard, _ = _both(gpu, ct, ref, SALT, CID_KEY, off=off)
        assert (rc, st, pt, guard) == (0, 0, data, GUARD)
        rc, st, pt, guard, _ = _both(gpu, ct, ref, SALT, CID_KEY, off=off, inplace=True)
        assert (rc, st, pt, guard) == (0, 0, data, GUARD)
    # status_out == NULL
    pt = ctypes.create_string_buffer(max(n, 1))
    assert gpu.lib.glfsx_open(SALT, CID_KEY, ref, ct, n, pt, None) == 0
    assert pt.raw[:n] == data
    assert gpu.lib.glfsx_open(OTHER, CID_KEY, ref, ct, n, pt, None) == gpu.GLFSX_E_CORRUPT


def test_open_block_mirror(gpu, O):
    from glfs_amd import bigblob
    for n in (0, 1000, 70000):
        data, ref, ct = _msg(n, True)
        r = bigblob.Ref.from_bytes(ref)
        assert bigblob.open_block(ct, r, SALT, CID_KEY) == data
        assert bigblob.open_block(ct, r, None, CID_KEY) == data
        assert bigblob.open_block(ct, r, SALT, CID_KEY, want_ptext=False) == b""
        with pytest.raises(bigblob.ErrCorrupt) as ei:
            bigblob.open_block(ct, r, OTHER, CID_KEY)
        assert (ei.value.index, ei.value.cid, ei.value.status) == (0, r.cid, 2)
        with pytest.raises(bigblob.ErrCorrupt) as ei:
            bigblob.open_block(ct, r, SALT)
        assert ei.value.status == 1


# ------------------------------------------------------------- shared launches
def test_posts_and_opens_share_launches(gpu, O):
    """16 threads, each 50 calls alternating glfsx_post and glfsx_open on
    distinct messages of mixed small sizes: every ref, ciphertext, plaintext
    and status is the oracle's, and the calls went out as launches of the
    coalescing poster.  Every launch logged is in the table of the one-shot
    instantiations and carries at least one request per workgroup class; which
    array-form k_one_open kernels the run reached is printed, not asserted:
    whether two opens coalesce is a matter of thread timing, and no entry
    point opens several blocks in one call."""
    T, K = 16, 50
    sizes = [0, 1, 100, 1024, 4097, 16384, 16385, 20000, 40000, 65536, 333, 8191]
    work = []
    for t in range(T):
        mine = []
        for k in range(K):
            n = sizes[(t * 5 + k * 7) % len(sizes)]
            keyed = (t + k) % 3 == 0
            mine.append((k % 2, keyed, (t + k // 2) % 4 == 0) + _msg(n, keyed, seed=1 + t * K + k))
        work.append(mine)
    out = (ctypes.c_uint64 * 3)()
    errors = []
    start = threading.Barrier(T)

    def run(mine):
        try:
            gpu.set_device(0)
            start.wait()
            for is_open, keyed, unsalted, data, ref, ct in mine:
                n, key = len(data), (CID_KEY if keyed else None)
                if is_open:
                    salt = None if unsalted else SALT
                    pt = ctypes.create_string_buffer(n + 64)
                    st = ctypes.c_uint32(POISON)
                    rc = gpu.lib.glfsx_open(salt, key, ref, ct, n, pt, ctypes.byref(st))
                    assert (rc, st.value) == (0, 0)
                    assert pt.raw[:n] == data and pt.raw[n:] == bytes(64)
                    # and a foreign ref is refused in the same traffic
                    st.value = POISON
                    rc = gpu.lib.glfsx_open(salt, key, _flip(ref, 3), ct, n, pt, ctypes.byref(st))
                    assert (rc, st.value) == (gpu.GLFSX_E_CORRUPT, 1)
                else:
                    got_ref = ctypes.create_string_buffer(64)
                    got_ct = ctypes.create_string_buffer(n + 64)
                    assert gpu.lib.glfsx_post(SALT, data, n, got_ct, got_ref, key) == 0
                    assert got_ref.raw == ref
                    assert got_ct.raw[:n] == ct and got_ct.raw[n:] == bytes(64)
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errors.append(e)
            start.abort()

    gpu.set_open_route(0)
    gpu.lib.glfsx_one_stats(1, out)
    aux_reset(gpu)
    threads = [threading.Thread(target=run, args=(w,)) for w in work]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[0]
    log = aux_take(gpu, cap=4096, families=ONE_FAMILIES)
    table = aux_kernel_table()
    known = set().union(*(keys for keys, _ in table.values()))
    assert log and all(aux_key(r) in known for r in log)
    for r in log:
        # n requests, none above 64 KiB; one goes by value, more as an array
        assert r[0] in (ONE, ONE_OPEN)
        assert r == one_expect(r[0], r[9], r[8], salted=r[2]), r
    reached = sorted(name for name, (keys, _) in table.items()
                     if name.startswith("k_one_open<") and keys & {aux_key(r) for r in log})
    print("array-form k_one_open instantiations reached:", reached or "none")
    gpu.lib.glfsx_one_stats(1, out)
    launches, requests = out[0], out[1]
    # 25 posts and 25 + 25 opens per thread, every one through the poster
    assert requests == T * (K // 2) * 3
    assert 0 < launches <= requests
    assert sum(r[9] for r in log) == requests and len(log) >= launches
