"""The verified read (glfsx_open_batch[_device]: k_open and the composed
route) against the oracle: expected refs and ctext are O.post per block of
O.fill_splitmix data, never the library's own write path.  Every case runs
under route 1 (composed) and route 2 (k_open wherever able)."""
import ctypes
import functools

import pytest

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SALT = bytes(range(1, 33))
CID_KEY = bytes(range(101, 133))
# (bs, total): the smallest shapes at which each branch of k_open is live
SHAPES = [
    (MiB, 3 * MiB + 77),              # G=4 fast path, then a ragged generic tail
    (2 * MiB, 2 * MiB + 8192 + 64),   # G=8
    (65536, 2 * 65536 + 8191),        # G=1, 64 lanes, tail ending mid-64-byte block
    (4096, 33 * 4096 + 5),            # four active lanes, tree merge of 4
    (1088, 3 * 1088),                 # two chunks, the second 64 bytes long
    (128, 7 * 128),                   # whole: ROOT inside lane 0
    (8192, 5 * 8192),                 # exact multiple, no short block
    (MiB // 2, MiB + 8191),           # G=2
]
BIG = (8 * MiB, 4 * MiB + 64)         # above the fused limit: composed on both routes
VARIANT_SHAPES = [SHAPES[0], SHAPES[3]]
UNALIGNED_SHAPES = VARIANT_SHAPES + [SHAPES[7]]   # the byte-load k_open at G = 4, 1 and 2
# k_open's chunks per lane at each block size of SHAPES (launch_open)
OPEN_G = {MiB: 4, 2 * MiB: 8, MiB // 2: 2, 65536: 1, 4096: 1, 1088: 1, 128: 1, 8192: 1}
LOG_OPEN, LOG_WORDS = 4, 10           # GLFSX_LOG_OPEN, GLFSX_PASS_LOG_WORDS
POISON = 0x5A5A5A5A                   # the status array is not pre-zeroed


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def _case(bs, total, keyed=False):
    """(data, ctext, refs) of the shape from the oracle, computed once."""
    from oracle import oracle as O
    data = O.fill_splitmix(total, bs * 31 + total)
    refs, cts = [], []
    for o in range(0, total, bs):
        r, c = O.post(SALT, data[o:o + bs], CID_KEY if keyed else None)
        refs.append(r)
        cts.append(c)
    return data, b"".join(cts), b"".join(refs)


def _dev(torch, payload, off=0, pad=64):
    t = torch.zeros(off + len(payload) + pad, dtype=torch.uint8, device="cuda")
    t[off:off + len(payload)].copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
    return t


def _enqueue(N, torch, bs, total, ct, refs, salt=SALT, cid_key=None, off=0, inplace=False,
             no_pt=False):
    """Enqueue one open on the library's stream; returns the tensors."""
    d_ct = _dev(torch, ct, off)
    d_refs = _dev(torch, refs)
    n = -(-total // bs)
    d_st = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    d_pt = None if no_pt else (d_ct if inplace else
                               torch.zeros(off + len(ct) + 64, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    N.check(N.lib.glfsx_open_batch_device(
        salt, cid_key, d_ct.data_ptr() + off, total, bs, d_refs.data_ptr(),
        None if no_pt else d_pt.data_ptr() + off, d_st.data_ptr(), None))
    return d_ct, d_refs, d_st, d_pt


def _collect(torch, res, total, off=0):
    _, _, d_st, d_pt = res
    torch.cuda.synchronize()
    st = [int(x) & 0xFFFFFFFF for x in d_st.cpu().tolist()]
    if d_pt is None:
        return st, None, None
    raw = bytes(d_pt.cpu().numpy().tobytes())
    return st, raw[off:off + total], raw[off + total:off + total + 64]


def _open(N, torch, bs, total, ct, refs, **kw):
    off = kw.get("off", 0)
    return _collect(torch, _enqueue(N, torch, bs, total, ct, refs, **kw), total, off)


def _open_log_reset(N):
    """Empties the launch log (glfsx_debug_pass_log), which is process-wide
    and holds whatever earlier tests launched."""
    N.check(N.lib.glfsx_debug_pass_log(1, None, 0, None))


def _open_log(N):
    """The k_open records of the launch log since _open_log_reset; empties it."""
    buf = (ctypes.c_uint32 * (LOG_WORDS * 64))()
    n = ctypes.c_size_t()
    N.check(N.lib.glfsx_debug_pass_log(1, buf, 64, ctypes.byref(n)))
    assert n.value <= 64
    recs = [tuple(buf[i * LOG_WORDS:(i + 1) * LOG_WORDS]) for i in range(n.value)]
    return [r for r in recs if r[0] == LOG_OPEN]


def _flip(b, at, bit=0):
    x = bytearray(b)
    x[at] ^= 1 << bit
    return bytes(x)


@pytest.fixture(params=[1, 2], ids=["composed", "fused"])
def route(gpu, request):
    gpu.set_open_route(request.param)
    yield request.param
    gpu.set_open_route(0)


@pytest.fixture
def routes(gpu):
    yield gpu.set_open_route
    gpu.set_open_route(0)


# ------------------------------------------------------------------ clean input
@pytest.mark.parametrize("bs,total", SHAPES + [BIG])
def test_clean(gpu, O, route, bs, total):
    torch = _torch()
    data, ct, refs = _case(bs, total)
    _open_log_reset(gpu)
    st, pt, tail = _open(gpu, torch, bs, total, ct, refs)
    log = _open_log(gpu)
    if route == 2 and (bs, total) != BIG:
        # k_open ran, at this block size's G, aligned, one workgroup per block
        n = len(st)
        assert log == [(LOG_OPEN, OPEN_G[bs], 1, 1, 2, 0, n, 0, 0, n)]
    else:
        assert log == []               # the composed route
    assert st == [0] * len(st)
    assert pt == data
    assert tail == bytes(64)           # nothing written past the end


@pytest.mark.parametrize("bs,total", SHAPES + [BIG])
def test_routes_agree(gpu, O, routes, bs, total):
    """Identical status arrays and plaintext from both routes, on clean input
    and on input with a damaged block and a foreign ref."""
    torch = _torch()
    _, ct, refs = _case(bs, total)
    n = -(-total // bs)
    bad_ct = _flip(ct, total - 1, 7)
    bad_refs = _flip(refs, 40, 3) if n > 1 else refs
    got = []
    for r in (1, 2):
        routes(r)
        got.append((_open(gpu, torch, bs, total, ct, refs),
                    _open(gpu, torch, bs, total, bad_ct, bad_refs)))
    assert got[0] == got[1]
    want = [0] * n
    want[0] = 2 if n > 1 else 3
    want[n - 1] = 3
    assert got[0][1][0] == want


# ---------------------------------------------------------------------- variants
@pytest.mark.parametrize("bs,total", VARIANT_SHAPES)
def test_in_place(gpu, O, route, bs, total):
    torch = _torch()
    data, ct, refs = _case(bs, total)
    st, pt, tail = _open(gpu, torch, bs, total, ct, refs, inplace=True)
    assert st == [0] * len(st) and pt == data and tail == bytes(64)


@pytest.mark.parametrize("bs,total", UNALIGNED_SHAPES)
def test_unaligned_pointers(gpu, O, route, bs, total):
    torch = _torch()
    data, ct, refs = _case(bs, total)
    d_ct, d_refs, d_st, d_pt = res = _enqueue(gpu, torch, bs, total, ct, refs, off=1)
    st, pt, tail = _collect(torch, res, total, off=1)
    assert st == [0] * len(st) and pt == data and tail == bytes(64)
    assert int(d_pt[0]) == 0           # nor before the start


@pytest.mark.parametrize("bs,total", VARIANT_SHAPES)
def test_keyed_cid(gpu, O, route, bs, total):
    torch = _torch()
    data, ct, refs = _case(bs, total, True)
    st, pt, _ = _open(gpu, torch, bs, total, ct, refs, cid_key=CID_KEY)
    assert st == [0] * len(st) and pt == data
    # the unkeyed hash of the same bytes is another CID; the DEK still matches
    st, pt, _ = _open(gpu, torch, bs, total, ct, refs)
    assert st == [1] * len(st) and pt == data


@pytest.mark.parametrize("bs,total", VARIANT_SHAPES)
def test_no_plaintext(gpu, O, route, bs, total):
    torch = _torch()
    _, ct, refs = _case(bs, total)
    st, pt, _ = _open(gpu, torch, bs, total, ct, refs, no_pt=True)
    assert pt is None and st == [0] * len(st)
    n = len(st)
    st, _, _ = _open(gpu, torch, bs, total, _flip(ct, bs + 5), _flip(refs, 64 * (n - 1) + 33),
                     no_pt=True)
    want = [0] * n
    want[1], want[n - 1] = 3, 2
    assert st == want


@pytest.mark.parametrize("bs,total", VARIANT_SHAPES)
def test_no_salt(gpu, O, route, bs, total):
    torch = _torch()
    data, ct, refs = _case(bs, total)
    n = -(-total // bs)
    # a foreign DEK goes unnoticed without the salt (and decrypts to garbage);
    # a damaged block still fails its CID
    st, pt, _ = _open(gpu, torch, bs, total, _flip(ct, bs), _flip(refs, 32), salt=None)
    want = [0] * n
    want[1] = 1
    assert st == want
    assert pt[2 * bs:] == data[2 * bs:] and pt[:bs] != data[:bs]


# ------------------------------------------------------------------------ damage
def _lane173(bs):
    g = max(1, bs // (256 * 1024))
    return 173 * g * 1024 + 13


@pytest.mark.parametrize("bs,total", VARIANT_SHAPES + [SHAPES[1]])
def test_damage(gpu, O, route, bs, total):
    """One change at a time; the exact status array is asserted."""
    torch = _torch()
    _, ct, refs = _case(bs, total)
    n = -(-total // bs)

    def status(ct=ct, refs=refs, total=total, **kw):
        return _open(gpu, torch, bs, total, ct, refs, **kw)[0]

    def only(**at):
        want = [0] * n
        for j, v in at.items():
            want[int(j[1:])] = v
        return want

    assert status(ct=_flip(ct, bs)) == only(b1=3)                 # byte 0 of block 1
    if _lane173(bs) < bs:                                         # inside lane 173's chunks
        assert status(ct=_flip(ct, _lane173(bs), 5)) == only(b0=3)
    assert status(ct=_flip(ct, total - 1, 2)) == only(**{f"b{n - 1}": 3})
    assert status(refs=_flip(refs, 64 + 7, 1)) == only(b1=1)      # a ref's CID
    assert status(refs=_flip(refs, 64 + 32 + 31, 7)) == only(b1=2)  # a ref's DEK
    assert status(salt=bytes(32)) == [2] * n                      # the wrong salt
    assert status(total=total - 1) == only(**{f"b{n - 1}": 3})    # a byte short
    if n > 2:
        swapped = ct[bs:2 * bs] + ct[:bs] + ct[2 * bs:]
        assert status(ct=swapped) == only(b0=3, b1=3)


# ----------------------------------------------------------------------- repeats
def test_back_to_back(gpu, O, route):
    """Two launches on one stream over different shapes, no wait between."""
    torch = _torch()
    (bs_a, tot_a), (bs_b, tot_b) = SHAPES[0], SHAPES[3]
    da, ca, ra = _case(bs_a, tot_a)
    db, cb, rb = _case(bs_b, tot_b)
    cb = _flip(cb, 2 * bs_b + 9)
    alone_a = _open(gpu, torch, bs_a, tot_a, ca, ra)
    alone_b = _open(gpu, torch, bs_b, tot_b, cb, rb)
    res_a = _enqueue(gpu, torch, bs_a, tot_a, ca, ra)
    res_b = _enqueue(gpu, torch, bs_b, tot_b, cb, rb)
    res_a2 = _enqueue(gpu, torch, bs_a, tot_a, ca, ra)
    assert _collect(torch, res_a, tot_a) == alone_a
    assert _collect(torch, res_b, tot_b) == alone_b
    assert _collect(torch, res_a2, tot_a) == alone_a
    assert alone_a[1] == da and alone_b[0][2] == 3 and sum(alone_b[0]) == 3


# ------------------------------------------------------------------- auto route
def test_auto_route_at_size(gpu, O, routes):
    """1024 blocks of 1 MiB in HBM, where auto leaves the composed route: the
    same status array and plaintext as either route forced.  Too large for
    the oracle to post whole: the first and the last block's refs are checked
    against it, the rest stand on the write path's own parity tests."""
    torch = _torch()
    N = gpu
    bs, n = MiB, 1024
    total = n * bs - 5
    src = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    ct = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    refs = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib.glfsx_fill_splitmix_device(src.data_ptr(), 0, total, 5, None))
    N.check(N.lib.glfsx_post_batch_device(SALT, src.data_ptr(), total, bs, ct.data_ptr(),
                                          refs.data_ptr(), None, None))
    torch.cuda.synchronize()
    for j in (0, n - 1):
        block = bytes(src[j * bs:min((j + 1) * bs, total)].cpu().numpy().tobytes())
        assert bytes(refs[64 * j:64 * j + 64].cpu().numpy().tobytes()) == O.post(SALT, block)[0]
    ct[700 * bs + 99] ^= 4
    want = torch.zeros(n, dtype=torch.int32, device="cuda")
    want[700] = 3
    got = []
    for r in (0, 1, 2):
        routes(r)
        st = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
        pt = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        N.check(N.lib.glfsx_open_batch_device(SALT, None, ct.data_ptr(), total, bs,
                                              refs.data_ptr(), pt.data_ptr(), st.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(st, want)
        assert torch.equal(pt[:700 * bs], src[:700 * bs])
        assert torch.equal(pt[701 * bs:total], src[701 * bs:total])
        assert not pt[total:].any()
        got.append(pt)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


# --------------------------------------------------------------------- host call
def test_host_call(gpu, O, route):
    """glfsx_open_batch over three 64 MiB slabs, block 70 damaged."""
    N = gpu
    bs, total = MiB, 130 * MiB + 5
    data, ct, refs = _case(bs, total)
    n = -(-total // bs)
    out = ctypes.create_string_buffer(total)
    st = (ctypes.c_uint32 * n)(*([POISON] * n))
    nbad = ctypes.c_uint64(99)
    assert N.lib.glfsx_open_batch(SALT, None, ct, total, bs, refs, out, st, nbad) == 0
    assert nbad.value == 0 and list(st) == [0] * n
    assert out.raw == data
    bad = bytearray(ct)
    bad[70 * bs + 12345] ^= 0x10
    out = ctypes.create_string_buffer(total)
    rc = N.lib.glfsx_open_batch(SALT, None, bytes(bad), total, bs, refs, out, st, nbad)
    assert rc == N.GLFSX_E_CORRUPT
    assert "block 70 " in N.last_error()
    want = [0] * n
    want[70] = 3
    assert nbad.value == 1 and list(st) == want
    got = out.raw
    assert got[:70 * bs] == data[:70 * bs] and got[71 * bs:] == data[71 * bs:]
    # the outputs are optional
    assert N.lib.glfsx_open_batch(SALT, None, bytes(bad), total, bs, refs, None, None,
                                  None) == N.GLFSX_E_CORRUPT
