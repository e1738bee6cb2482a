"""glfsx_tree_decode_device (k_td_count / k_td_index / k_td_parse /
k_td_write) against the host decoder glfsx_tree_decode: every column, every
status word and the counts, with guard bytes around every output; then the
decoded columns as the inputs of the verified read, and get_tree_slice /
verify_tree over the native path."""
import ctypes
import random

import numpy as np
import pytest

import tree_decode_corpus as C

pytestmark = pytest.mark.gpu

GUARD = 64
K_TREE_WG = 256       # kernels.h kTreeWG: lines per parse workgroup
K_TD_SPAN = 16 * 1024  # kernels.h kTdSpan: bytes per count / index workgroup
K_IMG = 60 * 1024     # tree_kernels.hip kImg: the LDS image


class _Out:
    """A device output of nbytes with GUARD bytes of 0xA5 either side (and
    `shift` more in front)."""

    def __init__(self, torch, nbytes, shift=0):
        self.t = torch.full((GUARD + shift + nbytes + GUARD,), 0xA5, dtype=torch.uint8,
                            device="cuda")
        self.lo, self.n = GUARD + shift, nbytes
        self.ptr = self.t.data_ptr() + self.lo

    def host(self, dtype=np.uint8):
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == 0xA5).all() and (h[self.lo + self.n:] == 0xA5).all(), "guard"
        return h[self.lo:self.lo + self.n].copy().view(dtype)

    def untouched(self):
        return bool((self.t == 0xA5).all())


def _place(torch, data: bytes, shift=0, at_end=False):
    """data in HBM `shift` bytes past a 16-byte boundary; at_end: its last
    byte is the last byte of the tensor (a 512-byte multiple, the
    allocator's granule), so a read past the input leaves the tensor."""
    if at_end:
        size = -(-(len(data) + 16) // 512) * 512
        shift = size - len(data)
    else:
        size = shift + len(data) + 32
    t = torch.full((size,), 0x0A, dtype=torch.uint8, device="cuda")  # newlines around it
    if data:
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


def _decode_device(torch, N, ptr, length, want, roots_shift=0, caps=None):
    """One full call with outputs sized by `want` (the host decoder's
    columns; caps = (names_cap, types_cap, n_cap) overrides the capacities).
    Returns (rc, counts, outputs)."""
    n, nl, tl = want.n, len(want.names), len(want.types)
    o = dict(names=_Out(torch, nl), name_offs=_Out(torch, 8 * (n + 1)), modes=_Out(torch, 4 * n),
             types=_Out(torch, tl), type_offs=_Out(torch, 8 * (n + 1)),
             roots=_Out(torch, 64 * n, roots_shift), sizes=_Out(torch, 8 * n),
             block_sizes=_Out(torch, 8 * n), status=_Out(torch, 4 * n))
    ncap, tcap, lcap = caps or (nl, tl, n)
    counts = (ctypes.c_uint64 * 5)()
    torch.cuda.synchronize()
    rc = N.lib.glfsx_tree_decode_device(ptr, length, o["names"].ptr, ncap, o["name_offs"].ptr,
                                        o["modes"].ptr, o["types"].ptr, tcap, o["type_offs"].ptr,
                                        o["roots"].ptr, o["sizes"].ptr, o["block_sizes"].ptr,
                                        o["status"].ptr, lcap, counts, None)
    torch.cuda.synchronize()
    return rc, list(counts), o


def _check_equal(torch, N, data, ptr, want, roots_shift=0):
    rc, counts, o = _decode_device(torch, N, ptr, len(data), want, roots_shift)
    assert rc == 0, N.last_error()
    assert counts == [want.n, len(want.names), len(want.types), want.n_bad, int(want.tail)]
    for k, dt in (("names", np.uint8), ("name_offs", np.uint64), ("modes", np.uint32),
                  ("types", np.uint8), ("type_offs", np.uint64), ("roots", np.uint8),
                  ("sizes", np.uint64), ("block_sizes", np.uint64), ("status", np.uint32)):
        got = o[k].host(dt)
        assert np.array_equal(got, getattr(want, k)), k


def _counts_only(N, ptr, length, n_cap):
    counts = (ctypes.c_uint64 * 5)()
    rc = N.lib.glfsx_tree_decode_device(ptr, length, None, 0, None, None, None, 0, None, None,
                                        None, None, None, n_cap, counts, None)
    return rc, list(counts)


@pytest.fixture(scope="module")
def mixed():
    """The 3,000-entry mixed pool of test_tree_encode_device_vs_host (every
    escaping class, names of 300-2,000 bytes that force the global-byte
    path), in tree order; its lines and the host decoder's columns."""
    from glfs_amd import tree as T
    ents = C.positive_entries(3000, seed=17, long_names=True)
    data, _ = T.encode_lines(ents)
    want = T.decode_lines(data)
    assert want.n == len(ents) and want.n_bad == 0
    assert max(len(T.go_bytes(e.name)) for e in ents) > 300
    return data, want


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_device_equals_host_input_shifts(gpu, mixed, shift):
    import torch
    data, want = mixed
    t, ptr = _place(torch, data, shift)
    _check_equal(torch, gpu, data, ptr, want)


@pytest.mark.parametrize("roots_shift", [1, 4, 8])
def test_device_equals_host_roots_shifts(gpu, mixed, roots_shift):
    import torch
    data, want = mixed
    t, ptr = _place(torch, data, 3)
    _check_equal(torch, gpu, data, ptr, want, roots_shift)


def test_too_small_capacity_writes_nothing(gpu, mixed):
    import torch
    data, want = mixed
    t, ptr = _place(torch, data, 5)
    n, nl, tl = want.n, len(want.names), len(want.types)
    for caps in ((nl - 1, tl, n), (nl, tl - 1, n), (nl, tl, n - 1)):
        rc, counts, o = _decode_device(torch, gpu, ptr, len(data), want, caps=caps)
        assert rc == gpu.GLFSX_E_ARG, caps
        assert counts[0] == n and counts[4] == 0
        if caps[2] == n:  # the index held the lines: every needed count
            assert counts[:3] == [n, nl, tl]
        for k, out in o.items():
            assert out.untouched(), (caps, k)
    # counts only; and an index too small for the lines
    assert _counts_only(gpu, ptr, len(data), n) == (0, [n, nl, tl, 0, 0])
    assert _counts_only(gpu, ptr, len(data), 1 << 62) == (0, [n, nl, tl, 0, 0])
    rc, counts = _counts_only(gpu, ptr, len(data), n - 1)
    assert rc == gpu.GLFSX_E_ARG and counts == [n, 0, 0, 0, 0]
    rc, counts = _counts_only(gpu, ptr, len(data), 0)
    assert rc == gpu.GLFSX_E_ARG and counts[0] == n


def _numbered(n, name_len=7, pad=0):
    """n canonical lines with "%0<name_len>d" names, from arrays."""
    from glfs_amd import _native as N
    names = np.frombuffer(b"".join(b"%0*d" % (name_len, i) for i in range(n)), dtype=np.uint8)
    no = np.arange(n + 1, dtype=np.uint64) * name_len
    types = np.frombuffer(b"blob" * n, dtype=np.uint8)
    to = np.arange(n + 1, dtype=np.uint64) * 4
    modes = np.full(n, 0o644, dtype=np.uint32)
    rng = np.random.default_rng(n)
    roots = rng.integers(0, 256, 64 * n, dtype=np.uint8)
    sizes = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    bss = np.full(n, 2 << 20, dtype=np.uint64)
    total = ctypes.c_uint64()
    p = lambda a: a.ctypes.data
    N.check(N.lib.glfsx_tree_encode(n, p(names), p(no), p(modes), p(types), p(to), p(roots),
                                    p(sizes), p(bss), None, 0, ctypes.byref(total), None))
    out = np.empty(total.value, dtype=np.uint8)
    N.check(N.lib.glfsx_tree_encode(n, p(names), p(no), p(modes), p(types), p(to), p(roots),
                                    p(sizes), p(bss), p(out), total.value, ctypes.byref(total),
                                    None))
    return out.tobytes()


@pytest.mark.parametrize("n", [1, K_TREE_WG - 1, K_TREE_WG, K_TREE_WG + 1])
def test_line_counts_at_workgroup_edges(gpu, n):
    import torch
    from glfs_amd import tree as T
    data = _numbered(n)
    t, ptr = _place(torch, data, 9)
    _check_equal(torch, gpu, data, ptr, T.decode_lines(data))


def test_empty_input_and_tail_only(gpu):
    import torch
    from glfs_amd import tree as T
    t, ptr = _place(torch, b"", 0)
    _check_equal(torch, gpu, b"", ptr, T.decode_lines(b""))
    no = _Out(torch, 8)
    counts = (ctypes.c_uint64 * 5)(9, 9, 9, 9, 9)
    assert gpu.lib.glfsx_tree_decode_device(None, 0, None, 0, no.ptr, None, None, 0, None, None,
                                            None, None, None, 0, counts, None) == 0
    assert list(counts) == [0] * 5 and no.host(np.uint64).tolist() == [0]
    data = C.line()[:-1]  # no newline: a tail, no line
    t, ptr = _place(torch, data, 2)
    want = T.decode_lines(data)
    assert (want.n, want.n_bad, want.tail) == (0, 1, True)
    _check_equal(torch, gpu, data, ptr, want)
    # more lines than canonical ones could be: decode_lines_device sizes its index again
    t, ptr = _place(torch, b"\n" * 1000, 1)
    c = T.decode_lines_device(ptr, 1000)
    assert (c.n, c.n_bad, c.tail) == (1000, 1000, False)
    assert c.status.cpu().tolist() == [1] * 1000 and c.name_offs.cpu().tolist() == [0] * 1001


def test_lines_against_span_edges(gpu):
    """A line longer than a count-pass span (a span without a newline, and a
    workgroup past the LDS image), a line whose newline is a span's last
    byte and one whose newline is its first, for inputs at shift 0 and 5
    (spans are cut from the 16-byte boundary below the input)."""
    import torch
    from glfs_amd import tree as T
    head = _numbered(300, 9)   # a workgroup on the LDS path before the long lines
    for shift in (0, 5):
        base = shift + len(head)
        first = C.line(name='"a"')
        # the second line's newline is a span's last byte
        pad = -(base + len(first) + len(C.line(name='"b"'))) % K_TD_SPAN
        second = C.line(name='"b' + "x" * pad + '"')
        assert (base + len(first) + len(second)) % K_TD_SPAN == 0
        # the third covers four whole spans; its newline is a span's first byte
        pad = 4 * K_TD_SPAN + 1 - len(C.line(name='"c"'))
        third = C.line(name='"c' + "y" * pad + '"')
        assert (base + len(first) + len(second) + len(third) - 1) % K_TD_SPAN == 0
        assert len(third) > 2 * K_TD_SPAN and len(third) > K_IMG
        data = head + first + second + third + C.line(name='"d"')
        want = T.decode_lines(data)
        assert want.n == 304 and want.n_bad == 0
        t, ptr = _place(torch, data, shift)
        _check_equal(torch, gpu, data, ptr, want)


def test_more_spans_than_one_prefix_chunk(gpu):
    """k_tree_prefix scans 1,024 words a chunk: the smallest n of config-4
    lines that gives the count pass more than 1,024 spans, so that the span
    prefix, and with it every line's index, crosses a chunk."""
    import torch
    from glfs_amd import tree as T
    n = 70_000  # ~245 bytes a line: 1,024 spans end near line 68,550
    data = _numbered(n)
    assert (len(data) + K_TD_SPAN - 1) // K_TD_SPAN > 1024
    assert (n + K_TREE_WG - 1) // K_TREE_WG < 1024
    want = T.decode_lines(data)
    assert want.n == n and want.n_bad == 0
    t, ptr = _place(torch, data, 0)
    _check_equal(torch, gpu, data, ptr, want)


def test_negative_corpus_statuses_equal_host(gpu):
    """The negative corpus in one buffer, every input between canonical
    lines, the buffer at the end of its tensor: line for line the host
    decoder's statuses (and columns)."""
    import torch
    from glfs_amd import tree as T
    parts, k = [], 0
    for strict, x in C.negative_corpus():
        parts.append(C.line(name='"k%05d"' % k))
        parts.append(x)
        k += 1
    parts.append(C.line(name='"zz"'))
    parts.append(C.line()[:40])  # a tail
    data = b"".join(parts)
    want = T.decode_lines(data)
    bad = int((want.status & 1 != 0).sum())
    assert want.tail and bad > 1000 and want.n - bad > 1000
    assert (want.status & 2).any()   # ORDER where a substitution left a canonical line
    t, ptr = _place(torch, data, at_end=True)
    _check_equal(torch, gpu, data, ptr, want)
    c = T.decode_lines_device(ptr, len(data))
    assert c.n == want.n and c.n_bad == want.n_bad and c.tail
    assert np.array_equal(c.status.cpu().numpy().view(np.uint32), want.status)


def test_decoded_columns_feed_the_verified_read(gpu, O):
    """Config 4's read side at small size, device-resident: 600 blobs of
    1..40,000 bytes -> glfsx_post_tree_device -> glfsx_tree_decode_device over
    its lines -> glfsx_open_ragged_device with the decoded roots and sizes."""
    import torch
    from glfs_amd import tree as T
    N = gpu
    n, MIB = 600, 1 << 20
    rng = random.Random(600)
    lens_h = [rng.choice([1, 63, 100, 1024, 4096, 5000, 16384, 40000, rng.randrange(1, 40001)])
              for _ in range(n)]
    offs_h, o = [], 0
    for ln in lens_h:
        offs_h.append(o)
        o += ln + rng.randrange(3)
    data = torch.empty(o + 64, dtype=torch.uint8, device="cuda")
    N.check(N.lib.glfsx_fill_splitmix_device(data.data_ptr(), 0, o + 8 - o % 8, n, None))
    names = [(b"n%06d" % i) + rng.choice([b"", b"\"", b"<&>", "é".encode()]) for i in range(n)]
    types = [rng.choice([b"blob", b"tree"]) for _ in range(n)]
    modes = [rng.choice([0o644, 0o755, 0o40000]) for _ in range(n)]
    nb, tb = b"".join(names), b"".join(types)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dn, dt = cuda(np.frombuffer(nb, dtype=np.uint8).copy()), cuda(np.frombuffer(tb, dtype=np.uint8).copy())
    dno = cuda(np.cumsum([0] + [len(x) for x in names]).astype(np.int64))
    dto = cuda(np.cumsum([0] + [len(x) for x in types]).astype(np.int64))
    dm = cuda(np.array(modes, dtype=np.int32))
    dbs = cuda(np.full(n, 2 * MIB, dtype=np.int64))
    offs, lens = cuda(np.array(offs_h, dtype=np.int64)), cuda(np.array(lens_h, dtype=np.int64))
    bsalt, tsalt = O.derive_key(bytes(32), b"blob"), O.derive_key(bytes(32), b"tree")
    cap = 400 * n
    roots = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    ctext = torch.zeros_like(data)
    lines = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    r, total = N.glfsx_root(), ctypes.c_uint64()
    N.check(N.lib.glfsx_post_tree_device(n, 2 * MIB, bsalt, tsalt, None, data.data_ptr(),
                                         offs.data_ptr(), lens.data_ptr(), 40000,
                                         ctext.data_ptr(), roots.data_ptr(), dn.data_ptr(),
                                         dno.data_ptr(), dm.data_ptr(), dt.data_ptr(),
                                         dto.data_ptr(), dbs.data_ptr(), 2 * MIB,
                                         lines.data_ptr(), cap, None, ctypes.byref(r),
                                         ctypes.byref(total), None))
    torch.cuda.synchronize()
    c = T.decode_lines_device(lines.data_ptr(), total.value)
    torch.cuda.synchronize()
    assert (c.n, c.n_bad, c.tail) == (n, 0, False)
    assert not bool(c.status.any())
    assert torch.equal(c.roots, roots) and torch.equal(c.sizes, lens)
    assert torch.equal(c.names, dn) and torch.equal(c.name_offs, dno)
    assert torch.equal(c.types, dt) and torch.equal(c.type_offs, dto)
    assert torch.equal(c.modes, dm) and torch.equal(c.block_sizes, dbs)
    raw = O.derive_key(bsalt, b"raw")

    def open_all(ct):
        st = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        pt = torch.zeros_like(ct)
        N.check(N.lib.glfsx_open_ragged_device(raw, None, ct.data_ptr(), offs.data_ptr(),
                                               c.sizes.data_ptr(), n, 40000, c.roots.data_ptr(),
                                               pt.data_ptr(), st.data_ptr(), None))
        torch.cuda.synchronize()
        return st.cpu().tolist(), pt

    st, pt = open_all(ctext)
    assert st == [0] * n
    for i in (0, 1, n // 2, n - 1):
        assert torch.equal(pt[offs_h[i]:offs_h[i] + lens_h[i]],
                           data[offs_h[i]:offs_h[i] + lens_h[i]])
    mask = torch.zeros(data.numel(), dtype=torch.bool, device="cuda")
    for a, ln in zip(offs_h, lens_h):
        mask[a:a + ln] = True
    assert torch.equal(pt[mask], data[mask])        # every plaintext byte
    victim = 311
    bad = ctext.clone()
    bad[offs_h[victim] + lens_h[victim] // 2] ^= 1
    st, _ = open_all(bad)
    assert [i for i, s in enumerate(st) if s] == [victim]


def test_get_tree_slice_and_verify_tree_native(gpu, monkeypatch):
    """A flat tree of 5,000 one-block files through post_blobs + post_tree_map:
    get_tree_slice and verify_tree over the native decoder (the Python loop
    patched to raise) give what the Python loop gives."""
    from glfs_amd import bigblob, glfs, tree as T
    s = bigblob.MemStore(2 << 20)
    m = glfs.Machine()
    rng = random.Random(5)
    blobs = [rng.randbytes(rng.randrange(1, 300)) for _ in range(5000)]
    refs = m.post_blobs(s, blobs)
    tref = m.post_tree_map(s, {"f%05d<&>" % i: r for i, r in enumerate(refs)})
    with monkeypatch.context() as mp:   # the Python loop, as before
        mp.setattr(T, "read_tree_bytes", T.read_tree_bytes_py)
        want = m.get_tree_slice(s, tref)
        want_blocks = m.verify_tree(s, tref)
    assert len(want) == 5000 and [e.ref for e in want] == refs

    def boom(*a, **k):
        raise AssertionError("fell back to the Python decoder")
    monkeypatch.setattr(T, "read_tree_bytes_py", boom)
    assert m.get_tree_slice(s, tref) == want
    assert m.verify_tree(s, tref) == want_blocks
