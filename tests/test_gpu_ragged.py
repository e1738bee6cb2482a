"""The ragged post: glfsx_post_ragged_device over batches of messages of
unequal length, and the two routes that use its kernels (glfsx_post_blobs_device
and glfsx_post_blobs for single-block blobs above 16 KiB).  Every ref and
every ciphertext byte is compared with the oracle's post (ref.go:98-161);
nothing is sampled.  The device ciphertext buffer starts at zero and is
compared whole, so a store outside a message's own bytes shows up too."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_small_decrypt_matrix import (POST_CID, POST_DEK, RAG_CHUNK, RAG_FAMILIES,
                                           RAG_MERGE_A, RAG_MERGE_B, aux_reset, aux_take,
                                           latency_wgs_now, rag_expect)

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
MAX_RAGGED = 16 * MIB
SALT = bytes(range(7, 39))
CID_KEY = bytes(range(100, 132))

EDGE_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3073, 5 * KIB, 6 * KIB + 1, 7 * KIB,
             16384, 16385, 17 * KIB + 5, 65535, 65536, 65537, 100 * KIB + 3, 262143, 262144,
             262145, 257 * KIB, 513 * KIB + 700, 1 * MIB, 2 * MIB, 2 * MIB + 1, 5 * MIB + 77]

_cache = {}


def _messages(O, name, lens, seed):
    """The messages of a case (consecutive slices of one splitmix stream) and
    the oracle's (ref, ctext) of each, unkeyed and keyed CID: computed once."""
    if name not in _cache:
        stream = O.fill_splitmix(sum(lens) + 1, seed)
        msgs, o = [], 0
        for ln in lens:
            msgs.append(stream[o:o + ln])
            o += ln
        _cache[name] = (msgs, {})
    return _cache[name]


def _want(O, name, key):
    msgs, posts = _cache[name]
    if key not in posts:
        posts[key] = [O.post(SALT, m, key) for m in msgs]
    return posts[key]


def _offsets(lens, align, phase, gap=0):
    """Message i at the first offset = phase (mod align) at or after the end
    of message i - 1 plus gap."""
    offs, o = [], 0
    for ln in lens:
        o += (phase - o) % align
        offs.append(o)
        o += ln + gap
    return offs, o + 64


def _image(total, offs, pieces):
    img = np.zeros(total, dtype=np.uint8)
    for o, p in zip(offs, pieces):
        img[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return img


def _launch(N, torch, d_data, offs, lens, max_len, ctext, key, stream=None):
    """One call; returns the device tensors (refs, ctext or None) without
    synchronising anything itself."""
    n = len(lens)
    do = torch.tensor(offs, dtype=torch.int64, device="cuda")
    dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
    refs = torch.full((64 * n,), 0xA5, dtype=torch.uint8, device="cuda")
    ct = {"none": None, "inplace": d_data}.get(ctext, None)
    if ctext == "separate":
        ct = torch.zeros_like(d_data)
    torch.cuda.synchronize()
    N.check(N.lib.glfsx_post_ragged_device(
        SALT, key, d_data.data_ptr(), do.data_ptr(), dl.data_ptr(), n, max_len,
        ct.data_ptr() if ct is not None else None, refs.data_ptr(),
        stream.cuda_stream if stream is not None else None))
    return refs, ct, (do, dl)


def _check(torch, refs, ct, offs, want, total):
    torch.cuda.synchronize()
    got = refs.cpu().numpy().tobytes()
    bad = [i for i in range(len(want)) if got[64 * i:64 * i + 64] != want[i][0]]
    assert not bad, ("refs differ", bad[:10], len(bad))
    if ct is not None:
        img = _image(total, offs, [c for _, c in want])
        diff = np.flatnonzero(ct.cpu().numpy() != img)
        assert diff.size == 0, ("ctext differs", diff[:10], diff.size)


def _run(N, O, name, lens, seed, offs, total, ctext="separate", key=None, max_len=None,
         stream=None):
    import torch
    msgs, _ = _messages(O, name, lens, seed)
    d = torch.from_numpy(_image(total, offs, msgs)).cuda()
    refs, ct, _keep = _launch(N, torch, d, offs, lens,
                              max(lens) if max_len is None else max_len, ctext, key, stream)
    _check(torch, refs, ct, offs, _want(O, name, key), total)
    return refs.cpu().numpy().tobytes()


@pytest.fixture
def latency_wgs(gpu):
    prev = []

    def set_(v):
        prev.append(gpu.set_latency_wgs(v))
    yield set_
    if prev:
        gpu.set_latency_wgs(prev[0])


def _edge_order():
    lens = list(EDGE_LENS)
    random.Random(11).shuffle(lens)
    return lens


@pytest.mark.parametrize("thr", [None, 0])
@pytest.mark.parametrize("align,phase", [(64, 0), (64, 16), (2, 1)])
def test_edge_lengths(gpu, O, latency_wgs, align, phase, thr):
    """Chunk counts 1 .. 5121 on both sides of the wave (64), merge-group
    (256) and level-B boundaries, at 64-B aligned, 16-B aligned and odd
    offsets, in the compiler's ARX form (default threshold) and the asm form
    (threshold 0).  The aux log says which k_rag_chunk ran in each pass and
    that both merge levels did."""
    if thr is not None:
        latency_wgs(thr)
    lens = _edge_order()
    offs, total = _offsets(lens, align, phase, gap=3)
    aux_reset(gpu)
    _run(gpu, O, "edge", lens, 21, offs, total)
    log = aux_take(gpu, families=RAG_FAMILIES)
    # the DEK pass, then the CID pass: chunks, level A (a message of more than
    # one chunk), level B (one of more than 256)
    assert max(lens) > 256 * KIB
    assert [(r[0], r[1], r[4]) for r in log] == [
        (family, kind, form if family == RAG_CHUNK else 0)
        for kind in (POST_DEK, POST_CID)
        for form in ((0,) if thr is None else (2,))
        for family in (RAG_CHUNK, RAG_MERGE_A, RAG_MERGE_B)]
    lat = latency_wgs_now(gpu)      # the default, or thr
    assert thr is None or lat == thr
    assert log == rag_expect(lens, POST_DEK, lat) + rag_expect(lens, POST_CID, lat)


def test_keyed_cid_no_ctext_in_place(gpu, O):
    lens = _edge_order()
    offs, total = _offsets(lens, 64, 0, gap=3)
    a = _run(gpu, O, "edge", lens, 21, offs, total, ctext="none", key=CID_KEY)
    b = _run(gpu, O, "edge", lens, 21, offs, total, ctext="inplace", key=CID_KEY)
    c = _run(gpu, O, "edge", lens, 21, offs, total, ctext="separate", key=CID_KEY)
    assert a == b == c
    u = _run(gpu, O, "edge", lens, 21, offs, total, ctext="inplace")
    assert u == _run(gpu, O, "edge", lens, 21, offs, total, ctext="none")
    assert u != a


def _many():
    lens = [i % 1025 for i in range(70001)]
    lens[35000] = 300 * KIB
    return lens


def test_many_messages(gpu, O):
    """70 001 messages: the plan's second level (274 plan workgroups), tiles
    mixing hundreds of messages, one message that starts inside a tile and
    spans 300 of them."""
    lens = _many()
    offs, total = _offsets(lens, 1, 0)
    _run(gpu, O, "many", lens, 22, offs, total)


def test_dense_against_scattered(gpu, O):
    """317 blobs of exactly 64 KiB back to back (every wave holds 64 full
    chunks of one blob) and the same blobs at permuted 16-B aligned offsets."""
    lens = [64 * KIB] * 317
    dense, total = _offsets(lens, 1, 0)
    a = _run(gpu, O, "dense", lens, 23, dense, total)
    slots, stotal = _offsets(lens, 64, 16, gap=5)
    perm = list(range(len(lens)))
    random.Random(12).shuffle(perm)
    scattered = [slots[perm[i]] for i in range(len(lens))]
    b = _run(gpu, O, "dense", lens, 23, scattered, stotal)
    assert a == b


def test_the_limit(gpu, O):
    import torch
    lens = [MAX_RAGGED]
    offs, total = _offsets(lens, 64, 0)
    alone = _run(gpu, O, "limit1", lens, 24, offs, total)
    lens = [1 + 10 * i for i in range(50)] + [MAX_RAGGED] + [1024 - i for i in range(50)]
    offs, total = _offsets(lens, 16, 0)
    msgs, _ = _messages(O, "limit101", lens, 25)
    msgs[50] = _cache["limit1"][0][0]  # the same 16 MiB message
    among = _run(gpu, O, "limit101", lens, 25, offs, total)
    assert among[64 * 50:64 * 51] == alone
    # one byte more: refused before any launch
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    refs = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = gpu.lib.glfsx_post_ragged_device(SALT, None, d.data_ptr(), z.data_ptr(), z.data_ptr(),
                                          1, MAX_RAGGED + 1, None, refs.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == gpu.GLFSX_E_UNSUPPORTED
    assert bytes(refs.cpu().numpy().tobytes()) == b"\xa5" * 64


def test_offsets_above_4gib(gpu, O):
    """Messages just below 2 GiB, just below 4 GiB and above 4 GiB of one
    buffer (small_kernels.h: a sign-extended readfirstlane once sent every
    wave of the upper 2 GiB of each 4 GiB down the wrong path)."""
    import torch
    N = gpu
    big, small = 70 * KIB + 9, KIB + 1
    lens = [big, small, big, small, big, small]
    GIB = 1 << 30
    offs = [2 * GIB - 80 * KIB, 2 * GIB - 2 * KIB, 4 * GIB - 80 * KIB, 4 * GIB - 2 * KIB,
            4 * GIB + 64 * KIB, 4 * GIB + 2 * MIB - 2 * KIB]
    msgs, _ = _messages(O, "far", lens, 26)
    want = _want(O, "far", None)
    total = 4 * GIB + 2 * MIB
    d = torch.empty(total, dtype=torch.uint8, device="cuda")
    ct = torch.empty(total, dtype=torch.uint8, device="cuda")
    # the regions used: 128 KiB around each pair, zero outside the messages
    regions = [(2 * GIB - 96 * KIB, 2 * GIB + 32 * KIB), (4 * GIB - 96 * KIB, 4 * GIB + 160 * KIB),
               (4 * GIB + 2 * MIB - 4 * KIB, total)]
    for lo, hi in regions:
        d[lo:hi] = 0
        ct[lo:hi] = 0
    for o, m in zip(offs, msgs):
        d[o:o + len(m)] = torch.from_numpy(np.frombuffer(m, dtype=np.uint8).copy()).cuda()
    n = len(lens)
    do = torch.tensor(offs, dtype=torch.int64, device="cuda")
    dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
    refs = torch.full((64 * n,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib.glfsx_post_ragged_device(SALT, None, d.data_ptr(), do.data_ptr(),
                                           dl.data_ptr(), n, big, ct.data_ptr(),
                                           refs.data_ptr(), None))
    torch.cuda.synchronize()
    got = refs.cpu().numpy().tobytes()
    assert [got[64 * i:64 * i + 64] for i in range(n)] == [r for r, _ in want]
    for lo, hi in regions:
        img = np.zeros(hi - lo, dtype=np.uint8)
        for o, (_, c) in zip(offs, want):
            if lo <= o < hi:
                img[o - lo:o - lo + len(c)] = np.frombuffer(c, dtype=np.uint8)
        assert np.array_equal(ct[lo:hi].cpu().numpy(), img), (lo, hi)


def test_reuse(gpu, O):
    """The per-stream scratch across calls of different shapes: three cases
    back to back on one stream, twice, then one shape on two streams with no
    synchronisation between the calls."""
    import torch
    N = gpu
    edge = _edge_order()
    cases = [("edge", edge, 21, _offsets(edge, 64, 0, gap=3)),
             ("many", _many(), 22, _offsets(_many(), 1, 0)),
             ("dense", [64 * KIB] * 317, 23, _offsets([64 * KIB] * 317, 1, 0))]
    s = torch.cuda.Stream()
    dev = []
    for name, lens, seed, (offs, total) in cases:
        msgs, _ = _messages(O, name, lens, seed)
        dev.append(torch.from_numpy(_image(total, offs, msgs)).cuda())
    runs = []
    for _ in range(2):
        for (name, lens, seed, (offs, total)), d in zip(cases, dev):
            runs.append((name, offs, total,
                         _launch(N, torch, d, offs, lens, max(lens), "separate", None, s)))
    for name, offs, total, (refs, ct, _keep) in runs:
        _check(torch, refs, ct, offs, _want(O, name, None), total)
    name, lens, seed, (offs, total) = cases[0]
    s2 = torch.cuda.Stream()
    two = [_launch(N, torch, dev[0], offs, lens, max(lens), "separate", None, st)
           for st in (s, s2, s, s2)]
    for refs, ct, _keep in two:
        _check(torch, refs, ct, offs, _want(O, name, None), total)


def _open_no_plaintext(N, O, torch, name, bs, n, stream):
    """A verified read of n blocks of bs bytes on the composed route, salted,
    no plaintext buffer, block 1 damaged and the last ref's DEK foreign: the
    status words, and what the oracle's refs say they are."""
    if name not in _cache:
        data = O.fill_splitmix(n * bs, 31 + n * bs)
        posts = [O.post(SALT, data[o:o + bs], None) for o in range(0, n * bs, bs)]
        ct = bytearray(b"".join(c for _, c in posts))
        refs = bytearray(b"".join(r for r, _ in posts))
        ct[bs + 5] ^= 1
        refs[64 * (n - 1) + 33] ^= 1
        _cache[name] = (bytes(ct), bytes(refs))
    ct, refs = _cache[name]
    d_ct = torch.from_numpy(np.frombuffer(ct, dtype=np.uint8).copy()).cuda()
    d_refs = torch.from_numpy(np.frombuffer(refs, dtype=np.uint8).copy()).cuda()
    d_st = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib.glfsx_open_batch_device(SALT, None, d_ct.data_ptr(), n * bs, bs,
                                          d_refs.data_ptr(), None, d_st.data_ptr(),
                                          stream.cuda_stream))
    torch.cuda.synchronize()
    want = [0] * n
    want[1], want[n - 1] = 3, 2  # CID and DEK of block 1; the DEK of the last
    return [int(x) & 0xFFFFFFFF for x in d_st.cpu().tolist()], want


def test_scratch_small_large_small(gpu, O):
    """The two routes whose per-stream scratch outgrows its 1 MiB floor at
    small sizes, on a stream of their own (so its buffers start empty): a
    small call, a large one that makes the buffer grow, the small one again.
    Ragged post: 64 messages of about 1 MiB in all, then 48 MiB (more than
    32768 chunks at 32 B of CV scratch each).  Verified read, composed route,
    no plaintext buffer (the scratch holds the plaintext): 8 x 64 KiB, then
    8 x 1 MiB.  Every ref and status word is the oracle's, and the third
    result is the first byte for byte."""
    import torch
    N = gpu
    s = torch.cuda.Stream()
    small = [(i * 997) % (32 * KIB) + 1 for i in range(64)]
    large = ([5 * MIB + 77] * 4 + [3 * MIB + 1025] * 5 + [2 * MIB] * 4 + [MIB + 1] * 4 +
             [100 * KIB + 3] * 8 + [0, 1, 1023, 1025, 65537])
    random.Random(15).shuffle(large)
    assert abs(sum(small) - MIB) < MIB // 8
    assert sum((ln + 1023) // 1024 for ln in large) > 32768
    got = []
    for name, lens, seed in (("grow_s", small, 29), ("grow_l", large, 30), ("grow_s", small, 29)):
        offs, total = _offsets(lens, 16, 0, gap=3)
        got.append(_run(N, O, name, lens, seed, offs, total, stream=s))
    assert got[0] == got[2]
    prev = N.set_open_route(1)
    try:
        got = []
        for name, bs in (("open_s", 64 * KIB), ("open_l", MIB), ("open_s", 64 * KIB)):
            st, want = _open_no_plaintext(N, O, torch, name, bs, 8, s)
            assert st == want, (name, st)
            got.append(st)
        assert got[0] == got[2]
    finally:
        N.set_open_route(prev)


ROUTE_LENS = [0, 100, 4096, 16384, 16385, 40000, 65536, 300000, 2 * MIB, 2 * MIB + 1, 5 * MIB]


@pytest.mark.parametrize("bs", [2 * MIB, 64 * KIB])
def test_route_post_blobs_device(gpu, O, bs):
    """glfsx_post_blobs_device over a mix of small, single-block and
    multi-block blobs: every root is the oracle's Create of the blob, the
    ciphertext of every single-block blob the oracle's."""
    import torch
    N = gpu
    salt = O.derive_key(bytes(32), b"blob")
    rng = random.Random(13)
    lens = [rng.choice(ROUTE_LENS) for _ in range(200)]
    offs, total = _offsets(lens, 64, 0)
    data = O.fill_splitmix(total, 27)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    ct = torch.zeros_like(d)
    n = len(lens)
    do = torch.tensor(offs, dtype=torch.int64, device="cuda")
    dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
    roots = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib.glfsx_post_blobs_device(bs, salt, None, d.data_ptr(), do.data_ptr(),
                                          dl.data_ptr(), n, max(lens), ct.data_ptr(),
                                          roots.data_ptr(), None))
    torch.cuda.synchronize()
    got, gct = roots.cpu().numpy().tobytes(), ct.cpu().numpy()
    for i, (o, ln) in enumerate(zip(offs, lens)):
        root, _, _, posts = O.create(data[o:o + ln], bs, salt=salt)
        assert got[64 * i:64 * i + 64] == root, (i, ln)
        if 0 < ln <= bs:  # one block: its Post's ctext
            assert len(posts) == 1
            assert gct[o:o + ln].tobytes() == posts[0][3], (i, ln)


def _host_batch(O):
    if "host" not in _cache:
        counts = {0: 12, 100: 20, 4096: 20, 16384: 12, 16385: 12, 40000: 20, 65536: 12,
                  300000: 12, 2 * MIB: 68, 2 * MIB + 1: 6, 5 * MIB: 6}
        assert set(counts) == set(ROUTE_LENS)
        lens = [ln for ln, c in counts.items() for _ in range(c)]
        random.Random(14).shuffle(lens)
        offs, total = _offsets(lens, 1, 0, gap=3)
        data = O.fill_splitmix(total, 28)
        salt = O.derive_key(bytes(32), b"blob")
        bs = 2 * MIB
        want, first = [], []  # the Post log; each blob's first Post in it
        for o, ln in zip(offs, lens):
            first.append(len(want))
            want += O.create(data[o:o + ln], bs, salt=salt)[3]
        _cache["host"] = (lens, offs, data, salt, bs, want, first)
    return _cache["host"]


def _post_blobs_host(N, batch, fail_at=0):
    lens, offs, data, salt, bs, _, _ = batch
    log = []

    @N.POST_FN
    def sink(_ctx, kind, ref, ct, n):
        log.append((kind, ctypes.string_at(ref, 64), n, ctypes.string_at(ct, n) if n else b""))
        return 1 if len(log) == fail_at else 0

    n = len(lens)
    roots = ctypes.create_string_buffer(64 * n)
    rc = N.lib.glfsx_post_blobs(bs, bs, salt, None, data, (ctypes.c_uint64 * n)(*offs),
                                (ctypes.c_uint64 * n)(*lens), n, sink, None, roots)
    return rc, log


def test_route_post_blobs_host(gpu, O):
    """glfsx_post_blobs from host memory, the single-block blobs above 16 KiB
    in the 64 MiB groups (three of them) with the small ones: the whole Post
    log (kind, ref, ctext) is that of n sequential PostBlob calls."""
    batch = _host_batch(O)
    lens = batch[0]
    assert sum(ln for ln in lens if ln <= 2 * MIB) > 2 * (64 * MIB)  # three groups
    rc, log = _post_blobs_host(gpu, batch)
    assert rc == 0, gpu.last_error()
    assert log == batch[5]


@pytest.mark.parametrize("where", [4096, 40000, 5 * MIB])
def test_route_post_blobs_host_store_error(gpu, O, where):
    """The store fails at the k-th Post -- in a small blob, in a 40 000-byte
    blob (ragged), in a multi-block blob (its second Post): GLFSX_E_STORE,
    and the store was handed exactly Posts 1 .. k in order, k - 1 of them
    delivered and nothing after the one that failed."""
    batch = _host_batch(O)
    lens, want, first = batch[0], batch[5], batch[6]
    i = [j for j, ln in enumerate(lens) if ln == where][len(lens) // 40]
    k = first[i] + (2 if where > 2 * MIB else 1)
    rc, log = _post_blobs_host(gpu, batch, fail_at=k)
    assert rc == gpu.GLFSX_E_STORE
    assert len(log) == k
    assert log[:k - 1] == want[:k - 1]
    assert log[k - 1] == want[k - 1]
