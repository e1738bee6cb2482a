"""The ragged open: glfsx_open_ragged_device over batches of messages of
unequal length, and glfsx_open_blobs from host memory.  Refs and ciphertexts
are the oracle's posts (ref.go:98-161); every status word and every byte of
every buffer is compared, nothing is sampled.  Buffers start at a fill byte
and are compared whole, so a store outside a message's own bytes shows up."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_small_decrypt_matrix import (OPEN0, OPEN1, OPEN2, RAG_CHUNK, RAG_FAMILIES,
                                           RAG_MERGE_A, RAG_MERGE_B, aux_reset, aux_take,
                                           latency_wgs_now, rag_expect)

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
MAX_RAGGED = 16 * MIB
SALT = bytes(range(7, 39))
FOREIGN = bytes(range(9, 41))
CID_KEY = bytes(range(100, 132))
GAP, PT_FILL, ST_FILL = 0x5C, 0xEE, 0x5A5A5A5A

# tests/test_gpu_ragged.py's edge lengths (chunk counts on both sides of 1,
# 64, 256 and the merge-B boundary), and a second 7 KiB message for the swap
EDGE_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3073, 5 * KIB, 6 * KIB + 1, 7 * KIB,
             16384, 16385, 17 * KIB + 5, 65535, 65536, 65537, 100 * KIB + 3, 262143, 262144,
             262145, 257 * KIB, 513 * KIB + 700, 1 * MIB, 2 * MIB, 2 * MIB + 1, 5 * MIB + 77]

_cache = {}


def _batch(O, name, lens, seed, key=None):
    """The messages of a case (consecutive slices of one splitmix stream) and
    the oracle's refs and ctexts of them: computed once per (case, key)."""
    if name not in _cache:
        stream = O.fill_splitmix(sum(lens) + 1, seed)
        msgs, o = [], 0
        for ln in lens:
            msgs.append(stream[o:o + ln])
            o += ln
        _cache[name] = (msgs, {})
    msgs, posts = _cache[name]
    if key not in posts:
        p = [O.post(SALT, m, key) for m in msgs]
        posts[key] = ([r for r, _ in p], [c for _, c in p])
    return msgs, posts[key][0], posts[key][1]


def _offsets(lens, align, phase, gap=0):
    """Message i at the first offset = phase (mod align) at or after the end
    of message i - 1 plus gap; guard bytes before the first and after the
    last message."""
    offs, o = [], 48
    for ln in lens:
        o += (phase - o) % align
        offs.append(o)
        o += ln + gap
    return offs, o + 64


def _image(total, offs, pieces, fill):
    img = np.full(total, fill, dtype=np.uint8)
    for o, p in zip(offs, pieces):
        img[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return img


def _dev(torch, b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def _launch(N, torch, d_ct, offs, lens, max_len, refs, ptext="separate", salt=SALT, key=None,
            stream=None, thr=False):
    """One call; returns the device tensors (status, ptext or None) without
    synchronising anything itself.  thr (None: the default latency threshold,
    else its value): the aux log must show the one pass in the call's mode --
    2 with a salt, else 1 with a plaintext buffer, else 0 -- in the ARX form
    of that threshold, and the merge levels the lengths have work for."""
    n = len(lens)
    do = torch.tensor(offs, dtype=torch.int64, device="cuda")
    dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
    d_refs = refs if hasattr(refs, "data_ptr") else _dev(torch, b"".join(refs))
    st = torch.full((n,), ST_FILL, dtype=torch.int32, device="cuda")
    pt = {"none": None, "inplace": d_ct}.get(ptext)
    if ptext == "separate":
        pt = torch.full_like(d_ct, PT_FILL)
    torch.cuda.synchronize()
    aux_reset(N)
    rc = N.lib.glfsx_open_ragged_device(
        salt, key, d_ct.data_ptr(), do.data_ptr(), dl.data_ptr(), n, max_len,
        d_refs.data_ptr(), pt.data_ptr() if pt is not None else None, st.data_ptr(),
        stream.cuda_stream if stream is not None else None)
    assert rc == 0, N.last_error()
    if thr is not False:
        kind = OPEN2 if salt is not None else OPEN1 if pt is not None else OPEN0
        form = 0 if thr is None else 2
        log = aux_take(N, families=RAG_FAMILIES)
        sel = [ln for ln in lens if ln <= max_len]
        assert thr is None or latency_wgs_now(N) == thr
        assert log == rag_expect(sel, kind, latency_wgs_now(N)), (kind, thr)
        if max(sel) > 256 * KIB:
            assert [(r[0], r[1], r[4]) for r in log] == [
                (RAG_CHUNK, kind, form), (RAG_MERGE_A, kind, 0), (RAG_MERGE_B, kind, 0)]
    return st, pt, (do, dl, d_refs)


def _status(torch, st):
    torch.cuda.synchronize()
    return [int(x) & 0xFFFFFFFF for x in st.cpu().tolist()]


def _same(got, want, what):
    diff = np.flatnonzero(got.cpu().numpy() != want)
    assert diff.size == 0, (what, diff[:10], diff.size)


def _run(N, O, name, lens, seed, offs, total, ptext="separate", key=None, salt=SALT,
         stream=None, want=None, thr=False):
    """A clean batch in one ptext mode: every status 0 (or `want`), the
    plaintext the messages, every other byte of every buffer its fill."""
    import torch
    msgs, refs, cts = _batch(O, name, lens, seed, key)
    ct_img = _image(total, offs, cts, GAP)
    d_ct = torch.from_numpy(ct_img.copy()).cuda()
    st, pt, _keep = _launch(N, torch, d_ct, offs, lens, max(lens), refs, ptext, salt, key, stream,
                            thr)
    got = _status(torch, st)
    assert got == (want if want is not None else [0] * len(lens)), \
        [(i, s) for i, s in enumerate(got) if s][:10]
    if ptext == "separate":
        _same(pt, _image(total, offs, msgs, PT_FILL), "ptext")
        _same(d_ct, ct_img, "ctext changed")
    elif ptext == "inplace":
        _same(d_ct, _image(total, offs, msgs, GAP), "ptext in place")
    else:
        _same(d_ct, ct_img, "ctext changed")
    return got


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
    return lens + [7 * KIB]


@pytest.mark.parametrize("thr", [None, 0])
@pytest.mark.parametrize("align,phase", [(64, 0), (64, 16), (2, 1)])
def test_edge_lengths(gpu, O, latency_wgs, align, phase, thr):
    """Chunk counts 1 .. 5121 at 64-B aligned, 16-B aligned and odd offsets
    with gaps, in the compiler's ARX form (default threshold) and the asm
    form (threshold 0); plaintext separate, in place and absent."""
    if thr is not None:
        latency_wgs(thr)
    lens = _edge_order()
    offs, total = _offsets(lens, align, phase, gap=3)
    for ptext in ("separate", "inplace", "none"):
        _run(gpu, O, "edge", lens, 21, offs, total, ptext=ptext, thr=thr)      # mode 2


def test_keyed_cid_and_no_salt(gpu, O):
    """A keyed store; without a salt only the CID is checked -- with a
    plaintext buffer (keystream, no DEK chain) and without (CID alone)."""
    lens = _edge_order()
    offs, total = _offsets(lens, 16, 0, gap=5)
    for ptext in ("separate", "inplace", "none"):
        _run(gpu, O, "edge", lens, 21, offs, total, ptext=ptext, key=CID_KEY, thr=None)
        _run(gpu, O, "edge", lens, 21, offs, total, ptext=ptext, key=CID_KEY, salt=None, thr=None)
        _run(gpu, O, "edge", lens, 21, offs, total, ptext=ptext, salt=None, thr=None)
    # the wrong CID key: bit 0 everywhere, the DEK check still passes
    import torch
    msgs, refs, cts = _batch(O, "edge", lens, 21, CID_KEY)
    d_ct = torch.from_numpy(_image(total, offs, cts, GAP)).cuda()
    st, pt, _k = _launch(gpu, torch, d_ct, offs, lens, max(lens), refs, "separate", SALT, None)
    assert _status(torch, st) == [1] * len(lens)
    _same(pt, _image(total, offs, msgs, PT_FILL), "ptext")


def _damaged(lens, refs, cts):
    """Each kind of damage on another message of the edge batch: the ctexts,
    the refs and the status words they must give."""
    cts, refs = [bytearray(c) for c in cts], [bytearray(r) for r in refs]
    want = [0] * len(lens)
    at = lens.index

    def flip(ln, byte):
        cts[at(ln)][byte] ^= 0x10
        want[at(ln)] = 3

    flip(63, 0)                          # the first byte
    flip(65537, 65536)                   # the last byte
    flip(3073, 1023)                     # the end of a multi-chunk message's chunk 0
    flip(5 * KIB, 1024)                  # the start of its chunk 1
    flip(513 * KIB + 700, 255 * KIB + 5)  # chunk 255 of 514: the end of merge group 0
    flip(1 * MIB, 256 * KIB + 5)         # chunk 256 of 1024: the start of group 1
    refs[at(64)][3] ^= 1                 # a CID byte of the ref
    want[at(64)] = 1
    refs[at(2048)][40] ^= 1              # a DEK byte of the ref
    want[at(2048)] = 2
    refs[at(0)][63] ^= 0x80              # ... and of the empty message's
    want[at(0)] = 2
    a, b = [i for i, ln in enumerate(lens) if ln == 7 * KIB]
    refs[a], refs[b] = refs[b], refs[a]  # two equal-length messages' refs swapped
    want[a] = want[b] = 3
    return [bytes(c) for c in cts], [bytes(r) for r in refs], want


@pytest.mark.parametrize("thr", [None, 0])
def test_damage(gpu, O, latency_wgs, thr):
    import torch
    if thr is not None:
        latency_wgs(thr)
    lens = _edge_order()
    offs, total = _offsets(lens, 16, 0, gap=3)
    _, refs, cts = _batch(O, "edge", lens, 21)
    cts, refs, want = _damaged(lens, refs, cts)
    ct_img = _image(total, offs, cts, GAP)
    for ptext in ("separate", "none"):
        d_ct = torch.from_numpy(ct_img.copy()).cuda()
        st, _pt, _k = _launch(gpu, torch, d_ct, offs, lens, max(lens), refs, ptext, thr=thr)
        assert _status(torch, st) == want
        # no salt: only bit 0, where the CID is wrong (mode 1 with a plaintext
        # buffer, mode 0 without: both ARX forms of each over the two thr)
        st, _pt, _k = _launch(gpu, torch, d_ct, offs, lens, max(lens), refs, ptext, salt=None,
                              thr=thr)
        assert _status(torch, st) == [w & 1 for w in want]
    # a foreign salt: bit 1 on every message, the empty one included
    st, _pt, _k = _launch(gpu, torch, d_ct, offs, lens, max(lens), refs, "none", salt=FOREIGN)
    assert _status(torch, st) == [w | 2 for w in want]


def _many():
    lens = [i % 1025 for i in range(70001)]
    lens[35000] = 300 * KIB
    return lens


def test_many_messages(gpu, O):
    """70 001 messages: the plan's second level (274 plan workgroups), tiles
    mixing hundreds of messages, one message that starts inside a tile and
    spans 300 of them; a handful damaged."""
    import torch
    lens = _many()
    offs, total = _offsets(lens, 1, 0)
    _run(gpu, O, "many", lens, 22, offs, total)
    msgs, refs, cts = _batch(O, "many", lens, 22)
    cts, refs, want = list(cts), list(refs), [0] * len(lens)
    for i, byte, st in ((1, 0, 3), (1024, 1023, 3), (35000, 200 * KIB, 3), (35001, 5, 3),
                       (70000, 0, 3)):
        c = bytearray(cts[i])
        c[byte] ^= 1
        cts[i], want[i] = bytes(c), st
    r = bytearray(refs[0])   # the empty message at the very start
    r[0] ^= 1
    refs[0], want[0] = bytes(r), 1
    r = bytearray(refs[69999])
    r[32] ^= 1
    refs[69999], want[69999] = bytes(r), 2
    d_ct = torch.from_numpy(_image(total, offs, cts, GAP)).cuda()
    st, _pt, _k = _launch(gpu, torch, d_ct, offs, lens, max(lens), refs, "none")
    got = _status(torch, st)
    assert got == want, [(i, s) for i, s in enumerate(got) if s != want[i]][:10]


def test_the_limit(gpu, O):
    """A 16 MiB message alone and among 100 small ones; one byte more is
    refused before any launch; a message above max_len inside a batch fails
    closed, untouched, beside neighbours that are checked normally."""
    import torch
    lens = [MAX_RAGGED]
    offs, total = _offsets(lens, 64, 0)
    _run(gpu, O, "limit1", lens, 24, offs, total)
    big = _cache["limit1"]
    lens = [1 + 10 * i for i in range(50)] + [MAX_RAGGED] + [1024 - i for i in range(50)]
    offs, total = _offsets(lens, 16, 0)
    msgs, refs, cts = _batch(O, "limit101", lens[:50] + [0] + lens[51:], 25)
    msgs, refs, cts = list(msgs), list(refs), list(cts)
    msgs[50], refs[50], cts[50] = big[0][0], big[1][None][0][0], big[1][None][1][0]
    ct_img = _image(total, offs, cts, GAP)
    d_ct = torch.from_numpy(ct_img.copy()).cuda()
    st, pt, _k = _launch(gpu, torch, d_ct, offs, lens, MAX_RAGGED, refs)
    assert _status(torch, st) == [0] * len(lens)
    _same(pt, _image(total, offs, msgs, PT_FILL), "ptext")
    # one byte more: refused before any launch, status and ptext untouched
    do = torch.tensor(offs, dtype=torch.int64, device="cuda")
    dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
    d_refs = _dev(torch, b"".join(refs))
    st = torch.full((len(lens),), ST_FILL, dtype=torch.int32, device="cuda")
    pt = torch.full_like(d_ct, PT_FILL)
    torch.cuda.synchronize()
    rc = gpu.lib.glfsx_open_ragged_device(SALT, None, d_ct.data_ptr(), do.data_ptr(),
                                          dl.data_ptr(), len(lens), MAX_RAGGED + 1,
                                          d_refs.data_ptr(), pt.data_ptr(), st.data_ptr(), None)
    assert rc == gpu.GLFSX_E_UNSUPPORTED
    assert _status(torch, st) == [ST_FILL] * len(lens)
    assert bool((pt == PT_FILL).all())
    # max_len below the big message: it alone gets GLFSX_BAD_CID, unread and
    # unwritten; a damaged and the clean neighbours are checked as ever
    c = bytearray(cts[49])
    c[7] ^= 1
    bad_cts = cts[:49] + [bytes(c)] + cts[50:]
    d_ct = torch.from_numpy(_image(total, offs, bad_cts, GAP)).cuda()
    st, pt, _k = _launch(gpu, torch, d_ct, offs, lens, 4096, refs)
    want = [0] * len(lens)
    want[49], want[50] = 3, gpu.GLFSX_BAD_CID
    assert _status(torch, st) == want
    got = pt.cpu().numpy()
    o = offs[50]
    assert bool((got[o:o + MAX_RAGGED] == PT_FILL).all())
    exp = _image(total, offs, msgs[:50] + [b""] + msgs[51:], PT_FILL)
    exp[offs[49]:offs[49] + lens[49]] = got[offs[49]:offs[49] + lens[49]]  # damaged: any bytes
    assert np.array_equal(got, exp)


def test_reuse(gpu, O):
    """The per-stream scratch across calls of different shapes: three cases
    back to back on one stream, twice, then one shape on two streams with no
    synchronisation between the calls."""
    import torch
    N = gpu
    edge = _edge_order()
    dense = [64 * KIB] * 317
    cases = [("edge", edge, 21, _offsets(edge, 64, 0, gap=3)),
             ("many", _many(), 22, _offsets(_many(), 1, 0)),
             ("dense", dense, 23, _offsets(dense, 1, 0))]
    s = torch.cuda.Stream()
    dev, exp = [], []
    for name, lens, seed, (offs, total) in cases:
        msgs, refs, cts = _batch(O, name, lens, seed)
        dev.append((torch.from_numpy(_image(total, offs, cts, GAP)).cuda(),
                    _dev(torch, b"".join(refs))))
        exp.append(_image(total, offs, msgs, PT_FILL))
    runs = []
    for _ in range(2):
        for k, (name, lens, seed, (offs, total)) in enumerate(cases):
            runs.append((k, _launch(N, torch, dev[k][0], offs, lens, max(lens), dev[k][1],
                                    stream=s)))
    for k, (st, pt, _keep) in runs:
        assert _status(torch, st) == [0] * len(cases[k][1])
        _same(pt, exp[k], "ptext")
    name, lens, seed, (offs, total) = cases[0]
    s2 = torch.cuda.Stream()
    two = [_launch(N, torch, dev[0][0], offs, lens, max(lens), dev[0][1], stream=st_)
           for st_ in (s, s2, s, s2)]
    for st, pt, _keep in two:
        assert _status(torch, st) == [0] * len(lens)
        _same(pt, exp[0], "ptext")


def test_scratch_small_large_small(gpu, O):
    """On a stream of its own (so its buffers start empty): a small call, one
    whose CV scratch (64 B a chunk, more than 16384 chunks) outgrows the 1 MiB
    floor, the small one again."""
    import torch
    s = torch.cuda.Stream()
    small = [(i * 997) % (32 * KIB) + 1 for i in range(64)]
    large = ([5 * MIB + 77] * 2 + [3 * MIB + 1025] * 3 + [2 * MIB] * 2 + [MIB + 1] * 2 +
             [100 * KIB + 3] * 4 + [0, 1, 1023, 1025, 65537])
    random.Random(15).shuffle(large)
    assert sum((ln + 1023) // 1024 for ln in large) > 16384
    for name, lens, seed in (("grow_s", small, 29), ("grow_l", large, 30), ("grow_s", small, 29)):
        offs, total = _offsets(lens, 16, 0, gap=3)
        _run(gpu, O, name, lens, seed, offs, total, stream=s)
    torch.cuda.synchronize()


def _host_batch(O):
    """More than 128 MiB of mixed lengths (three groups of at most 64 MiB)
    at offsets with gaps; a few damaged, the first in the second group."""
    if "host" not in _cache:
        counts = {0: 5, 1: 5, 100: 20, 4096: 20, 16385: 10, 65537: 10, 300000: 10,
                  MIB + 1: 20, 2 * MIB: 34, 5 * MIB + 77: 6, 3 * MIB + 1025: 3}
        lens = [ln for ln, c in counts.items() for _ in range(c)]
        random.Random(14).shuffle(lens)
        assert sum(lens) > 2 * (64 * MIB)
        offs, total = _offsets(lens, 1, 0, gap=3)
        msgs, refs, cts = _batch(O, "hostmsgs", lens, 28)
        cts, refs, want = list(cts), list(refs), [0] * len(lens)
        acc, first = 0, None
        for i, ln in enumerate(lens):  # the first message past 70 MiB with some bytes
            acc += ln
            if acc > 70 * MIB and ln > 4096:
                first = i
                break
        c = bytearray(cts[first])
        c[len(c) // 2] ^= 4
        cts[first], want[first] = bytes(c), 3
        last = max(i for i, ln in enumerate(lens) if ln == 100)
        assert last > first
        r = bytearray(refs[last])
        r[50] ^= 1
        refs[last], want[last] = bytes(r), 2
        mid = next(i for i in range(first + 1, len(lens)) if lens[i] == 2 * MIB)
        r = bytearray(refs[mid])
        r[0] ^= 1
        refs[mid], want[mid] = bytes(r), 1
        _cache["host"] = (lens, offs, total, msgs, refs, cts, want, first)
    return _cache["host"]


def test_host_form(gpu, O):
    """glfsx_open_blobs from host memory over three groups: statuses, n_bad,
    GLFSX_E_CORRUPT and its text, the whole of ptext, and the device form's
    results on the same bytes."""
    import torch
    N = gpu
    lens, offs, total, msgs, refs, cts, want, first = _host_batch(O)
    n = len(lens)
    ct = _image(total, offs, cts, GAP)
    pt = np.full(total, PT_FILL, dtype=np.uint8)
    st = (ctypes.c_uint32 * n)(*([ST_FILL] * n))
    bad = ctypes.c_uint64(99)
    O_, L_ = (ctypes.c_uint64 * n)(*offs), (ctypes.c_uint64 * n)(*lens)
    rb = b"".join(refs)
    rc = N.lib.glfsx_open_blobs(SALT, None, ct.ctypes.data, O_, L_, n, rb, pt.ctypes.data, st,
                                ctypes.byref(bad))
    err = N.last_error()
    assert rc == N.GLFSX_E_CORRUPT
    assert list(st) == want
    assert bad.value == 3
    assert f"message {first} of {n} failed its CID and DEK checks (3 bad in all)" in err, err
    exp = _image(total, offs, msgs, PT_FILL)
    for i, w in enumerate(want):
        if w & 2:  # damaged bytes, or a ref with another DEK: any plaintext
            exp[offs[i]:offs[i] + lens[i]] = pt[offs[i]:offs[i] + lens[i]]
    assert np.array_equal(pt, exp)
    assert np.array_equal(ct, _image(total, offs, cts, GAP))
    # check only, no outputs: the same verdict
    assert N.lib.glfsx_open_blobs(SALT, None, ct.ctypes.data, O_, L_, n, rb, None, None,
                                  None) == N.GLFSX_E_CORRUPT
    # the device form on the same bytes
    d_ct = torch.from_numpy(ct).cuda()
    dst, dpt, _k = _launch(N, torch, d_ct, offs, lens, max(lens), refs)
    assert _status(torch, dst) == want
    assert np.array_equal(dpt.cpu().numpy(), pt)
    # a clean batch returns 0 and counts nothing
    _, good_refs, good_cts = _batch(O, "hostmsgs", lens, 28)
    ct = _image(total, offs, good_cts, GAP)
    pt2 = np.full(total, PT_FILL, dtype=np.uint8)
    rc = N.lib.glfsx_open_blobs(SALT, None, ct.ctypes.data, O_, L_, n, b"".join(good_refs),
                                pt2.ctypes.data, st, ctypes.byref(bad))
    assert rc == 0, N.last_error()
    assert list(st) == [0] * n and bad.value == 0
    assert np.array_equal(pt2, _image(total, offs, msgs, PT_FILL))
