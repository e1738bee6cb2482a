"""The checked per-block read interface of the mirror: Machine.get_f /
get_piece / read_at / Reader with salt= / cid_key= (every block and index
node through glfsx_open), and glfs.Machine(with_verify()).  Blobs are written
by the library's Writer into a MemStore; one stored blob is then overwritten,
the way tests/test_gpu_verify.py tampers with its store."""
import random

import pytest

pytestmark = pytest.mark.gpu

SALT = bytes(range(7, 39))
MiB = 1 << 20
DEEP = (1024, 256 * 1024 + 1)        # depth 3 at bf 16: 257 data blocks, 17 + 2 + 1 nodes
SHAPES = [(1024, 0), (1024, 1), (1024, 1024), (1024, 16 * 1024 + 5), DEEP]
ODD = (130, 1000)                    # bs % 64 != 0, bf 2: 8 data blocks, 4 + 2 + 1 nodes
BIG = (2 * MiB, 3 * MiB)             # the staged route: two blocks and a 2 MiB index node


@pytest.fixture(autouse=True)
def _auto_route(gpu):
    gpu.set_open_route(0)
    yield
    gpu.set_open_route(0)


@pytest.fixture(scope="module")
def blobs(O):
    """{shape: (data, root, {cid: ctext}, post log)}, written once; the tests
    work on copies of the blob dict."""
    from glfs_amd import bigblob
    out = {}
    for bs, size in SHAPES + [ODD, BIG]:
        data = O.fill_splitmix(size, size + 11)
        store = bigblob.MemStore(bs)
        root = bigblob.Machine(block_size=bs).create(store, SALT, data)
        if bs % 64 == 0 and size <= MiB:
            assert root.ref.marshal_binary() == O.create(data, bs, salt=SALT)[0]
        out[(bs, size)] = (data, root, dict(store.blobs), list(store.log))
    return out


def _store(blobs, shape):
    from glfs_amd import bigblob
    data, root, stored, log = blobs[shape]
    s = bigblob.MemStore(shape[0])
    s.blobs = dict(stored)
    return data, root, s, log


def _damage(store, cid, at):
    b = bytearray(store.blobs[cid])
    b[at % len(b)] ^= 0x20
    store.blobs[cid] = bytes(b)


def _offsets(size, bs, seed, k=24):
    rng = random.Random(seed)
    return [(rng.randrange(size), rng.randrange(1, 3 * bs)) for _ in range(k)] if size else []


def _check_reads(m, store, root, data, bs, seed, **kw):
    r = m.new_reader(store, root, **kw)
    assert r.read() == data
    assert r.read(10) == b""
    for off, n in _offsets(len(data), bs, seed):
        got, eof = m.read_at(store, root, off, n, **kw)
        end = min((off // bs + 1) * bs, len(data))
        assert got == data[off:min(off + n, end)]
        assert eof == (off + len(got) == len(data))
        assert r.read_at(n, off)[0] == got


@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_checked_reader_clean(gpu, O, blobs, shape):
    from glfs_amd import bigblob
    data, root, store, _ = _store(blobs, shape)
    bs = shape[0]
    m = bigblob.Machine(block_size=bs)
    _check_reads(m, store, root, data, bs, 1, salt=SALT)
    _check_reads(bigblob.Machine(block_size=bs), store, root, data, bs, 2, cid_key=None, salt=SALT)
    if not data:     # the empty blob: one post of no bytes under the index salt
        assert m.read_at(store, root, 0, 1, salt=SALT) == (b"", True)
    # a blob written under another salt: the first block read refuses its DEK
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        bigblob.Machine(block_size=bs).read_at(store, root, 0, 1, salt=bytes(32))
    assert ei.value.status == 2 and ei.value.level == bigblob.depth(root.size, bs)
    # a store keyed otherwise: its CID
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        bigblob.Machine(block_size=bs).read_at(store, root, 0, 1, cid_key=bytes(range(32)))
    assert ei.value.status == 1 and ei.value.cid == root.ref.cid
    # traverse / populate with the checks see the same tree
    a, b = bigblob.CIDSet(), bigblob.CIDSet()
    m.populate(store, root, a)
    m.populate(store, root, b, salt=SALT)
    assert a.cids == b.cids and len(b.cids) == len(store)


def test_derived_salts_are_cached(gpu, O, blobs, monkeypatch):
    """A read_at must not pay two derive_key GPU calls."""
    from glfs_amd import bigblob
    data, root, store, _ = _store(blobs, DEEP)
    m = bigblob.Machine(block_size=DEEP[0])
    calls = []
    real = bigblob.derive_key
    monkeypatch.setattr(bigblob, "derive_key", lambda *a, **k: calls.append(a) or real(*a, **k))
    for off in (0, 5000, 200000):
        assert m.read_at(store, root, off, 10, salt=SALT)[0] == data[off:off + 10]
    assert len(calls) == 2                # "index" and "raw", once per Machine and salt


def test_block_size_not_a_multiple_of_64(gpu, O, blobs):
    """bs 130: every stored blob passes get_f's checks under its level's salt
    (130-byte messages through k_one_open).  The Reader itself cannot walk
    such a blob, checked or not: getPiece wants index nodes of bf * 64 = 128
    bytes and the Writer makes them bs = 130 long (blob.go:59 against
    blob.go:111; the reference's own quirk, kept)."""
    from glfs_amd import bigblob
    data, root, store, log = _store(blobs, ODD)
    bs = ODD[0]
    m = bigblob.Machine(block_size=bs)
    index_salt, raw_salt = m._level_salts(SALT)
    blocks = [bigblob.Ref.from_bytes(ref) for kind, ref, _ in log if kind == bigblob.KIND_DATA]
    nodes = [bigblob.Ref.from_bytes(ref) for kind, ref, _ in log if kind == bigblob.KIND_INDEX]
    assert (len(blocks), len(nodes)) == (8, 7)
    got = b"".join(m.get_f(store, r, raw_salt) for r in blocks)
    assert got == data
    for r in nodes:
        node = m.get_f(store, r, index_salt)
        assert len(node) == bs and node[128:] == bytes(2)
    with pytest.raises(bigblob.ErrCorrupt) as ei:   # a data block under the nodes' salt
        bigblob.Machine(block_size=bs).get_f(store, blocks[3], index_salt)
    assert ei.value.status == 2
    _damage(store, blocks[7].cid, 89)               # the short last block
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        bigblob.Machine(block_size=bs).get_f(store, blocks[7], raw_salt)
    assert (ei.value.cid, ei.value.status) == (blocks[7].cid, 3)
    for kw in ({}, {"salt": SALT}):                 # the quirk, with and without the checks
        with pytest.raises(ValueError, match="not correct size for index"):
            bigblob.Machine(block_size=bs).new_reader(store, root, **kw).read()
    _damage(store, root.ref.cid, 5)                 # ... and the check comes before it
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        bigblob.Machine(block_size=bs).new_reader(store, root, salt=SALT).read()
    assert (ei.value.cid, ei.value.level) == (root.ref.cid, 3)


@pytest.mark.parametrize("level", [0, 1, 3])
def test_overwritten_blob(gpu, O, blobs, level):
    from glfs_amd import bigblob
    data, root, store, _ = _store(blobs, DEEP)
    bs = DEEP[0]
    levels = bigblob._tree_levels(store.get, root)
    assert [len(lv) for lv in levels] == [1, 2, 17, 257]
    j = {0: 200, 1: 11, 3: 0}[level]
    victim = levels[3 - level][j]
    # a data block anywhere; an index node in the DEK of a slot in use, so that
    # the unchecked walk still finds the child and decrypts it with a wrong key
    slot = {0: 0, 1: 2, 3: 0}[level]
    _damage(store, victim.cid, 70 if level == 0 else slot * 64 + 40)
    span = bs * 16 ** level                         # bytes below the victim
    lo, hi = j * span, min((j + 1) * span, len(data))
    hit = lo + (70 if level == 0 else slot * (span // 16) + 9)
    m = bigblob.Machine(block_size=bs, cache_size=1024)

    # the gap being closed: an unchecked Reader hands out wrong bytes, or walks
    # into a ref the damage spells -- never an error that names the blob
    try:
        got = m.read_at(store, root, hit, 64)[0]
        assert len(got) == 64 and got != data[hit:hit + 64]
        assert level < 3
    except (bigblob.ErrNotFound, ValueError):
        assert level == 3                           # garbage refs two levels up
    # the checked read raises, also now that the unchecked one has cached it
    for mm in (m, bigblob.Machine(block_size=bs)):
        for call in (lambda: mm.read_at(store, root, hit, 64, salt=SALT),
                     lambda: mm.new_reader(store, root, salt=SALT).read()):
            with pytest.raises(bigblob.ErrCorrupt) as ei:
                call()
            assert (ei.value.cid, ei.value.level) == (victim.cid, level)
            assert ei.value.status & 1
    # CID only (no salt) finds overwritten bytes as well
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        bigblob.open_block(store.get(victim.cid), victim, None)
    assert ei.value.status == 1
    # a checked read whose path avoids the victim still returns the data
    good = bigblob.Machine(block_size=bs)
    if level < 3:
        for off in (0, lo - 1, hi, len(data) - 1):
            assert good.read_at(store, root, off, 64, salt=SALT)[0] == \
                data[off:min(off + 64, (off // bs + 1) * bs, len(data))]
    with pytest.raises(bigblob.ErrCorrupt):
        good.read_at(store, root, hit, 64, salt=SALT)


def test_cache_entries_record_their_checks(gpu, O, blobs):
    from glfs_amd import bigblob
    data, root, store, _ = _store(blobs, (1024, 1024))
    m = bigblob.Machine(block_size=1024)
    index_salt, raw_salt = m._level_salts(SALT)
    ref = root.ref
    gets = []
    real = store.get
    store.get = lambda cid: gets.append(cid) or real(cid)
    assert m.get_f(store, ref) == data and len(gets) == 1
    assert m.get_f(store, ref) == data and len(gets) == 1            # unchecked: a hit
    assert m.get_f(store, ref, raw_salt) == data and len(gets) == 2  # unchecked entry: not enough
    assert m.get_f(store, ref, raw_salt) == data and len(gets) == 2  # now it is
    assert m.get_f(store, ref) == data and len(gets) == 2
    with pytest.raises(bigblob.ErrCorrupt):                          # another salt: checked anew
        m.get_f(store, ref, index_salt)
    assert len(gets) == 3
    assert m.get_f(store, ref, raw_salt) == data and len(gets) == 3  # the good entry survived
    m2 = bigblob.Machine(block_size=1024)
    key = bytes(range(32))
    with pytest.raises(bigblob.ErrCorrupt):
        m2.get_f(store, ref, None, key)
    assert len(m2._cache) == 0                                        # a bad block is not cached


def test_glfs_with_verify(gpu, O):
    from glfs_amd import bigblob, glfs
    store = bigblob.MemStore(2 * MiB)
    w = glfs.Machine()
    payload = O.fill_splitmix(100000, 77)
    small = w.post_blob(store, b"test data")
    big = w.post_blob(store, payload)
    tref = w.post_tree_map(store, {"a.txt": small, "dir/b.bin": big})
    v = glfs.Machine(glfs.with_verify())
    assert v.get_blob(store, small).read() == b"test data"
    assert v.get_blob_bytes(store, big, 1 << 20) == payload
    assert v.get_typed(store, "", big).read(10) == payload[:10]
    names = [e.name for e in v.get_tree_slice(store, tref)]
    assert names == [e.name for e in w.get_tree_slice(store, tref)] and names
    assert v.get_at_path(store, tref, "dir/b.bin").equals(big)
    assert v.get_at_path(store, tref, "a.txt").equals(small)
    # a store keyed otherwise than the Machine was told
    with pytest.raises(bigblob.ErrCorrupt):
        glfs.Machine(glfs.with_verify(bytes(range(32)))).get_blob(store, small).read()
    # the blob damaged in the store
    _damage(store, big.root.ref.cid, 4097)
    assert w.get_blob(store, big).read() != payload            # unchecked: wrong bytes
    assert v.get_blob(store, big).read() == payload            # v's LRU: the block it checked
    v = glfs.Machine(glfs.with_verify())                       # ... a Machine that fetches it
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        v.get_blob(store, big).read()
    assert (ei.value.cid, ei.value.level, ei.value.status) == (big.root.ref.cid, 0, 3)
    with pytest.raises(bigblob.ErrCorrupt):
        v.get_blob_bytes(store, big, 1 << 20)
    assert v.get_blob(store, small).read() == b"test data"     # the others still read
    # the tree blob damaged in the store
    _damage(store, tref.root.ref.cid, 3)
    for call in (lambda: v.get_tree_slice(store, tref),
                 lambda: v.get_at_path(store, tref, "a.txt")):
        with pytest.raises(bigblob.ErrCorrupt) as ei:
            call()
        assert ei.value.cid == tref.root.ref.cid
