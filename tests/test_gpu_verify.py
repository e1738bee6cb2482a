"""The verified read through the Python mirror: Machine.verify (fsck),
read_all / _tree_levels with a salt, Sync into a pre-hashed store with
verify=True, and glfs.Machine.verify -- on clean trees and on stores with one
blob overwritten.  Expected posts and CIDs come from the oracle."""
import pytest

pytestmark = pytest.mark.gpu

SALT = bytes(range(7, 39))
MiB = 1 << 20
DEEP = (1024, 1024 * 16 * 16 + 1)   # depth 3 at bf 16: 257 data blocks, 17 + 2 + 1 nodes
FLAT = (MiB, 3 * MiB)               # depth 1


@pytest.fixture(autouse=True)
def _auto_route(gpu):
    gpu.set_open_route(0)
    yield
    gpu.set_open_route(0)


@pytest.fixture(scope="module")
def trees(O):
    """{shape: (data, root, {cid: ctext}, oracle posts)}, created once; the
    tests work on copies of the blob dict."""
    from glfs_amd import bigblob
    out = {}
    for bs, size in (DEEP, FLAT, (1024, 0), (1024, 700)):
        data = O.fill_splitmix(size, size + 3)
        store = bigblob.MemStore(bs)
        root = bigblob.Machine(block_size=bs).create(store, SALT, data)
        want_root, _, _, posts = O.create(data, bs, salt=SALT)
        assert root.ref.marshal_binary() == want_root
        out[(bs, size)] = (data, root, dict(store.blobs), posts)
    return out


def _store(trees, shape):
    from glfs_amd import bigblob
    data, root, blobs, posts = trees[shape]
    s = bigblob.MemStore(shape[0])
    s.blobs = dict(blobs)
    return data, root, s, posts


def _damage(store, cid, at=3):
    b = bytearray(store.blobs[cid])
    b[at % len(b)] ^= 0x20
    store.blobs[cid] = bytes(b)


@pytest.mark.parametrize("shape", [DEEP, FLAT, (1024, 0), (1024, 700)])
def test_clean_tree(gpu, O, trees, shape):
    from glfs_amd import bigblob
    data, root, store, posts = _store(trees, shape)
    m = bigblob.Machine(block_size=shape[0])
    assert m.verify(store, root, salt=SALT) == len(posts)
    assert m.verify(store, root) == len(posts)            # CIDs only
    assert bigblob.read_all(store, root, salt=SALT) == data
    assert bigblob.read_all(store, root) == data
    with pytest.raises(bigblob.ErrCorrupt):               # another blob's salt
        m.verify(store, root, salt=bytes(32))


@pytest.mark.parametrize("level", [0, 1, 3])
def test_overwritten_blob(gpu, O, trees, level):
    from glfs_amd import bigblob
    data, root, store, _ = _store(trees, DEEP)
    m = bigblob.Machine(block_size=DEEP[0])
    levels = bigblob._tree_levels(store.get, root)
    assert [len(lv) for lv in levels] == [1, 2, 17, 257]
    j = {0: 200, 1: 11, 3: 0}[level]
    victim = levels[3 - level][j]
    _damage(store, victim.cid, at=70)
    for call in (lambda: m.verify(store, root, salt=SALT), lambda: m.verify(store, root),
                 lambda: bigblob.read_all(store, root, salt=SALT)):
        with pytest.raises(bigblob.ErrCorrupt) as ei:
            call()
        assert (ei.value.cid, ei.value.level) == (victim.cid, level)
        assert ei.value.status & 1
        if level == 0:
            assert ei.value.index == j
    if level == 0:   # unchanged: without a salt the damaged block comes back as data
        got = bigblob.read_all(store, root)
        assert len(got) == len(data) and got != data
        assert got[:j * 1024] == data[:j * 1024] and got[(j + 1) * 1024:] == data[(j + 1) * 1024:]


def test_empty_blob_with_bytes_under_its_cid(gpu, O, trees):
    from glfs_amd import bigblob
    _, root, store, _ = _store(trees, (1024, 0))
    store.blobs[root.ref.cid] = b"x"
    m = bigblob.Machine(block_size=1024)
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        m.verify(store, root, salt=SALT)
    assert (ei.value.cid, ei.value.status) == (root.ref.cid, 1)
    dst = bigblob.MemStore(1024)
    with pytest.raises(bigblob.ErrCorrupt):
        m.sync(dst, store, root, verify=True)
    assert len(dst) == 0


def _reachable(store, root):
    from glfs_amd import bigblob
    return [r.cid for lv in bigblob._tree_levels(store.get, root) for r in lv]


def test_sync_verify_refuses_damaged_source(gpu, O, trees):
    from glfs_amd import bigblob
    _, root, src, _ = _store(trees, FLAT)
    cids = _reachable(src, root)
    victim = cids[2]                      # data block 1
    _damage(src, victim, at=12345)
    m = bigblob.Machine(block_size=MiB)
    dst = bigblob.NativeStore(MiB, mode="trust")
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        m.sync(dst, src, root, verify=True)
    assert (ei.value.cid, ei.value.level, ei.value.status) == (victim, 0, 1)
    assert not dst.exists(root.ref.cid)
    for cid in cids:                      # whatever got there hashes to its CID
        if dst.exists(cid):
            assert O.blake3(dst.get(cid)) == cid
    # the unverified copy is what this guards against: the bytes land under the CID
    dst2 = bigblob.NativeStore(MiB, mode="trust")
    m.sync(dst2, src, root)
    assert O.blake3(dst2.get(victim)) != victim


@pytest.mark.parametrize("shape", [DEEP, FLAT, (1024, 0)])
def test_sync_verify_clean(gpu, O, trees, shape, monkeypatch):
    from glfs_amd import bigblob
    _, root, src, _ = _store(trees, shape)
    monkeypatch.setattr(bigblob, "SYNC_VERIFY_BYTES", 8 * shape[0])   # several batches
    m = bigblob.Machine(block_size=shape[0])
    a, b = bigblob.MemStore(shape[0]), bigblob.MemStore(shape[0])
    m.sync(a, src, root, verify=True)
    m.sync(b, src, root)
    assert a.log == b.log and a.blobs == b.blobs          # same posts, same order
    na, nb = (bigblob.NativeStore(shape[0], mode="trust") for _ in range(2))
    m.sync(na, src, root, verify=True)
    m.sync(nb, src, root)
    cids = set(_reachable(src, root))
    assert len(na) == len(nb) == len(cids)
    assert all(na.exists(c) and nb.exists(c) for c in cids)


def test_glfs_verify(gpu, O):
    from glfs_amd import bigblob, glfs
    s = bigblob.MemStore(2 << 20)
    m = glfs.Machine()
    blob = m.post_blob(s, O.fill_splitmix(5000, 9))
    tree = m.post_tree_map(s, {"a.bin": blob, "b.txt": m.post_blob(s, b"hello")})
    assert m.verify(s, blob) == 1
    assert m.verify(s, tree) == 1
    for ref in (blob, tree):
        _damage(s, ref.root.ref.cid, at=1)
        with pytest.raises(bigblob.ErrCorrupt) as ei:
            m.verify(s, ref)
        assert ei.value.cid == ref.root.ref.cid
