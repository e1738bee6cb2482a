"""glfs.Machine.verify_tree: the fsck of everything a tree ref reaches, on a
tree of about 300 files of mixed sizes in three directories, clean and with
one store blob damaged."""
import pytest

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
BIG = 2 * MIB + 1   # two blocks and an index node at the default block size


@pytest.fixture(scope="module")
def forest(O):
    """(machine, tree ref, {cid: ctext}, {path: file ref}), posted once
    through the mirror; the tests work on copies of the blob dict."""
    from glfs_amd import bigblob, glfs
    m = glfs.Machine()
    store = bigblob.MemStore(m.block_size)
    sizes = {"empty": 0, "one": 1, "k16m": 16 * KIB - 1, "k16": 16 * KIB, "k16p": 16 * KIB + 1,
             "mid": 300000, "big": BIG}
    for i in range(200):
        sizes[f"f{i:03d}"] = 2 + (i * 7919) % 40000
    for i in range(60):
        sizes[f"sub/s{i:02d}"] = 3 + (i * 104729) % 70000
    for i in range(35):
        sizes[f"sub/nested/n{i:02d}"] = 5 + (i * 1299709) % 20000
    paths = sorted(sizes)
    stream = O.fill_splitmix(sum(sizes.values()), 77)
    blobs, o = [], 0
    for p in paths:
        blobs.append(stream[o:o + sizes[p]])
        o += sizes[p]
    assert len(set(blobs)) == len(blobs)   # distinct contents: one store blob each
    refs = dict(zip(paths, m.post_blobs(store, blobs)))
    tree = m.post_tree_map(store, refs)
    assert tree.type == glfs.TYPE_TREE
    return m, tree, dict(store.blobs), refs


def _store(forest):
    from glfs_amd import bigblob
    m, tree, blobs, refs = forest
    s = bigblob.MemStore(m.block_size)
    s.blobs = dict(blobs)
    return m, tree, s, refs


def _damage(store, cid, at=3):
    b = bytearray(store.blobs[cid])
    b[at % len(b)] ^= 0x20
    store.blobs[cid] = bytes(b)


def test_clean_tree_counts_every_blob(gpu, forest, monkeypatch):
    """The number of blobs the store holds for the tree: 302 files of one
    block or none, three blobs of the two-block file, three tree blobs; and
    the walk batches: at most 2 open_blobs calls (blobs, trees) per tree
    level and 64 MiB."""
    from glfs_amd import bigblob
    m, tree, store, refs = _store(forest)
    assert len(refs) == 302 and len(store) == 301 + 3 + 3
    calls = []
    real = bigblob.open_blobs

    def counted(ctexts, *a, **kw):
        calls.append(sum(len(c) for c in ctexts))
        return real(ctexts, *a, **kw)

    monkeypatch.setattr(bigblob, "open_blobs", counted)
    assert m.verify_tree(store, tree) == len(store)
    depth = 3                                   # root, sub, sub/nested
    groups = -(-sum(calls) // (64 * MIB))       # 1: the tree holds a few MiB
    assert groups == 1
    assert 1 <= len(calls) <= depth * 2 * groups, calls
    # a blob ref is its own walk: one object
    assert m.verify_tree(store, refs["mid"]) == 1
    assert m.verify_tree(store, refs["big"]) == 3
    assert m.verify_tree(store, refs["empty"]) == 1


def _victims(forest):
    from glfs_amd import bigblob
    m, tree, store, refs = _store(forest)
    sub = m.get_at_path(store, tree, "sub")
    second = bigblob._tree_levels(store.get, refs["big"].root)[-1][1]
    return {"root file": ("f017", refs["f017"].root.ref.cid),
            "nested file": ("sub/nested/n03", refs["sub/nested/n03"].root.ref.cid),
            "subtree blob": ("sub", sub.root.ref.cid),
            "second block": ("big", second.cid)}


@pytest.mark.parametrize("what", ["root file", "nested file", "subtree blob", "second block"])
def test_damage_is_found_with_its_path(gpu, forest, what):
    from glfs_amd import bigblob
    path, cid = _victims(forest)[what]
    m, tree, store, refs = _store(forest)
    _damage(store, cid)
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        m.verify_tree(store, tree)
    e = ei.value
    assert e.cid == cid
    assert e.path == path
    assert e.status & gpu.GLFSX_BAD_CID
    # Machine.verify, as before, sees only the tree blob itself
    assert m.verify(store, tree) == 1


def test_first_bad_blob_in_walk_order(gpu, forest):
    """Two damaged blobs: the one nearer the root is reported, and among the
    entries of one directory the first by name."""
    from glfs_amd import bigblob
    v = _victims(forest)
    m, tree, store, refs = _store(forest)
    _damage(store, v["nested file"][1])
    _damage(store, v["root file"][1])
    _damage(store, refs["f100"].root.ref.cid)
    with pytest.raises(bigblob.ErrCorrupt) as ei:
        m.verify_tree(store, tree)
    assert ei.value.path == "f017" and ei.value.cid == v["root file"][1]
