"""Tree against tree on the GPU: glfsx_tree_join_device (k_tree_join) against
the host join, every output word; glfsx_tree_select_device (k_ts_len /
k_ts_write) against numpy indexing over the same columns; and Machine.compare
on both of its routes against a restatement of compare.go written here.  Guard
bytes around every device output."""
import ctypes
import random

import numpy as np
import pytest

import tree_join_cases as J

pytestmark = pytest.mark.gpu

GUARD = 64


class _Out:
    """A device output of nbytes with GUARD bytes of 0xA5 either side."""

    def __init__(self, torch, nbytes):
        self.t = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.n = nbytes
        self.ptr = self.t.data_ptr() + GUARD

    def host(self, dtype=np.uint8):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + self.n:] == 0xA5).all(), "guard"
        return h[GUARD:GUARD + self.n].copy().view(dtype)

    def untouched(self):
        return bool((self.t == 0xA5).all())


def _place(torch, data: np.ndarray, shift=0, at_end=False):
    """The bytes in HBM `shift` bytes past a 16-byte boundary; at_end: their
    last byte is the last byte of the tensor (a 512-byte multiple, the
    allocator's granule), so a read past them leaves the tensor."""
    n = data.size
    if at_end:
        size = -(-(n + 16) // 512) * 512
        shift = size - n
    else:
        size = shift + n + 32
    t = torch.full((size,), 0xEE, dtype=torch.uint8, device="cuda")
    if n:
        t[shift:shift + n] = torch.from_numpy(data.copy())
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


class _Dev:
    """A side's host columns (J.columns) in device memory and the
    glfsx_tree_cols over them; the name pool placed by _place."""

    def __init__(self, torch, N, cols, shift=0, at_end=False):
        self.keep = []
        ptr = {}
        for k in J.COLS:
            h = cols[k].view(np.uint8)
            if k == "names":
                t, p = _place(torch, h, shift, at_end)
            else:
                t, p = _place(torch, h, 0)
            self.keep.append(t)
            ptr[k] = p
        self.struct = N.glfsx_tree_cols(cols["n"], *[ptr[k] for k in J.COLS])
        self.ref = ctypes.byref(self.struct)


def _host_join(N, ca, cb):
    sa, sb = J.host_struct(N, ca), J.host_struct(N, cb)
    am, bm = np.empty(ca["n"], np.int64), np.empty(cb["n"], np.int64)
    ac = np.empty(ca["n"], np.uint8)
    assert N.lib.glfsx_tree_join(ctypes.byref(sa), ctypes.byref(sb), am.ctypes.data,
                                 bm.ctypes.data, ac.ctypes.data) == 0
    return am, bm, ac


def _device_join(torch, N, ca, cb, place):
    da, db = _Dev(torch, N, ca, **place), _Dev(torch, N, cb, **place)
    am, bm, ac = _Out(torch, 8 * ca["n"]), _Out(torch, 8 * cb["n"]), _Out(torch, ca["n"])
    torch.cuda.synchronize()
    rc = N.lib.glfsx_tree_join_device(da.ref, db.ref, am.ptr, bm.ptr, ac.ptr, None)
    torch.cuda.synchronize()
    assert rc == 0, N.last_error()
    return am.host(np.int64), bm.host(np.int64), ac.host()


PLACES = [dict(at_end=True)] + [dict(shift=s) for s in (1, 7, 15)]
JOIN_CASES = J.special_cases() + J.size_cases()


@pytest.mark.parametrize("case", JOIN_CASES, ids=[c[0] for c in JOIN_CASES])
def test_join_device_equals_host(gpu, case):
    """Every word of the three outputs, the name pools once ending at the
    end of their tensor and once 1-15 bytes past a 16-byte boundary."""
    import torch
    _, a, b = case
    ca, cb = J.columns(a), J.columns(b)
    want = _host_join(gpu, ca, cb)
    for w, py in zip(want, J.py_join(a, b)):   # the host form is itself the dict's
        assert np.array_equal(w, py)
    rng = random.Random(len(a) * 1009 + len(b))
    for place in (PLACES[0], PLACES[1 + rng.randrange(3)]):
        got = _device_join(torch, gpu, ca, cb, place)
        for g, w, name in zip(got, want, ("a_match", "b_match", "a_class")):
            assert np.array_equal(g, w), (name, place)


def test_join_device_big(gpu):
    """70 000 x 50 000: hundreds of workgroups, the boundary between the
    sides inside one."""
    import torch
    _, a, b = J.big_case()
    ca, cb = J.columns(a), J.columns(b)
    want = _host_join(gpu, ca, cb)
    assert (want[0] >= 0).sum() > 10000
    got = _device_join(torch, gpu, ca, cb, dict(at_end=True))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_join_device_nullable_outputs_and_empty_sides(gpu):
    import torch
    a, b = J.sized(257, 300, 5)
    ca, cb = J.columns(a), J.columns(b)
    want = _host_join(gpu, ca, cb)
    da, db = _Dev(torch, gpu, ca, shift=3), _Dev(torch, gpu, cb, shift=5)
    for k in range(3):
        outs = [_Out(torch, 8 * 257), _Out(torch, 8 * 300), _Out(torch, 257)]
        ptrs = [o.ptr if i == k else None for i, o in enumerate(outs)]
        torch.cuda.synchronize()
        assert gpu.lib.glfsx_tree_join_device(da.ref, db.ref, *ptrs, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(outs[k].host((np.int64, np.int64, np.uint8)[k]), want[k])
        assert all(o.untouched() for i, o in enumerate(outs) if i != k)
    none = gpu.glfsx_tree_cols()
    assert gpu.lib.glfsx_tree_join_device(ctypes.byref(none), ctypes.byref(none), None, None, None,
                                          None) == 0
    bad = gpu.glfsx_tree_cols(3)   # entries without a name column
    assert gpu.lib.glfsx_tree_join_device(ctypes.byref(bad), db.ref, None, None, None,
                                          None) == gpu.GLFSX_E_ARG


def test_join_device_unsorted_side(gpu):
    """A broken precondition: the results are unspecified, but the guards
    hold and every match is -1 or an index of the other side."""
    import torch
    _, a, b = J.unsorted_case()
    am, bm, ac = _device_join(torch, gpu, J.columns(a), J.columns(b), dict(at_end=True))
    assert ((am >= -1) & (am < len(b))).all() and ((bm >= -1) & (bm < len(a))).all()
    assert (ac <= J.DIFF).all()


# --------------------------------------------------------------------- select
def _select_sides():
    """Two sides with names of 0 and 300 bytes among the numbered ones, and
    distinct modes and status words."""
    rng = random.Random(11)
    a = J.side(J.numbered(range(0, 400, 2), rng) + [J.entry(b"", mode=5), J.entry(b"y" * 300, b"tree", 3)])
    b = J.side(J.numbered(range(1, 300, 3), rng) + [J.entry(b"z" * 300, b"", 4), J.entry(b"", b"x" * 40)])
    ca, cb = J.columns(a), J.columns(b)
    ca["status"] = np.arange(len(a), dtype=np.uint32) * 3 + 1
    cb["status"] = np.arange(len(b), dtype=np.uint32) * 5 + 2
    return ca, cb


def _np_select(ca, cb, sel):
    """The selected entries by numpy indexing over the two sides' columns."""
    idx = np.where(sel >= 0, sel, ca["n"] + (-1 - sel)).astype(np.int64)
    out = {}
    for k in ("modes", "sizes", "block_sizes", "status"):
        out[k] = np.concatenate([ca[k], cb[k]])[idx]
    out["roots"] = np.concatenate([ca["roots"], cb["roots"]]).reshape(-1, 64)[idx].reshape(-1)
    for s, o in (("names", "name_offs"), ("types", "type_offs")):
        parts = [c[s][int(c[o][i]):int(c[o][i + 1])] for c in (ca, cb) for i in range(c["n"])]
        picked = [parts[i] for i in idx.tolist()]
        out[s] = np.concatenate(picked) if picked else np.empty(0, np.uint8)
        out[o] = np.cumsum([0] + [p.size for p in picked], dtype=np.uint64)
    return out


DT = dict(names=np.uint8, name_offs=np.uint64, modes=np.uint32, types=np.uint8,
          type_offs=np.uint64, roots=np.uint8, sizes=np.uint64, block_sizes=np.uint64,
          status=np.uint32)


def _device_select(torch, N, da, db, sel, want, caps=None):
    k = sel.size
    o = {c: _Out(torch, want[c].nbytes) for c in J.COLS}
    ncap, tcap, kcap = caps or (want["names"].size, want["types"].size, k)
    d_sel = torch.from_numpy(sel.copy()).cuda() if k else None
    counts = (ctypes.c_uint64 * 2)(77, 77)
    torch.cuda.synchronize()
    rc = N.lib.glfsx_tree_select_device(
        da.ref, db.ref, d_sel.data_ptr() if k else None, k, o["names"].ptr, ncap,
        o["name_offs"].ptr, o["modes"].ptr, o["types"].ptr, tcap, o["type_offs"].ptr,
        o["roots"].ptr, o["sizes"].ptr, o["block_sizes"].ptr, o["status"].ptr, kcap, counts, None)
    torch.cuda.synchronize()
    return rc, list(counts), o


def _sel_variants(k, na, nb):
    rng = random.Random(k)
    both = lambda i: (i % na) if i % 2 == 0 else -1 - (i % nb)
    return {
        "all-a": np.array([(7 * i) % na for i in range(k)], dtype=np.int64).reshape(k),
        "all-b": np.array([-1 - ((5 * i) % nb) for i in range(k)], dtype=np.int64).reshape(k),
        "alternating": np.array([both(i) for i in range(k)], dtype=np.int64).reshape(k),
        "repeats": np.array([rng.choice((0, na - 1, -1, -nb, 3)) for _ in range(k)],
                            dtype=np.int64).reshape(k),
        "descending": np.array(sorted((both(3 * i) for i in range(k)), reverse=True),
                               dtype=np.int64).reshape(k),
    }


@pytest.mark.parametrize("k", [0, 1, 255, 256, 257])
def test_select_device_equals_numpy(gpu, k):
    import torch
    ca, cb = _select_sides()
    da, db = _Dev(torch, gpu, ca, at_end=True), _Dev(torch, gpu, cb, shift=9)
    for label, sel in _sel_variants(k, ca["n"], cb["n"]).items():
        want = _np_select(ca, cb, sel)
        rc, counts, o = _device_select(torch, gpu, da, db, sel, want)
        assert rc == 0, (label, gpu.last_error())
        assert counts == [want["names"].size, want["types"].size], label
        for c in J.COLS:
            assert np.array_equal(o[c].host(DT[c]), want[c]), (label, c)
        if k == 257 and label != "descending":   # the long and the empty names were among them
            lens = np.diff(want["name_offs"].astype(np.int64))
            assert lens.max() == 300 and lens.min() == 0, label
    # all outputs NULL: the counts only
    sel = _sel_variants(max(k, 1), ca["n"], cb["n"])["alternating"]
    want = _np_select(ca, cb, sel)
    counts = (ctypes.c_uint64 * 2)()
    d_sel = torch.from_numpy(sel.copy()).cuda()
    torch.cuda.synchronize()
    assert gpu.lib.glfsx_tree_select_device(da.ref, db.ref, d_sel.data_ptr(), sel.size, None, 0,
                                            None, None, None, 0, None, None, None, None, None, 0,
                                            counts, None) == 0
    assert list(counts) == [want["names"].size, want["types"].size]


def test_select_device_capacity_one_short_writes_nothing(gpu):
    import torch
    ca, cb = _select_sides()
    da, db = _Dev(torch, gpu, ca, shift=1), _Dev(torch, gpu, cb, at_end=True)
    sel = _sel_variants(257, ca["n"], cb["n"])["alternating"]
    want = _np_select(ca, cb, sel)
    nl, tl = want["names"].size, want["types"].size
    for caps in ((nl - 1, tl, 257), (nl, tl - 1, 257), (nl, tl, 256)):
        rc, counts, o = _device_select(torch, gpu, da, db, sel, want, caps)
        assert rc == gpu.GLFSX_E_ARG, caps
        assert counts == [nl, tl], caps
        assert all(x.untouched() for x in o.values()), caps


def test_select_device_sel_out_of_range_writes_nothing(gpu):
    import torch
    ca, cb = _select_sides()
    da, db = _Dev(torch, gpu, ca, shift=2), _Dev(torch, gpu, cb, shift=13)
    good = _sel_variants(300, ca["n"], cb["n"])["alternating"]
    want = _np_select(ca, cb, good)
    for at, v in ((0, ca["n"]), (299, -1 - cb["n"]), (255, 1 << 62), (256, -(1 << 63))):
        sel = good.copy()
        sel[at] = v
        rc, counts, o = _device_select(torch, gpu, da, db, sel, want)
        assert rc == gpu.GLFSX_E_ARG and "sel" in gpu.last_error(), (at, v)
        assert all(x.untouched() for x in o.values()), (at, v)
    rc, counts, o = _device_select(torch, gpu, da, db, good, want)   # and the flag is gone again
    assert rc == 0 and np.array_equal(o["names"].host(), want["names"])


# -------------------------------------------------------------------- compare
def restated_compare(m, dst, src, left, right):
    """compare.go:21-50 Compare, line by line, as (left, right, both)."""
    from glfs_amd import glfs
    if left.type != right.type:                                   # :22-27
        return (left, right, None)
    if left.type == glfs.TYPE_TREE:                               # :29
        l_tree = m.get_tree_slice(src, left, 10 ** 6)             # :31
        r_tree = m.get_tree_slice(src, right, 10 ** 6)            # :35
        return restated_compare_trees(m, dst, src, l_tree, r_tree)  # :39
    if left.equals(right):                                        # :41
        return (None, None, left)                                 # :42
    return (left, right, None)                                    # :44-47


def restated_compare_trees(m, dst, src, l_tree, r_tree):
    """compare.go:52-104 compareTrees, with :56's swapped arguments."""
    from glfs_amd import tree as T
    only_in_first = lambda a, b: [e for e in a if T.lookup(b, e.name) is None]   # :106-113
    only_left = only_in_first(l_tree, r_tree)                     # :53
    only_right = only_in_first(r_tree, l_tree)                    # :54
    both = []                                                     # :55

    def fn(l_ent, r_ent):                                         # :56-82
        d_left, d_right, d_both = restated_compare(m, dst, src, l_ent.ref, r_ent.ref)   # :57
        if d_left is not None:                                    # :61-67
            only_left.append(T.TreeEntry(l_ent.name, l_ent.file_mode, d_left))
        if d_right is not None:                                   # :68-74
            only_right.append(T.TreeEntry(r_ent.name, r_ent.file_mode, d_right))
        if d_both is not None:                                    # :75-81
            both.append(T.TreeEntry(l_ent.name, l_ent.file_mode, d_both))

    for a_ent in r_tree:                                          # :56 forEachInBoth(rTree, lTree, fn)
        b_ent = T.lookup(l_tree, a_ent.name)                      # :115-124
        if b_ent is not None:
            fn(a_ent, b_ent)
    out = []
    for ents in (only_left, only_right, both):                    # :88-102
        out.append(m.post_tree_slice(dst, ents) if len(ents) > 0 else None)
    return tuple(out)


def _copy_store(s):
    from glfs_amd import bigblob
    c = bigblob.MemStore(s.max_size())
    c.blobs = dict(s.blobs)
    return c


@pytest.fixture(scope="module")
def world(gpu):
    """One store holding every tree and blob of the compare cases, and the
    cases as name -> (left ref, right ref)."""
    from glfs_amd import bigblob, glfs, tree as T
    m = glfs.Machine()
    src = bigblob.MemStore(m.block_size)
    blobs = m.post_blobs(src, [b"blob %d" % i for i in range(900)])
    ent = lambda name, ref, mode=None: T.TreeEntry(name, T.get_file_mode(ref) if mode is None
                                                   else mode, ref)
    post = lambda ents: m.post_tree(src, list(ents))

    def flat(extra_x=(), extra_y=()):
        x = [ent("L%04d" % i, blobs[i]) for i in range(200)]
        y = [ent("R%04d" % i, blobs[200 + i]) for i in range(150)]
        x += [ent("D%04d" % i, blobs[350 + i]) for i in range(100)]
        y += [ent("D%04d" % i, blobs[450 + i]) for i in range(100)]
        x += [ent("E%04d" % i, blobs[550 + i], 0o644) for i in range(150)]
        y += [ent("E%04d" % i, blobs[550 + i], 0o600) for i in range(150)]   # equal refs, other modes
        return post(x + list(extra_x)), post(y + list(extra_y))

    cases = {"flat": flat()}
    # three matched subtree pairs, two levels deep
    deep_x = post([ent("only-x", blobs[700]), ent("same", blobs[701]), ent("diff", blobs[702])])
    deep_y = post([ent("only-y", blobs[703]), ent("same", blobs[701]), ent("diff", blobs[704])])
    subs_x, subs_y = [], []
    for k in range(3):
        sx = post([ent("a", blobs[710 + k]), ent("deep", deep_x, 0o700 | T.MODE_DIR),
                   ent("x%d" % k, blobs[720 + k])])
        sy = post([ent("a", blobs[710 + k] if k else blobs[730]), ent("deep", deep_y),
                   ent("y%d" % k, blobs[740 + k])])
        subs_x.append(ent("sub%d" % k, sx, 0o711 | T.MODE_DIR))
        subs_y.append(ent("sub%d" % k, sy))
    cases["subtrees"] = flat(subs_x, subs_y)
    empty = m.post_tree_map(src, {})
    cases["empty-subtrees"] = (post([ent("e", empty), ent("f", blobs[750])]),
                               post([ent("e", empty), ent("g", blobs[751])]))
    cases["same-subtree"] = (post([ent("s", deep_x), ent("f", blobs[750])]),
                             post([ent("s", deep_x, 0o700 | T.MODE_DIR)]))
    cases["subtree-against-blob"] = (post([ent("n", deep_x), ent("o", blobs[752])]),
                                     post([ent("n", blobs[753]), ent("o", deep_y)]))
    cases["identical"] = (cases["flat"][0], cases["flat"][0])
    cases["disjoint"] = (post([ent("a%d" % i, blobs[760 + i]) for i in range(20)]),
                         post([ent("b%d" % i, blobs[760 + i]) for i in range(30)]))
    cases["empty-against-tree"] = (empty, deep_y)
    cases["both-empty"] = (empty, empty)
    return m, src, cases, blobs


TREE_CASES = ["flat", "subtrees", "empty-subtrees", "same-subtree", "subtree-against-blob",
              "identical", "disjoint", "empty-against-tree", "both-empty"]


def _run(m, src, left, right, device_min):
    from glfs_amd import glfs
    dst = _copy_store(src)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(glfs.Machine, "COMPARE_DEVICE_MIN", device_min)
        d = m.compare(dst, src, left, right)
    return (d.left, d.right, d.both), dst


@pytest.mark.parametrize("name", TREE_CASES)
def test_compare_both_routes_equal_the_restatement(world, name):
    from glfs_amd import tree as T
    m, src, cases, _ = world
    left, right = cases[name]
    ref_dst = _copy_store(src)
    want = restated_compare(m, ref_dst, src, left, right)
    if name == "flat":
        sizes = [len(m.get_tree_slice(ref_dst, r)) for r in want]
        assert sizes == [300, 250, 150]   # 200 + 100, 150 + 100, 150
        assert {e.file_mode for e in m.get_tree_slice(ref_dst, want[2])} == {0o600}   # Y's modes
    if name == "empty-subtrees":
        assert want[2] is None   # nothing in common: the pair of empty subtrees vanished
        assert all("e" not in [e.name for e in m.get_tree_slice(ref_dst, r)] for r in want[:2])
    # the entry route
    got, dst = _run(m, src, left, right, 1 << 62)
    assert got == want and dst.blobs == ref_dst.blobs
    # the column route, at every depth; no entry list may be built
    with pytest.MonkeyPatch.context() as mp:
        def boom(*a, **k):
            raise AssertionError("the column route built an entry list")
        mp.setattr(T, "entries_from_columns", boom)
        mp.setattr(T, "read_tree_bytes", boom)
        got, dst = _run(m, src, left, right, 0)
    assert got == want and dst.blobs == ref_dst.blobs


def test_compare_non_trees(world):
    from glfs_amd import glfs
    m, src, cases, blobs = world
    tree = cases["flat"][0]
    dst = _copy_store(src)
    n = len(dst.blobs)
    assert m.compare(dst, src, tree, blobs[0]) == glfs.Diff(tree, blobs[0], None)
    assert m.compare(dst, src, blobs[0], tree) == glfs.Diff(blobs[0], tree, None)
    assert m.compare(dst, src, blobs[1], blobs[1]) == glfs.Diff(None, None, blobs[1])
    assert m.compare(dst, src, blobs[1], blobs[2]) == glfs.Diff(blobs[1], blobs[2], None)
    assert restated_compare(m, dst, src, tree, blobs[0]) == (tree, blobs[0], None)
    assert restated_compare(m, dst, src, blobs[1], blobs[1]) == (None, None, blobs[1])
    assert restated_compare(m, dst, src, blobs[1], blobs[2]) == (blobs[1], blobs[2], None)
    assert len(dst.blobs) == n   # nothing is posted


def _raw_tree(m, store, lines: bytes):
    from glfs_amd import glfs
    tw = m.new_typed_writer(store, glfs.TYPE_TREE)
    tw.write(lines)
    return tw.finish()


def test_compare_takes_the_entry_route_when_it_must(world):
    """A tree with a line the decoder does not vouch for, and one with a name
    that holds a '/', are compared over entries even with the threshold at
    0: the restatement's result."""
    from glfs_amd import compare as C, tree as T
    m, src, cases, blobs = world
    src = _copy_store(src)
    ents = [T.TreeEntry("a", 0o644, blobs[0]), T.TreeEntry("b", 0o644, blobs[1])]
    loose = b"".join(T.entry_json_line(e) for e in ents).replace(b',"mode"', b', "mode"', 1)
    slash = T.entry_json_line(T.TreeEntry("a/b", 0o644, blobs[2])) + T.entry_json_line(
        T.TreeEntry("c", 0o644, blobs[3]))
    other = m.post_tree(src, [T.TreeEntry("b", 0o644, blobs[1]), T.TreeEntry("c", 0o644, blobs[4])])
    for odd in (_raw_tree(m, src, loose), _raw_tree(m, src, slash)):
        for left, right in ((odd, other), (other, odd)):
            ref_dst = _copy_store(src)
            want = restated_compare(m, ref_dst, src, left, right)
            calls = []
            with pytest.MonkeyPatch.context() as mp:
                real = C._compare_entries
                mp.setattr(C, "_compare_entries", lambda *a: calls.append(1) or real(*a))
                got, dst = _run(m, src, left, right, 0)
            assert calls and got == want and dst.blobs == ref_dst.blobs


@pytest.mark.parametrize("device_min", [0, 1 << 62])
def test_compare_checks_referential_integrity(world, device_min):
    """TreeWriter.Put's ExistsUnit check (tree.go:306-308) on dst: an output
    entry whose CID dst lacks is a TreeError, and nothing is written."""
    from glfs_amd import bigblob, glfs, tree as T
    m, src, cases, _ = world
    left, right = cases["disjoint"]
    dst = bigblob.MemStore(m.block_size)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(glfs.Machine, "COMPARE_DEVICE_MIN", device_min)
        with pytest.raises(T.TreeError, match="name='a0'.*referential integrity"):
            m.compare(dst, src, left, right)
    assert len(dst.blobs) == 0


def test_compare_default_threshold_chooses_the_route(world):
    """With Machine.COMPARE_DEVICE_MIN as committed, a pair of trees with
    fewer entries goes over entries and a pair with more over columns."""
    from glfs_amd import compare as C, glfs
    m, src, cases, _ = world
    assert 50 < glfs.Machine.COMPARE_DEVICE_MIN <= 850
    for name, want_route in (("disjoint", "entries"), ("flat", "columns")):
        seen = []
        with pytest.MonkeyPatch.context() as mp:
            ents, cols = C._compare_entries, C._compare_columns
            mp.setattr(C, "_compare_entries", lambda *a: seen.append("entries") or ents(*a))
            mp.setattr(C, "_compare_columns", lambda *a: seen.append("columns") or cols(*a))
            d = m.compare(_copy_store(src), src, *cases[name])
        assert seen == [want_route], (name, seen)
        assert (d.left, d.right, d.both) == restated_compare(m, _copy_store(src), src, *cases[name])


def test_compare_on_a_verifying_machine(world):
    """A Machine made with_verify reads both trees with the verified read on
    either route: the same refs, and a flipped bit in a tree blob is
    ErrCorrupt, not a wrong diff."""
    from glfs_amd import bigblob, glfs
    m, src, cases, _ = world
    left, right = cases["subtrees"]
    want = restated_compare(m, _copy_store(src), src, left, right)
    mv = glfs.Machine(glfs.with_verify())
    for device_min in (0, 1 << 62):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(glfs.Machine, "COMPARE_DEVICE_MIN", device_min)
            d = mv.compare(_copy_store(src), src, left, right)
            assert (d.left, d.right, d.both) == want
            bad = _copy_store(src)
            ct = bytearray(bad.blobs[right.root.ref.cid])
            ct[len(ct) // 2] ^= 4
            bad.blobs[right.root.ref.cid] = bytes(ct)
            with pytest.raises(bigblob.ErrCorrupt):
                mv.compare(_copy_store(src), bad, left, right)
