"""Compare: what two objects have in common and what each has alone.

Reference: compare.go:19-124 (blobcache/glfs, Go).  Compare of two trees
matches their entries by name, recurses into matched subtrees and posts up to
three new trees: the entries only the left one has, those only the right one
has, and those both have.

Quirk kept for parity: compareTrees calls forEachInBoth(rTree, lTree, ...)
(compare.go:56), so inside its callback `lEnt` is the RIGHT tree's entry and
`rEnt` the left tree's.  With X the left argument and Y the right one:

  Left  = X's unmatched entries; for a matched pair that differs, Y's whole
          entry; for a matched pair of trees, (Y's mode, the name, sub.left)
  Right = Y's unmatched entries; X's whole entry of a differing pair;
          (X's mode, the name, sub.right)
  Both  = Y's whole entry of an equal pair; (Y's mode, the name, sub.both)

where sub = Compare(Y's ref, X's ref): the sides swap again one level down.

Two routes give the same refs and the same store contents:

  the entry route   a transcription of compare.go over get_tree_slice's
                    entries and post_tree_slice: any tree, any cid form.
  the column route  for a pair of trees whose every line the native decoder
                    vouches for: decode on the GPU, glfsx_tree_join_device,
                    the three outputs assembled by glfsx_tree_select_device
                    and encoded by glfsx_tree_encode_device.  No TreeEntry is
                    built; the host sees the refs of the matched subtree pairs
                    (to recurse) and each output's roots column (for
                    TreeWriter.Put's ExistsUnit check).
"""
from __future__ import annotations

import ctypes
from typing import Optional

from . import _native as N
from . import bigblob
from . import glfs
from . import tree as T
from .glfs import Diff

MAX_ENTS = 10 ** 6   # compare.go:31,35: GetTreeSlice(ctx, src, ref, 1e6)
COUNT_BYTES = 4 << 20   # trees up to this size have their lines counted on the host


def compare(machine: "glfs.Machine", dst, src, left: glfs.Ref, right: glfs.Ref,
            cid_json=T.cid_json_hex, cid_from_json=T._cid_from_json) -> Diff:
    """compare.go:19-50 Compare."""
    if left.type != right.type:
        return Diff(left, right, None)
    if left.type != glfs.TYPE_TREE:
        if left.equals(right):
            return Diff(None, None, left)
        return Diff(left, right, None)
    kw = machine._read_kw(glfs.TYPE_TREE)
    xb = bigblob.read_all(src, left.root, **kw)
    yb = bigblob.read_all(src, right.root, **kw)
    default_cid = cid_json is T.cid_json_hex and cid_from_json is T._cid_from_json
    # Enough entries for the column route?  Canonical lines hold no newline
    # but their last byte, so the newlines of small trees are counted here;
    # large ones are counted by the decoder (_compare_columns asks again).
    few = len(xb) + len(yb) <= COUNT_BYTES and (
        xb.count(b"\n") + yb.count(b"\n") < machine.COMPARE_DEVICE_MIN)
    if default_cid and not few:
        d = _compare_columns(machine, dst, src, xb, yb, cid_json, cid_from_json)
        if d is not None:
            return d
    x = T.read_tree_bytes(xb, cid_from_json)[:MAX_ENTS]
    y = T.read_tree_bytes(yb, cid_from_json)[:MAX_ENTS]
    return _compare_entries(machine, dst, src, x, y, cid_json, cid_from_json)


# -------------------------------------------------------------- entry route
def _compare_entries(machine, dst, src, l_tree, r_tree, cid_json, cid_from_json) -> Diff:
    """compare.go:52-104 compareTrees."""
    only_left = [e for e in l_tree if T.lookup(r_tree, e.name) is None]    # onlyInFirst
    only_right = [e for e in r_tree if T.lookup(l_tree, e.name) is None]
    both = []
    for l_ent in r_tree:               # forEachInBoth(rTree, lTree, ...): swapped
        r_ent = T.lookup(l_tree, l_ent.name)
        if r_ent is None:
            continue
        d = compare(machine, dst, src, l_ent.ref, r_ent.ref, cid_json, cid_from_json)
        if d.left is not None:
            only_left.append(T.TreeEntry(l_ent.name, l_ent.file_mode, d.left))
        if d.right is not None:
            only_right.append(T.TreeEntry(r_ent.name, r_ent.file_mode, d.right))
        if d.both is not None:
            both.append(T.TreeEntry(l_ent.name, l_ent.file_mode, d.both))
    post = lambda ents: T.post_tree(machine, dst, list(ents), cid_json) if ents else None
    left = post(only_left)
    right = post(only_right)
    return Diff(left, right, post(both))


# ------------------------------------------------------------- column route
def _struct(c: T.TreeColumns, n: int) -> N.glfsx_tree_cols:
    p = lambda t: t.data_ptr() or None
    return N.glfsx_tree_cols(n, p(c.names), p(c.name_offs), p(c.modes), p(c.types),
                             p(c.type_offs), p(c.roots), p(c.sizes), p(c.block_sizes),
                             p(c.status))


def _decode(torch, data: bytes, stream) -> Optional[T.TreeColumns]:
    """The tree's columns on the device, or None when a line is not one the
    decoder vouches for, or a name holds a '/' (PostTree would split it into
    a subdirectory, tree.go:205-216)."""
    if data:
        d = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        c = T.decode_lines_device(d.data_ptr(), len(data), stream)
    else:
        c = T.decode_lines_device(None, 0, stream)
    if c.n_bad or bool((c.names == 0x2F).any()):
        return None
    return c


def select(torch, a: N.glfsx_tree_cols, b: N.glfsx_tree_cols, sel, stream) -> T.TreeColumns:
    """glfsx_tree_select_device: the entries sel names (v >= 0: a's entry v,
    v < 0: b's entry -1 - v) as new device columns."""
    k = int(sel.numel())
    counts = (ctypes.c_uint64 * 2)()
    ra, rb = ctypes.byref(a), ctypes.byref(b)
    nul = [None, 0, None, None, None, 0, None, None, None, None, None]
    N.check(N.lib.glfsx_tree_select_device(ra, rb, sel.data_ptr() or None, k, *nul, 0, counts,
                                           stream))
    nl, tl = counts[0], counts[1]
    e = lambda m, dt: torch.empty(m, dtype=dt, device="cuda")
    c = T.TreeColumns(k, e(nl, torch.uint8), e(k + 1, torch.int64), e(k, torch.int32),
                      e(tl, torch.uint8), e(k + 1, torch.int64), e(64 * k, torch.uint8),
                      e(k, torch.int64), e(k, torch.int64), e(k, torch.int32), 0, False)
    p = lambda t: t.data_ptr() or None
    N.check(N.lib.glfsx_tree_select_device(
        ra, rb, p(sel), k, p(c.names), nl, p(c.name_offs), p(c.modes), p(c.types), tl,
        p(c.type_offs), p(c.roots), p(c.sizes), p(c.block_sizes), p(c.status), k, counts, stream))
    return c


def _check_exists(dst, c: T.TreeColumns) -> None:
    """TreeWriter.Put's ExistsUnit check (tree.go:306-308) of every entry of
    device columns, over the downloaded roots column: one store call per
    distinct CID (nothing is posted between the checks of one tree), and the
    error names the first entry whose CID dst lacks."""
    roots = c.roots.cpu().numpy().tobytes()
    cids = [roots[o:o + 32] for o in range(0, len(roots), 64)]
    missing = {cid for cid in set(cids) if not T.exists_unit(dst, cid)}
    if not missing:
        return
    import numpy as np
    i = next(k for k, cid in enumerate(cids) if cid in missing)
    h = lambda t: t.cpu().numpy()
    one = lambda col, offs: h(col)[int(offs[i]):int(offs[i + 1])].tobytes().decode(
        "utf-8", "surrogateescape")
    te = T.TreeEntry(one(c.names, c.name_offs), int(h(c.modes).view(np.uint32)[i]), glfs.Ref(
        one(c.types, c.type_offs),
        bigblob.Root(bigblob.Ref(cids[i], roots[64 * i + 32:64 * i + 64]),
                     int(c.sizes[i]), int(c.block_sizes[i]))))
    raise T.TreeError(f"adding tree ent {te} would violate referential integrity")


def _post_columns(machine, dst, torch, c: T.TreeColumns, stream) -> glfs.Ref:
    """PostTreeSlice of sorted device columns (tree.go:195-248): the
    ExistsUnit check of every entry -- before anything is written -- then the
    lines encoded on the device into a typed writer under the tree type's
    salt."""
    _check_exists(dst, c)
    p = lambda t: t.data_ptr() or None
    args = [c.n, p(c.names), p(c.name_offs), p(c.modes), p(c.types), p(c.type_offs), p(c.roots),
            p(c.sizes), p(c.block_sizes)]
    total = ctypes.c_uint64()
    N.check(N.lib.glfsx_tree_encode_device(*args, None, 0, None, ctypes.byref(total), stream))
    lines = torch.empty(total.value, dtype=torch.uint8, device="cuda")
    N.check(N.lib.glfsx_tree_encode_device(*args, lines.data_ptr(), total.value, None,
                                           ctypes.byref(total), stream))
    tw = machine.new_typed_writer(dst, glfs.TYPE_TREE)
    try:
        tw.bw.write_device(lines.data_ptr(), total.value, stream)
        return tw.finish()
    finally:
        tw.bw.close()


def _compare_columns(machine, dst, src, xb: bytes, yb: bytes, cid_json,
                     cid_from_json) -> Optional[Diff]:
    """compareTrees over device columns; None when the pair has to take the
    entry route."""
    import numpy as np
    import torch
    with torch.cuda.stream(_stream(machine, torch)):
        stream = torch.cuda.current_stream().cuda_stream
        cx = _decode(torch, xb, stream)
        cy = _decode(torch, yb, stream) if cx is not None else None
        if cx is None or cy is None:
            return None
        nx, ny = min(cx.n, MAX_ENTS), min(cy.n, MAX_ENTS)
        if nx + ny < machine.COMPARE_DEVICE_MIN:
            return None
        X, Y = _struct(cx, nx), _struct(cy, ny)
        dev = dict(device="cuda")
        xm = torch.empty(nx, dtype=torch.int64, **dev)
        ym = torch.empty(ny, dtype=torch.int64, **dev)
        xc = torch.empty(nx, dtype=torch.uint8, **dev)
        p = lambda t: t.data_ptr() or None
        N.check(N.lib.glfsx_tree_join_device(ctypes.byref(X), ctypes.byref(Y), p(xm), p(ym), p(xc),
                                             stream))
        ix = torch.arange(nx, dtype=torch.int64, **dev)
        iy = torch.arange(ny, dtype=torch.int64, **dev)
        # Y's entries' classes: their partners' (the class is symmetric)
        yc = torch.zeros(ny, dtype=torch.uint8, **dev)
        matched = ym >= 0
        yc[matched] = xc[ym[matched]]
        # the matched subtree pairs, in name order: their refs come to the host
        ti = torch.nonzero(xc == N.GLFSX_JOIN_TREES).flatten()
        tj = xm[ti]
        nt = int(ti.numel())
        subs = []
        if nt:
            host = lambda c, idx: (c.roots.view(-1, 64)[idx].cpu().numpy(), c.sizes[idx].tolist(),
                                   c.block_sizes[idx].tolist())
            (xr, xs, xbs), (yr, ys, ybs) = host(cx, ti), host(cy, tj)
            ref = lambda r, s, b, k: glfs.Ref(glfs.TYPE_TREE, bigblob.Root(
                bigblob.Ref(r[k, :32].tobytes(), r[k, 32:].tobytes()), s[k], b[k]))
            for k in range(nt):   # compare.go:57: Compare(lEnt.Ref, rEnt.Ref), lEnt the right tree's
                subs.append(compare(machine, dst, src, ref(yr, ys, ybs, k), ref(xr, xs, xbs, k),
                                    cid_json, cid_from_json))

        def has(field, where, n):
            """per entry of a side: it is a subtree pair whose sub-result has `field`"""
            m = torch.zeros(n, dtype=torch.bool, **dev)
            if nt:
                m[where] = torch.tensor([getattr(s, field) is not None for s in subs], **dev)
            return m

        def output(keep, sel_all, field, where):
            """The output of the kept entries (in one side's name order), the
            subtree pairs' rows patched with their sub-results."""
            sel = sel_all[keep]
            if int(sel.numel()) == 0:
                return None
            c = select(torch, X, Y, sel, stream)
            got = [(k, getattr(s, field)) for k, s in enumerate(subs)
                   if getattr(s, field) is not None]
            if got:
                pos = (torch.cumsum(keep, 0) - 1)[where[torch.tensor([k for k, _ in got], **dev)]]
                raw = np.frombuffer(b"".join(r.root.ref.cid + r.root.ref.dek for _, r in got),
                                    dtype=np.uint8).reshape(-1, 64).copy()
                c.roots.view(-1, 64)[pos] = torch.from_numpy(raw).cuda()
                c.sizes[pos] = torch.tensor([r.root.size for _, r in got], dtype=torch.int64, **dev)
                c.block_sizes[pos] = torch.tensor([r.root.block_size for _, r in got],
                                                  dtype=torch.int64, **dev)
            return _post_columns(machine, dst, torch, c, stream)

        ONLY, TREES, SAME, DIFF = (N.GLFSX_JOIN_ONLY, N.GLFSX_JOIN_TREES, N.GLFSX_JOIN_SAME,
                                   N.GLFSX_JOIN_DIFF)
        # Left, in X's order: X's own entry when unmatched, else Y's
        left = output((xc == ONLY) | (xc == DIFF) | ((xc == TREES) & has("left", ti, nx)),
                      torch.where(xc == ONLY, ix, -1 - xm), "left", ti)
        # Right, in Y's order: Y's own entry when unmatched, else X's
        right = output((yc == ONLY) | (yc == DIFF) | ((yc == TREES) & has("right", tj, ny)),
                       torch.where(yc == ONLY, -1 - iy, ym), "right", tj)
        # Both, in X's order: Y's entry
        both = output((xc == SAME) | ((xc == TREES) & has("both", ti, nx)), -1 - xm, "both", ti)
        return Diff(left, right, both)


def _stream(machine, torch):
    """The stream the column route's torch ops and library calls share."""
    s = getattr(machine, "_compare_stream", None)
    if s is None:
        s = machine._compare_stream = torch.cuda.Stream()
    return s
