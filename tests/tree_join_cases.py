"""Inputs shared by the join tests (tests/test_tree_join.py on the CPU,
tests/test_gpu_tree_join.py on the GPU): pairs of column sets, the yardstick
join as a Python dict over bytes names, and the columns as numpy arrays.  A
helper module, not a conftest.

An entry is (name, type, root, size, block_size, mode): bytes, bytes, 64
bytes, int, int, int.  A side is a list of entries sorted by name the way
strings.Compare sorts (Python's bytes order: unsigned, a prefix first)."""
import random

import numpy as np

ONLY, TREES, SAME, DIFF = 0, 1, 2, 3   # include/glfsx.h GLFSX_JOIN_*


def root(seed: int) -> bytes:
    return random.Random(seed).randbytes(64)


def entry(name: bytes, ty: bytes = b"blob", seed: int = 0, size: int = 10, bs: int = 1 << 21,
          mode: int = 0o644):
    return (name, ty, root(seed), size, bs, mode)


def side(entries):
    out = sorted(entries, key=lambda e: e[0])
    assert all(a[0] < b[0] for a, b in zip(out, out[1:])), "duplicate name"
    return out


def numbered(idx, rng, tag=0):
    """Entries named %07d for idx; type, ref and sizes drawn so that a name
    on both sides meets every class."""
    out = []
    for i in idx:
        ty = (b"blob", b"tree", b"tre", b"")[rng.randrange(4)]
        out.append((b"%07d" % i, ty, root(rng.randrange(3)), rng.randrange(2), 1 + rng.randrange(2),
                    rng.randrange(1 << 32)))
    return out


def sized(na, nb, seed):
    """na x nb entries out of one pool of names, about half of them shared."""
    rng = random.Random(seed)
    pool = range(max(na, nb, (na + nb) * 3 // 4) + 1)
    a = side(numbered(rng.sample(pool, na), rng))
    b = side(numbered(rng.sample(pool, nb), rng))
    return a, b


def _long(at: int, c: int) -> bytes:
    x = bytearray(b"x" * 300)
    x[at] = c
    return bytes(x)


def special_cases():
    """(label, A, B): the cases a word-wise, signed or off-by-one compare gets
    wrong, the ends of either side, and every class."""
    cases = []
    pre = [b"a", b"ab", b"ab\x00"]
    cases.append(("prefixes", side(entry(n, seed=1) for n in pre),
                  side(entry(n, seed=1) for n in (b"ab", b"ab\x00", b"ab\x00\x00", b"abc"))))
    cases.append(("high-byte", side(entry(n) for n in (b"a\x7f", b"a\x80", b"a\xff", b"\x80")),
                  side(entry(n) for n in (b"a\x80", b"a\x7e", b"\x7f", b"\x80", b"a\xfe"))))
    ats = (3, 4, 7, 8, 15, 16, 299)
    cases.append(("long-names",
                  side([entry(_long(at, ord("a"))) for at in ats] + [entry(b"x" * 300)]),
                  side([entry(_long(at, 0xE9)) for at in ats] + [entry(_long(8, ord("a")))]
                       + [entry(b"x" * 300), entry(b"x" * 299)])))
    cases.append(("long-names-all-match",
                  side([entry(_long(at, c)) for at in ats for c in (ord("a"), 0xE9)]),
                  side([entry(_long(at, c)) for at in ats for c in (ord("a"), 0xE9)])))
    cases.append(("empty-name", side([entry(b""), entry(b"a")]), side([entry(b""), entry(b"b")])))
    cases.append(("empty-name-one-side", side([entry(b""), entry(b"a")]), side([entry(b"a")])))
    mid = [entry(b"m%03d" % i) for i in range(300)]
    cases.append(("match-at-first", side([entry(b"a")] + mid[:150]), side([entry(b"a")] + mid[150:])))
    cases.append(("match-at-last", side(mid[:150] + [entry(b"z")]), side(mid[150:] + [entry(b"z")])))
    cases.append(("first-of-a-last-of-b", side([entry(b"k")] + [entry(b"m%d" % i) for i in range(9)]),
                  side([entry(b"a%d" % i) for i in range(9)] + [entry(b"k")])))
    cases.append(("no-match", side(mid[:150]), side(mid[150:])))
    cases.append(("all-match", side(mid), side(mid)))
    # classes: the pair of types, then refs equal but for one field
    r = root(5)
    flip = lambda k: r[:k] + bytes([r[k] ^ 1]) + r[k + 1:]
    a = [(b"c0", b"tree", r, 1, 2, 0), (b"c1", b"blob", r, 1, 2, 0), (b"c2", b"blob", r, 1, 2, 0),
         (b"c3", b"tre", r, 1, 2, 0), (b"c4", b"blob", r, 1, 2, 0), (b"c5", b"blob", r, 1, 2, 0),
         (b"c6", b"blob", r, 1, 2, 0), (b"c7", b"blob", r, 1, 2, 0), (b"c8", b"tree", r, 1, 2, 0),
         (b"c9", b"tree", r, 1, 2, 0), (b"d0", b"", r, 1, 2, 0), (b"d1", b"blob", r, 1, 2, 7)]
    b = [(b"c0", b"tree", r, 1, 2, 0), (b"c1", b"tree", r, 1, 2, 0), (b"c2", b"blob", r, 1, 2, 0),
         (b"c3", b"tree", r, 1, 2, 0), (b"c4", b"blob", flip(17), 1, 2, 0),
         (b"c5", b"blob", flip(63), 1, 2, 0), (b"c6", b"blob", r, 9, 2, 0),
         (b"c7", b"blob", r, 1, 9, 0), (b"c8", b"tree", flip(0), 5, 6, 0),
         (b"c9", b"tre", r, 1, 2, 0), (b"d0", b"", r, 1, 2, 0), (b"d1", b"blob", r, 1, 2, 9)]
    cases.append(("classes", side(a), side(b)))
    return cases


SIZES = (0, 1, 255, 256, 257, 1000)


def size_cases():
    return [("%dx%d" % (na, nb), *sized(na, nb, 1000 * na + nb)) for na in SIZES for nb in SIZES]


def big_case():
    return ("70000x50000", *sized(70000, 50000, 9))


def unsorted_case():
    a, b = sized(1000, 700, 3)
    rng = random.Random(4)
    rng.shuffle(a)
    return ("unsorted", a, list(reversed(b)))


def want_class(x, y) -> int:
    if x[1] == b"tree" and y[1] == b"tree":
        return TREES
    return SAME if x[1:5] == y[1:5] else DIFF


def py_join(a, b):
    """(a_match, b_match, a_class) by a dict over the names."""
    ib = {e[0]: j for j, e in enumerate(b)}
    ia = {e[0]: i for i, e in enumerate(a)}
    am = np.array([ib.get(e[0], -1) for e in a], dtype=np.int64).reshape(len(a))
    bm = np.array([ia.get(e[0], -1) for e in b], dtype=np.int64).reshape(len(b))
    ac = np.array([ONLY if j < 0 else want_class(a[i], b[j]) for i, j in enumerate(am.tolist())],
                  dtype=np.uint8).reshape(len(a))
    return am, bm, ac


def columns(s):
    """A side as the decoder's host columns (a dict of numpy arrays)."""
    n = len(s)
    offs = lambda parts: np.cumsum([0] + [len(p) for p in parts], dtype=np.uint64)
    return dict(
        n=n,
        names=np.frombuffer(b"".join(e[0] for e in s), dtype=np.uint8).copy(),
        name_offs=offs([e[0] for e in s]),
        modes=np.array([e[5] for e in s], dtype=np.uint32).reshape(n),
        types=np.frombuffer(b"".join(e[1] for e in s), dtype=np.uint8).copy(),
        type_offs=offs([e[1] for e in s]),
        roots=np.frombuffer(b"".join(e[2] for e in s), dtype=np.uint8).copy(),
        sizes=np.array([e[3] for e in s], dtype=np.uint64).reshape(n),
        block_sizes=np.array([e[4] for e in s], dtype=np.uint64).reshape(n),
        status=np.zeros(n, dtype=np.uint32))


COLS = ("names", "name_offs", "modes", "types", "type_offs", "roots", "sizes", "block_sizes",
        "status")


def host_struct(N, c):
    """glfsx_tree_cols over host columns (keep `c` alive while it is used)."""
    return N.glfsx_tree_cols(c["n"], *[c[k].ctypes.data for k in COLS])
