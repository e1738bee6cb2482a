"""One row per instantiation of the small-blob and the decrypt kernels.

The second launch log (glfsx_debug_aux_log) records what launch_small_pass
and decrypt_with really launched: k_small<G, CHACHA, 0>, k_small_q<G, false,
2>, k_small_q<G, true, 1> for G in {1, 2, 4, 8, 16}, k_decrypt_lines<0|2>
and k_decrypt.  As in tests/test_gpu_pass_matrix.py a case resets the log,
makes one call, asserts the records and only then compares every output byte
with the oracle on the device; outputs start from a poison value, so a store
outside a message's own bytes fails.

test_tables_cover_the_reachable_sets asks launch_plan.h (through
tests/c/launch_plan_sweep.cpp, its "S" and "D" lines) which instantiations
small_plan and decrypt_plan can return: the tables below cover exactly those
20 + 3.  It needs no GPU.

Small blobs (glfsx_post_blobs_device, block size 2 MiB): G follows max_len =
G KiB.  A batch is built from groups of 64 consecutive blobs, which coincide
with the waves of k_small and the coarse items of k_small_q; the last n / 8
blobs run as fine items of 64 / G blobs, which never straddle a group
(SmallLayout).  Neither glfsx_post_blobs_device nor
glfsx_decrypt_batch_device is documented to work in place (include/glfsx.h),
so no row asks for it.

Decrypt (glfsx_decrypt_batch_device): the input is the oracle's post of the
splitmix stream, so the expected plaintext does not come from the library.

The same log holds the levels of the ragged passes and the one-shot classes.
Their 32 instantiations are asserted in the tests that already have their
shapes (test_gpu_ragged, test_gpu_open_ragged, test_gpu_one,
test_gpu_one_open), with rag_expect and one_expect below; aux_kernel_table
names each instantiation, the records that mean it ran and that test, and
test_aux_table_covers_the_reachable_set holds the table against
launch_plan.h ("R" and "O" lines of the sweep program) and replays
tests/golden/aux_launch_records.txt.  A call may now log families beside the
ones a test is about, so every comparison selects its own (aux_take).
"""
import collections
import ctypes
import functools
import os
import random
import re

import numpy as np
import pytest

from test_gpu_pass_matrix import (CID_KEY, KIB, LAT_ASM, LAT_C, LOG_WORDS, MIB, POISON, _run,
                                  _torch, assert_same, to_dev, to_host)
from test_gpu_pass_matrix import knobs, sweep_program  # noqa: F401  (fixtures, used by name)

GIB = 1 << 30
SMALL, SMALL_Q, LINES, DECRYPT = 5, 6, 7, 8   # GLFSX_LOG_* (include/glfsx.h)
RAG_CHUNK, RAG_MERGE_A, RAG_MERGE_B, ONE, MED, ONE_OPEN = 9, 10, 11, 12, 13, 14
SMALL_FAMILIES, DEC_FAMILIES = (SMALL, SMALL_Q), (LINES, DECRYPT)
RAG_FAMILIES, ONE_FAMILIES = (RAG_CHUNK, RAG_MERGE_A, RAG_MERGE_B), (ONE, MED, ONE_OPEN)
POST_DEK, POST_CID, OPEN0, OPEN1, OPEN2 = range(5)   # RagKind (launch_plan.h)
SMALL_GS = (1, 2, 4, 8, 16)
BS = 2 * MIB                                  # the blobs' block size
FINE_DIV = 8                                  # kSmallFineDiv (launch_plan.h)

gpu_test = pytest.mark.gpu


def rec(family, g, chacha, aligned, form, shift, grid, w7, w8, n):
    """An aux-log record, in the order of include/glfsx.h."""
    return (family, g, int(chacha), int(aligned), form, shift, grid, w7, w8, n)


# ---------------------------------------------------------------- the tables
def small_items(g, n):
    """(n_coarse, items) as small_plan gives them for a k_small_q launch."""
    fine = n // FINE_DIV if g > 1 else 0
    bpi = 64 // g
    n_coarse = (n - fine) >> 6
    return n_coarse, n_coarse + -(-(n - 64 * n_coarse) // bpi)


def small_expect(g, queue, n):
    """The two launches of one call: the DEK pass, then the CID pass.  Every
    grid here is far below the resident workgroups, so capped_grid leaves it."""
    if not queue:
        return [rec(SMALL, g, ch, 0, 0, 0, -(-n // 256), 0, 0, n) for ch in (0, 1)]
    n_coarse, items = small_items(g, n)
    return [rec(SMALL_Q, g, ch, 0, 1 if ch else 2, 0, -(-items // 4), n_coarse, items, n)
            for ch in (0, 1)]


SMALL_ROWS = [(g, queue) for g in SMALL_GS for queue in (False, True)]

# glfsx_decrypt_batch_device over `blocks` blocks of bs bytes, the last of
# `last`; the plan (units, upb_shift, whether k_decrypt runs) is decrypt_plan's,
# computed on the CPU.  src_off / dst_off: bytes off 16-byte alignment.
DecRow = collections.namedtuple("DecRow", "name bs blocks last units upb_shift tail src_off dst_off")
DEC_ROWS = [
    DecRow("12k-tail", 12288, 6, 4196, 16, 64, True, 0, 0),
    DecRow("12k-whole", 12288, 6, 12288, 18, 64, False, 0, 0),
    DecRow("20k", 20480, 3, 8255, 12, 64, True, 0, 0),
    DecRow("4k", 4096, 33, 5, 32, 0, True, 0, 0),
    DecRow("64k", 65536, 3, 8191, 33, 4, True, 0, 0),
    DecRow("128", 128, 7, 70, 0, 0, True, 0, 0),
    DecRow("8k-src1", 8192, 3, 100, 0, 0, True, 1, 0),
    DecRow("8k-dst1", 8192, 3, 100, 0, 0, True, 0, 1),
]
# At the default threshold: more than 4 x 16384 runs, so waves take further
# runs through the double buffer.  261 blocks: 1027 waves take a second run;
# 513: runs of two units, the last run partial and in the short block; 12 KiB
# blocks: the division path (upb_shift 64) with several runs per wave.
BigDecRow = collections.namedtuple("BigDecRow", "name bs blocks last units run_shift upb_shift")
BIG_DEC_ROWS = [
    BigDecRow("261x1m", MIB, 261, 12365, 66563, 0, 8),
    BigDecRow("513x1m", MIB, 513, 12365, 131075, 1, 8),
    BigDecRow("43691x12k", 12288, 43691, 100, 131070, 0, 64),
]


def dec_total(row):
    return (row.blocks - 1) * row.bs + row.last


def dec_expect(row, form, run_shift=0, lines_grid=None):
    out = []
    if row.units:
        runs = -(-row.units // (1 << run_shift))
        grid = lines_grid if lines_grid is not None else -(-runs // 4)
        out.append(rec(LINES, 0, 1, 1, form, run_shift, grid, row.upb_shift, row.units,
                       row.blocks))
    kbs, first_kb = -(-dec_total(row) // 64), row.units * 64
    if first_kb < kbs:
        aligned = not (getattr(row, "src_off", 0) or getattr(row, "dst_off", 0))
        out.append(rec(DECRYPT, 0, 1, aligned, 0, 0, -(-(kbs - first_kb) // 256), 0, first_kb,
                       row.blocks))
    return out


def table_kernels():
    small = {r[:3] + (r[4],) for g, q in SMALL_ROWS for r in small_expect(g, q, 2193)}
    dec = {(r[0], r[4]) for row in DEC_ROWS for form in (0, 2) for r in dec_expect(row, form)}
    dec |= {(r[0], r[4]) for row in BIG_DEC_ROWS for r in dec_expect(row, 2, row.run_shift, 16384)}
    return small, dec


# ---------------------------------- the ragged passes and the one-shot classes
# These 32 instantiations are asserted where their shapes already are: each
# test below resets the aux log, makes its call, and compares the records with
# rag_expect / one_expect before it compares bytes with the oracle.
def rag_totals(lens):
    """The plan's totals over the selected messages: chunks, merge groups,
    messages of more than 256 chunks (ragged_kernels.h k_rag_count)."""
    c = [max(1, -(-ln // 1024)) for ln in lens]
    return sum(c), sum(-(-x // 256) for x in c if x > 1), sum(x > 256 for x in c)


def latency_wgs_now(N):
    """The latency threshold in force (the setter returns the previous value)."""
    v = N.set_latency_wgs(0)
    N.set_latency_wgs(v)
    return v


def rag_expect(lens, kind, latency_wgs):
    """One ragged pass over messages of these lengths: the chunk level (form 0
    when its tiles of 256 chunks number at most latency_wgs, else 2), merge
    level A exactly when a message has more than one chunk, B when more than
    256."""
    return rag_expect_totals(rag_totals(lens), kind, latency_wgs)


def rag_expect_totals(tot, kind, latency_wgs):
    tiles = -(-tot[0] // 256)
    chacha = kind == POST_CID or kind >= OPEN1
    out = [rec(RAG_CHUNK, kind, chacha, 0, 0 if tiles <= latency_wgs else 2, 0,
               min(tiles, 1 << 20), 0, tot[0], 0)]
    for family, total in ((RAG_MERGE_A, tot[1]), (RAG_MERGE_B, tot[2])):
        if total:
            out.append(rec(family, kind, chacha, 0, 0, 0, min(total, 1 << 20), 0, total, 0))
    return out


def one_expect(family, n, max_len, salted=True):
    """One one-shot class launch: QUADS 16 up to 16 KiB, else 64 (the medium
    pair 64, a workgroup per 64 KiB); word 7 is 1 when the one descriptor went
    by value."""
    quads = 16 if max_len <= 16384 else 64
    wmax = -(-max_len // 65536) if family == MED else 1
    return rec(family, quads, salted if family == ONE_OPEN else 1, 1, 0, 0, n * wmax,
               int(n == 1), max_len, n)


T_RAG = "test_gpu_ragged.py::test_edge_lengths"
T_ORAG = "test_gpu_open_ragged.py::test_edge_lengths"
T_ORAG_01 = "test_gpu_open_ragged.py::test_damage"
T_ONE = "test_gpu_one.py::test_one_shot_post_edges"
T_MED = "test_gpu_one.py::test_medium_post_edges"
T_WRITER = "test_gpu_one.py::test_writer_small_blocks_one_shot"
T_OPEN = "test_gpu_one_open.py::test_clean"
T_SHARED = "test_gpu_one_open.py::test_posts_and_opens_share_launches"


def aux_kernel_table():
    """Instantiation -> (the record keys that mean it ran, as launch_plan_sweep
    prints them: family, kind, form / family, QUADS, salted, by value; the
    test that asserts them)."""
    t = {}
    for kind, name in ((POST_DEK, "false"), (POST_CID, "true")):
        for form in (0, 2):
            t["k_rag_chunk<%s, %d>" % (name, form)] = ({(RAG_CHUNK, kind, form)}, T_RAG)
    t["k_rag_merge_a"] = ({(RAG_MERGE_A, POST_DEK, 0), (RAG_MERGE_A, POST_CID, 0)}, T_RAG)
    t["k_rag_merge_b"] = ({(RAG_MERGE_B, POST_DEK, 0), (RAG_MERGE_B, POST_CID, 0)}, T_RAG)
    for mode, where in ((0, T_ORAG_01), (1, T_ORAG_01), (2, T_ORAG)):
        for form in (0, 2):
            t["k_rag_open_chunk<%d, %d>" % (mode, form)] = ({(RAG_CHUNK, OPEN0 + mode, form)}, where)
    for level, family in (("a", RAG_MERGE_A), ("b", RAG_MERGE_B)):
        t["k_rag_open_merge_%s<false>" % level] = ({(family, OPEN0, 0), (family, OPEN1, 0)},
                                                   T_ORAG_01)
        t["k_rag_open_merge_%s<true>" % level] = ({(family, OPEN2, 0)}, T_ORAG)
    for q in (16, 64):
        t["k_one_v<%d>" % q] = ({(ONE, q, 0, 1)}, T_ONE)
        t["k_one<%d>" % q] = ({(ONE, q, 0, 0)}, T_WRITER)
        for salted in (0, 1):
            name = "%d, %s>" % (q, "true" if salted else "false")
            t["k_one_open_v<" + name] = ({(ONE_OPEN, q, salted, 1)}, T_OPEN)
            # reached only when concurrent callers coalesce
            t["k_one_open<" + name] = ({(ONE_OPEN, q, salted, 0)}, T_SHARED)
    for half in ("dek", "cid"):     # one record for the pair
        t["k_med_%s_v" % half] = ({(MED, 64, 0, 1)}, T_MED)
        t["k_med_%s" % half] = ({(MED, 64, 0, 0)}, T_WRITER)
    return t


def aux_key(r):
    """The table's key of a logged record."""
    if r[0] in RAG_FAMILIES:
        return (r[0], r[1], r[4])
    return (r[0], r[1], r[2] if r[0] == ONE_OPEN else 0, r[7])


# ------------------------------------------------------------- CPU meta-tests
def test_aux_table_covers_the_reachable_set(sweep_program):
    """The 32 instantiations of the ragged and one-shot families: the table's
    record keys are exactly what rag_pass_recs and one_rec can return (the
    program itself fails unless that is the launchable set), and the pure
    functions reproduce the launches recorded from the old launchers."""
    lines = [ln.split() for ln in _run([sweep_program]).splitlines()]
    want = {tuple(int(x) for x in ln[1:]) for ln in lines if ln[0] in ("R", "O")}
    table = aux_kernel_table()
    have = set().union(*(keys for keys, _ in table.values()))
    assert have == want, (sorted(want - have), sorted(have - want))
    assert len(table) == 32 and len(want) == 34
    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "aux_launch_records.txt")
    n = sum(1 for _ in open(fixture))
    assert n >= 150
    assert "replayed %d\n" % n in _run([sweep_program, "--aux", fixture])
    # the helpers the GPU tests assert with agree with the fixture's rows
    for ln in open(fixture):
        w = ln.split()
        if w[0] == "R":
            tot, kind, lat = tuple(int(x) for x in w[1:4]), int(w[4]), int(w[5])
            recs = [tuple(int(x) for x in w[7 + 10 * i:17 + 10 * i]) for i in range(int(w[6]))]
            assert recs == rag_expect_totals(tot, kind, lat)
        else:
            cls, cnt, max_len = (int(x) for x in w[1:4])
            got = tuple(int(x) for x in w[5:15])
            family = (ONE, MED, ONE_OPEN, ONE_OPEN)[cls]
            assert got == one_expect(family, cnt, max_len, salted=cls == 3)


def test_tables_cover_the_reachable_sets(sweep_program):
    lines = [ln.split() for ln in _run([sweep_program]).splitlines()]
    want_small = {tuple(int(x) for x in ln[1:]) for ln in lines if ln[0] == "S"}
    want_dec = {tuple(int(x) for x in ln[1:]) for ln in lines if ln[0] == "D"}
    small, dec = table_kernels()
    assert small == want_small, (sorted(want_small - small), sorted(small - want_small))
    assert dec == want_dec, (sorted(want_dec - dec), sorted(dec - want_dec))
    assert len(want_small) == 20 and len(want_dec) == 3
    assert sum(ln[0] == "K" for ln in lines) == 60      # the pass log's set is as it was


def test_aux_log_hook_needs_no_device():
    from glfs_amd import _native as N
    n = ctypes.c_size_t(77)
    buf = (ctypes.c_uint32 * LOG_WORDS)()
    assert N.lib.glfsx_debug_aux_log(0, buf, 1, ctypes.byref(n)) == 0
    assert N.lib.glfsx_debug_aux_log(0, None, 0, None) == 0
    assert N.lib.glfsx_debug_aux_log(0, None, 1, None) == N.GLFSX_E_ARG


# ------------------------------------------------------------------- helpers
def aux_reset(N):
    N.check(N.lib.glfsx_debug_aux_log(1, None, 0, None))


def aux_take(N, cap=64, families=None):
    """The aux log since the last reset, emptied; `families`: only the records
    of the families a test is about (a call may launch others beside them)."""
    buf = (ctypes.c_uint32 * (LOG_WORDS * cap))()
    n = ctypes.c_size_t()
    N.check(N.lib.glfsx_debug_aux_log(1, buf, cap, ctypes.byref(n)))
    assert n.value <= cap, n.value
    log = [tuple(buf[i * LOG_WORDS:(i + 1) * LOG_WORDS]) for i in range(n.value)]
    return [r for r in log if families is None or r[0] in families]


def poisoned(torch, n):
    return torch.full((n,), POISON, dtype=torch.uint8, device="cuda")


def blob_salt(O):
    return O.derive_key(bytes(32), b"blob")


def oracle_blob(O, blob, key=None):
    """glfs.PostBlob of one single-block blob: (root ref, ctext).  The empty
    blob's post(indexSalt, "") is the oracle writer's own rule."""
    root, _, _, posts = O.create(blob, BS, salt=blob_salt(O), cid_key=key)
    return root, (posts[0][3] if blob else b"")


def ragged_lens(g):
    c = g * KIB
    return sorted({x for x in (0, 1, 63, 64, 65, 1023, 1024, 1025, c - 1, c, g * 512 + 1)
                   if x <= c})


def up16(o):
    return -(-o // 16) * 16


class Layout:
    """Offsets and lengths of a batch, group by group."""

    def __init__(self, g, start=0):
        self.g, self.c, self.o = g, g * KIB, start
        self.offs, self.lens = [], []

    def put(self, off, ln):
        self.offs.append(off)
        self.lens.append(ln)

    def dense(self, count=64):
        """(a) blobs of exactly G KiB back to back from a 16-byte-aligned offset."""
        self.o = up16(self.o)
        for _ in range(count):
            self.put(self.o, self.c)
            self.o += self.c

    def gap(self):
        """(b) the same with one 16-byte gap near the middle of the wave, inside
        a fine item (items of 64 / G blobs start at multiples of 64 / G)."""
        self.o = up16(self.o)
        at = 32 + (64 // self.g // 2 if self.g > 1 else 0)
        for i in range(64):
            self.o += 16 if i == at else 0
            self.put(self.o, self.c)
            self.o += self.c

    def permuted(self, rng):
        """(b) the same blobs in a permuted order: no fine item is dense."""
        base = up16(self.o)
        perm = list(range(64))
        rng.shuffle(perm)
        bpi = 64 // self.g
        for k in range(0, 64, bpi):
            assert perm[k:k + bpi] != list(range(perm[k], perm[k] + bpi))
        for p in perm:
            self.put(base + p * self.c, self.c)
        self.o = base + 64 * self.c

    def ragged(self, phases, count=64):
        """(c) phases (0,): every edge length at a 16-aligned offset; (d)
        phases (1, 4, 8): the same lengths off alignment."""
        lens = ragged_lens(self.g)
        for i in range(count):
            self.o = up16(self.o) + phases[i % len(phases)]
            self.put(self.o, lens[i % len(lens)])
            self.o += lens[i % len(lens)]


class SmallData:
    """G's batch and its oracle values, made once.  2193 blobs = 29 groups,
    which are the coarse items when G > 1 -- (2193 - 2193 // 8) >> 6 = 29 --
    and then 337 fine blobs: one group of each kind on either side, and (e) 17
    blobs at the end: a partial wave, a partial last fine item."""
    N_COARSE, N = 29, 29 * 64 + 5 * 64 + 17

    def __init__(self, torch, O, g):
        rng = random.Random(100 + g)
        lay = Layout(g)
        for region in range(2):
            lay.dense()
            lay.gap()
            lay.permuted(rng)
            lay.ragged((0,))
            lay.ragged((1, 4, 8))
            for _ in range(self.N_COARSE - 5 if region == 0 else 0):
                lay.dense()
        lay.dense(17)
        assert len(lay.offs) == self.N
        self.g, self.offs, self.lens = g, lay.offs, lay.lens
        self.total = up16(lay.o) + 64
        data = O.fill_splitmix(self.total, 7000 + g)
        image = bytearray([POISON]) * self.total
        roots, keyed = [], []
        for o, n in zip(lay.offs, lay.lens):
            root, ct = oracle_blob(O, data[o:o + n])
            image[o:o + n] = ct
            roots.append(root)
            keyed.append(oracle_blob(O, data[o:o + n], CID_KEY)[0])
        guard = bytes([POISON]) * 64
        self.src = to_dev(torch, data)
        self.src0 = self.src.clone()
        self.want_ct = to_dev(torch, guard + bytes(image) + guard)
        self.want_roots = {False: to_dev(torch, b"".join(roots) + guard),
                           True: to_dev(torch, b"".join(keyed) + guard)}
        self.d_offs = torch.tensor(lay.offs, dtype=torch.int64, device="cuda")
        self.d_lens = torch.tensor(lay.lens, dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def small_data(g):
    from oracle import oracle as O
    return SmallData(_torch(), O, g)


# ------------------------------------------------------- k_small, k_small_q
@gpu_test
@pytest.mark.parametrize("g,queue", SMALL_ROWS,
                         ids=["g%d-%s" % (g, "q" if q else "lane") for g, q in SMALL_ROWS])
def test_small(gpu, O, knobs, g, queue):
    """k_small<G, ., 0> (latency threshold 1 << 31) or k_small_q<G, false, 2>
    and <G, true, 1> (threshold 0) over SmallData: ctext out of place, no
    ctext (the DEK pass stages dense waves, the CID pass cannot), the ctext 3
    bytes off alignment with the source aligned, and a keyed CID."""
    torch = _torch()
    N, sd = gpu, small_data(g)
    n = sd.N
    knobs(LAT_ASM if queue else LAT_C)
    expect = small_expect(g, queue, n)
    if queue and g > 1:
        # the groups of the second region are exactly the fine blobs
        assert expect[0][7] == sd.N_COARSE and 64 * sd.N_COARSE == n - 337
    for variant in ("out", "none", "ct3", "keyed"):
        what = "G=%d %s %s" % (g, "k_small_q" if queue else "k_small", variant)
        off = 3 if variant == "ct3" else 0
        ct = None if variant == "none" else poisoned(torch, off + 64 + sd.total + 64)
        roots = poisoned(torch, 64 * n + 64)
        torch.cuda.synchronize()
        aux_reset(N)
        N.check(N.lib.glfsx_post_blobs_device(
            BS, blob_salt(O), CID_KEY if variant == "keyed" else None, sd.src.data_ptr(),
            sd.d_offs.data_ptr(), sd.d_lens.data_ptr(), n, g * KIB,
            ct.data_ptr() + off + 64 if ct is not None else None, roots.data_ptr(), None))
        torch.cuda.synchronize()
        assert aux_take(N, families=SMALL_FAMILIES) == expect, what
        assert_same(torch, roots, sd.want_roots[variant == "keyed"], what + " roots")
        if ct is not None:
            assert_same(torch, ct[off:], sd.want_ct, what + " ctext")
            assert bool((ct[:off] == POISON).all()), what
        assert_same(torch, sd.src, sd.src0, what + " source")


# The work-queue loop of k_small_q at the default latency threshold: 400 000
# blobs are 6250 items of 64, more than 4 x the resident grid, so waves take
# further items from the counter (item = waves + fetch_add).  The call runs
# twice on one stream: four k_small_q launches, the counter banks alternating
# by epoch.  64-byte blobs take the per-lane path, 1 KiB blobs the staged one.
# The log showed a grid of 1280 workgroups for the DEK pass and 1024 for the
# CID pass (5 and 4 resident workgroups on each of 256 CUs): 6250 > 4 x 1280.
QUEUE_N = 400_000


@gpu_test
@pytest.mark.parametrize("ln", [64, 1024])
def test_small_queue_loop(gpu, O, ln):
    torch = _torch()
    N, n = gpu, QUEUE_N
    total = n * ln
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    N.check(N.lib.glfsx_fill_splitmix_device(src.data_ptr(), 0, total, 8000 + ln, None))
    torch.cuda.synchronize()
    host = src.cpu().numpy()
    refs, ctext = np.empty(64 * n, dtype=np.uint8), np.empty(total, dtype=np.uint8)
    raw = O.derive_key(blob_salt(O), b"raw")
    O.lib().oracle_post_batch(refs.ctypes.data, ctext.ctypes.data, raw, host.ctypes.data, total,
                              ln, None, 16)
    want_roots = poisoned(torch, 64 * n + 64)
    want_roots[:64 * n] = torch.from_numpy(refs).cuda()
    want_ct = poisoned(torch, 64 + total + 64)
    want_ct[64:64 + total] = torch.from_numpy(ctext).cuda()
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * ln
    lens = torch.full((n,), ln, dtype=torch.int64, device="cuda")
    roots, ct = torch.empty_like(want_roots), torch.empty_like(want_ct)
    for run in range(2):
        roots.fill_(POISON)
        ct.fill_(POISON)
        torch.cuda.synchronize()
        aux_reset(N)
        N.check(N.lib.glfsx_post_blobs_device(BS, blob_salt(O), None, src.data_ptr(),
                                              offs.data_ptr(), lens.data_ptr(), n, ln,
                                              ct.data_ptr() + 64, roots.data_ptr(), None))
        torch.cuda.synchronize()
        log = aux_take(N, families=SMALL_FAMILIES)
        print("k_small_q ln=%d run %d:" % (ln, run), log)
        assert len(log) == 2
        for ch, r in enumerate(log):
            # the grid is the resident workgroups, the runtime's figure
            assert r == rec(SMALL_Q, 1, ch, 0, 1 if ch else 2, 0, r[6], 6250, 6250, n), (run, r)
            assert 0 < r[6] and r[8] > 4 * r[6], (run, r)   # some wave takes a second item
        assert_same(torch, roots, want_roots, "ln=%d run %d roots" % (ln, run))
        assert_same(torch, ct, want_ct, "ln=%d run %d ctext" % (ln, run))


# Blobs at offsets around 2 GiB and 4 GiB of a 4 GiB + 2 MiB source (and
# ctext): a lane's offset goes through two 32-bit readfirstlanes, whose low
# word once sign-extended from 2 GiB on (small_kernels.h).  Dense groups of
# 4 KiB blobs ending below 2 GiB, straddling 2 GiB, straddling 4 GiB and --
# the last group, fine items under k_small_q -- wholly between 2 and 4 GiB,
# and a ragged group above 4 GiB.  Only the blobs are written and compared,
# with 64 poisoned bytes around each group.
@functools.lru_cache(maxsize=None)
def high_layout():
    from oracle import oracle as O
    g, grp = 4, 64 * 4 * KIB
    starts = [2 * GIB - grp // 2 - 64 - grp, 2 * GIB - grp // 2, 4 * GIB + 2 * grp,
              4 * GIB - grp // 2, 3 * GIB]
    lay, spans = Layout(g), []
    for k, start in enumerate(starts):
        lay.o = start
        if k == 2:
            lay.ragged((0, 1, 4, 8))
        else:
            lay.dense()
        spans.append((start, up16(lay.o)))
    assert max(e for _, e in spans) + 64 <= 4 * GIB + 2 * MIB
    pieces, images, roots = [], [], []
    for k, (s, e) in enumerate(spans):
        data = O.fill_splitmix(e - s, 9000 + k)
        image = bytearray([POISON]) * (e - s + 128)
        for o, n in list(zip(lay.offs, lay.lens))[64 * k:64 * k + 64]:
            root, ct = oracle_blob(O, data[o - s:o - s + n])
            image[64 + o - s:64 + o - s + n] = ct
            roots.append(root)
        pieces.append(data)
        images.append(bytes(image))
    return lay, spans, pieces, images, b"".join(roots)


@gpu_test
@pytest.mark.parametrize("queue", [False, True], ids=["lane", "q"])
def test_small_offsets_above_2_and_4_gib(gpu, O, knobs, queue):
    """Fails, and does not skip, when the card has not 8.1 GiB free."""
    torch = _torch()
    N = gpu
    lay, spans, pieces, images, want_roots = high_layout()
    n = len(lay.offs)
    size = 4 * GIB + 2 * MIB
    src = torch.empty(size, dtype=torch.uint8, device="cuda")
    ct = torch.empty(size, dtype=torch.uint8, device="cuda")
    for (s, e), data in zip(spans, pieces):
        src[s:e] = to_dev(torch, data)
        ct[s - 64:e + 64] = POISON
    d_offs = torch.tensor(lay.offs, dtype=torch.int64, device="cuda")
    d_lens = torch.tensor(lay.lens, dtype=torch.int64, device="cuda")
    roots = poisoned(torch, 64 * n + 64)
    knobs(LAT_ASM if queue else LAT_C)
    torch.cuda.synchronize()
    aux_reset(N)
    N.check(N.lib.glfsx_post_blobs_device(BS, blob_salt(O), None, src.data_ptr(),
                                          d_offs.data_ptr(), d_lens.data_ptr(), n, 4 * KIB,
                                          ct.data_ptr(), roots.data_ptr(), None))
    torch.cuda.synchronize()
    expect = small_expect(4, queue, n)
    assert aux_take(N, families=SMALL_FAMILIES) == expect
    if queue:
        assert expect[0][7] == 4      # the last group runs as fine items
    assert_same(torch, roots, to_dev(torch, want_roots + bytes([POISON]) * 64), "roots")
    for k, ((s, e), image) in enumerate(zip(spans, images)):
        assert_same(torch, ct[s - 64:e + 64], to_dev(torch, image), "ctext of group %d" % k)
        assert_same(torch, src[s:e], to_dev(torch, pieces[k]), "source of group %d" % k)


# glfsx_post_tree_device under k_small_q: test_post_tree_device_equals_sequence
# (tests/test_gpu_tree_read.py) runs at the default threshold with at most
# 70 000 blobs, 274 workgroups, which selects k_small.  Here the CID pass of
# k_small_q writes the hex digits of each root into its tree line (put_hex32)
# from coarse items, from fine items that fall back to a lane per blob and
# from dense fine items (G lanes per blob).
@gpu_test
def test_post_tree_device_hex_digits_under_k_small_q(gpu, O, knobs):
    torch = _torch()
    N, n, g = gpu, 400, 4
    from test_gpu_tree_read import _tree_inputs
    rng = random.Random(41)
    lay = Layout(g)
    lay.dense()                                   # coarse, staged
    for _ in range(n - 128):                      # ragged, odd offsets
        ln = rng.choice([0, 1, 63, 100, 1024, 4096, 3000, rng.randrange(4097)])
        lay.put(lay.o, ln)
        lay.o += ln + rng.randrange(3)
    lay.dense()                                   # fine items 336..399, dense
    assert small_items(g, n) == (5, 10) and (n - 64 - 320) % 16 == 0
    alphabet = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
    names = set()
    for ln in range(1, 9):                        # 50 names of each length 1..8
        while len(names) < 50 * ln:
            names.add(bytes(rng.choice(alphabet) for _ in range(ln)))
    names = sorted(names)
    assert len(names) == n and {len(x) for x in names} == set(range(1, 9))
    data = torch.empty(up16(lay.o) + 64, dtype=torch.uint8, device="cuda")
    N.check(N.lib.glfsx_fill_splitmix_device(data.data_ptr(), 0, data.numel(), 43, None))
    offs = torch.tensor(lay.offs, dtype=torch.int64, device="cuda")
    lens = torch.tensor(lay.lens, dtype=torch.int64, device="cuda")
    dn, dno, dm, dt, dto, _, dbs = _tree_inputs(torch, names, [b"blob"] * n, [0o644] * n,
                                                lay.lens, [BS] * n)
    bsalt, tsalt = blob_salt(O), O.derive_key(bytes(32), b"tree")
    cap = 300 * n + 4096
    knobs(LAT_ASM)
    torch.cuda.synchronize()
    roots1 = poisoned(torch, 64 * n)
    N.check(N.lib.glfsx_post_blobs_device(BS, bsalt, None, data.data_ptr(), offs.data_ptr(),
                                          lens.data_ptr(), n, 4096, None, roots1.data_ptr(),
                                          None))
    out1 = poisoned(torch, cap)
    t1 = ctypes.c_uint64()
    N.check(N.lib.glfsx_tree_encode_device(n, dn.data_ptr(), dno.data_ptr(), dm.data_ptr(),
                                           dt.data_ptr(), dto.data_ptr(), roots1.data_ptr(),
                                           lens.data_ptr(), dbs.data_ptr(), out1.data_ptr(),
                                           cap, None, ctypes.byref(t1), None))
    r1 = N.glfsx_root()
    N.check(N.lib.glfsx_create_device(BS, tsalt, None, out1.data_ptr(), t1.value, None,
                                      ctypes.byref(r1), None, None))
    roots2, out2 = poisoned(torch, 64 * n), poisoned(torch, cap)
    r2, t2 = N.glfsx_root(), ctypes.c_uint64()
    torch.cuda.synchronize()
    aux_reset(N)
    N.check(N.lib.glfsx_post_tree_device(n, BS, bsalt, tsalt, None, data.data_ptr(),
                                         offs.data_ptr(), lens.data_ptr(), 4096, None,
                                         roots2.data_ptr(), dn.data_ptr(), dno.data_ptr(),
                                         dm.data_ptr(), dt.data_ptr(), dto.data_ptr(),
                                         dbs.data_ptr(), BS, out2.data_ptr(), cap, None,
                                         ctypes.byref(r2), ctypes.byref(t2), None))
    torch.cuda.synchronize()
    log = [r for r in aux_take(N) if r[0] in (SMALL, SMALL_Q)]
    assert log == small_expect(g, True, n)
    assert t2.value == t1.value and bytes(r2.ref) == bytes(r1.ref)
    assert_same(torch, roots2, roots1, "roots")
    assert_same(torch, out2[:t2.value], out1[:t1.value], "lines")
    text = to_host(out1[:t1.value])
    at = [m.end() for m in re.finditer(b'"cid":"', text)]
    assert len(at) == n and {i % 4 for i in at} == {0, 1, 2, 3}   # every residue of hex_pos
    host = to_host(data)
    want = b"".join(oracle_blob(O, host[o:o + ln])[0] for o, ln in zip(lay.offs, lay.lens))
    assert to_host(roots2) == want
    # nothing behind the lines: the digits stay inside their fields
    assert bool((out2[t2.value:] == POISON).all())


# ------------------------------------------------ k_decrypt_lines, k_decrypt
def oracle_posted(O, plain, total, bs):
    """(refs, ctext) of the oracle's post of `plain` (a numpy array), threaded."""
    n = -(-total // bs)
    refs, ct = np.empty(64 * n, dtype=np.uint8), np.empty(total, dtype=np.uint8)
    raw = O.derive_key(bytes(32), b"raw")
    O.lib().oracle_post_batch(refs.ctypes.data, ct.ctypes.data, raw, plain.ctypes.data, total, bs,
                              None, 16)
    return refs, ct


@gpu_test
@pytest.mark.parametrize("row", DEC_ROWS, ids=lambda r: r.name)
def test_decrypt(gpu, O, knobs, row):
    """Form 0 (latency threshold 1 << 31) and form 2 (threshold 0) of the line
    kernel and k_decrypt's tail: the plaintext is the oracle's splitmix stream,
    the ctext the oracle's post of it."""
    torch = _torch()
    N, total = gpu, dec_total(row)
    plain = np.frombuffer(O.fill_splitmix(total, 6000 + row.bs), dtype=np.uint8)
    refs, ct = oracle_posted(O, plain, total, row.bs)
    a, b = 64 + row.src_off, 64 + row.dst_off
    d_ct = poisoned(torch, a + total + 64)
    d_ct[a:a + total] = torch.from_numpy(ct).cuda()
    d_ct0 = d_ct.clone()
    d_refs = torch.from_numpy(refs).cuda()
    want = poisoned(torch, b + total + 64)
    want[b:b + total] = torch.from_numpy(plain.copy()).cuda()
    for lat, form in ((LAT_C, 0), (LAT_ASM, 2)):
        what = "%s form %d" % (row.name, form)
        knobs(lat)
        out = poisoned(torch, b + total + 64)
        torch.cuda.synchronize()
        aux_reset(N)
        N.check(N.lib.glfsx_decrypt_batch_device(d_ct.data_ptr() + a, total, row.bs,
                                                 d_refs.data_ptr(), out.data_ptr() + b, None))
        torch.cuda.synchronize()
        assert aux_take(N, families=DEC_FAMILIES) == dec_expect(row, form), what
        assert_same(torch, out, want, what)
        assert_same(torch, d_ct, d_ct0, what + " ctext")


@gpu_test
@pytest.mark.parametrize("row", BIG_DEC_ROWS, ids=lambda r: r.name)
def test_decrypt_runs_loop(gpu, O, knobs, row):
    """The line kernel's loop over runs (the next run's loads in flight while
    this one is decrypted) at the default threshold, form 2, and once more in
    form 0.  The record says that more than 4 x grid runs were there to take."""
    torch = _torch()
    N, total = gpu, dec_total(row)
    want = poisoned(torch, 64 + total + 64)
    N.check(N.lib.glfsx_fill_splitmix_device(want.data_ptr() + 64, 0, total, 6500 + row.blocks,
                                             None))
    torch.cuda.synchronize()
    plain = want[64:64 + total].cpu().numpy()
    refs, ct = oracle_posted(O, plain, total, row.bs)
    d_ct, d_refs = torch.from_numpy(ct).cuda(), torch.from_numpy(refs).cuda()
    out = torch.empty_like(want)
    for lat, form in ((None, 2), (LAT_C, 0)):
        what = "%s form %d" % (row.name, form)
        knobs(lat)
        out.fill_(POISON)
        torch.cuda.synchronize()
        aux_reset(N)
        N.check(N.lib.glfsx_decrypt_batch_device(d_ct.data_ptr(), total, row.bs,
                                                 d_refs.data_ptr(), out.data_ptr() + 64, None))
        torch.cuda.synchronize()
        log = aux_take(N, families=DEC_FAMILIES)
        assert log == dec_expect(row, form, row.run_shift, 16384), what
        lines = log[0]
        assert lines[5] == row.run_shift and lines[7] == row.upb_shift, what
        assert (lines[8] >> lines[5]) > 4 * lines[6], what      # runs > 4 x grid
        assert_same(torch, out, want, what)
