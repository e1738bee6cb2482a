"""One row per reachable instantiation of the bulk-pass kernels.

The host code (glfs_amd/csrc/launch_plan.h) picks a kernel from the shape,
the pointer alignment and two tuning values.  Every row below names the
smallest shape and knob setting that selects one instantiation, and the
launch log (glfsx_debug_pass_log) says which kernel the call really ran: a
case resets the log, makes one call, asserts that the records equal the
row's expectation and only then compares bytes with the oracle, bit for bit.
A shape that stops reaching its kernel after a retuning fails here.

test_table_covers_the_reachable_set asks the selection itself
(glfs_amd/csrc/launch_plan.h, pure functions) which instantiations it can
return: a stand-alone program (tests/c/launch_plan_sweep.cpp) sweeps it over
shapes and knob values, and the rows' expectations must cover exactly that
set, which is also the set the dispatchers can launch.  It needs no GPU.

Knobs: set_split_target(0) fixes G from the block size (no split up to
16 MiB blocks); set_latency_wgs(0) gives ARX forms 1/2, set_latency_wgs(1 <<
31) form 0 and the quad kernels.

k_pass rows use blocks of bs_G = 256 G KiB, so every lane of a full block
holds G chunks, and two blocks, so G follows the block size and not the last
length.  The last block is cut at the lengths of last_lens(): the chunk and
block edges, a whole message inside lane 0 (G KiB: ROOT inside the lane) and
its neighbours (the whole generic path, the two-lane path), exactly one wave
(64 G KiB), a mixed wave ((69 G + G/2) KiB + 199: wave 0 staged, in wave 1
lanes 64-68 on the unstaged fast path and lane 69 with fewer than G chunks,
the last of three full blocks and 7 bytes), and bs - 1.

The CID rows write random DEKs into the refs themselves, so the expected
ctext is ChaCha20 under a key that does not depend on the data: a keystream
or counter fault shows apart from a DEK fault.  The ctext of the last block
under a fixed DEK at length L is a prefix of the ctext at full length, so the
oracle encrypts each block once per G.
"""
import collections
import ctypes
import functools
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glfs_amd", "csrc")
KIB, MIB = 1 << 10, 1 << 20
POISON = 0xA5
SALT = bytes(range(7, 39))
CID_KEY = bytes(range(101, 133))
PASS, QUAD, PASS_DC, OPEN = 1, 2, 3, 4     # GLFSX_LOG_* (include/glfsx.h)
LOG_WORDS = 10                             # GLFSX_PASS_LOG_WORDS
LAT_ASM, LAT_C = 0, 1 << 31                # set_latency_wgs: forms 1/2, form 0
GS = (1, 2, 4, 8, 16, 32, 64)

gpu_test = pytest.mark.gpu


def rec(family, g, chacha, aligned, form, sl, grid, n, fine_div=0, items=0):
    """A log record, in the order of include/glfsx.h."""
    return (family, g, int(chacha), int(aligned), form, sl, grid, fine_div, items, n)


def kernel_of(r):
    """The instantiation a record names: family and template arguments."""
    return r[:5]


# ------------------------------------------------------------------ the table
def bs_of(g):
    return 256 * g * KIB


def dek_blocks_c(g):
    """Form 0 of the DEK pass: more than 16384 chunks (or quad_ok takes the
    launch) in the fewest blocks of bs_G -- 65, 33, 17, 9, 5, 3, 2."""
    return 64 // g + 1


def cid_form(g):
    """pass_rec: the aligned CID pass without split runs form 1 from G = 4."""
    return 1 if g >= 4 else 2


# One k_pass call: `blocks` blocks of bs_G + bs_delta bytes, the source
# src_off bytes and the ctext ct_off bytes off 16-byte alignment; ctext is
# None (the DEK pass), "none" (NULL), "out" or "in" (in place).
PassRow = collections.namedtuple(
    "PassRow", "name g chacha lat blocks bs_delta src_off ct_off ctext keyed expect")


def _pass_rows():
    rows = []
    for g in GS:
        def dek(name, lat, blocks, aligned, form, bs_delta=0, src_off=0):
            rows.append(PassRow(name, g, 0, lat, blocks, bs_delta, src_off, 0, None, False,
                                rec(PASS, g, 0, aligned, form, 0, blocks, blocks)))

        def cid(name, lat, aligned, form, ctext, bs_delta=0, src_off=0, ct_off=0, keyed=False):
            rows.append(PassRow(name, g, 1, lat, 2, bs_delta, src_off, ct_off, ctext, keyed,
                                rec(PASS, g, 1, aligned, form, 0, 2, 2)))

        dek("dek-asm", LAT_ASM, 2, 1, 2)
        dek("dek-c", LAT_C, dek_blocks_c(g), 1, 0)
        for off in (1, 4, 8):
            dek("dek-bytes-src%d" % off, LAT_ASM, 2, 0, 2, src_off=off)
        dek("dek-bytes-bs-1", LAT_ASM, 2, 0, 2, bs_delta=-1)
        f = cid_form(g)
        cid("cid-asm-out", LAT_ASM, 1, f, "out")
        cid("cid-asm-out-keyed", LAT_ASM, 1, f, "out", keyed=True)
        cid("cid-asm-in", LAT_ASM, 1, f, "in")
        cid("cid-asm-none", LAT_ASM, 1, f, "none")
        # form 0: no ctext buffer, or a block size that is a multiple of 16
        # but not of 64 (otherwise the latency route decrypts and hashes)
        cid("cid-c-none", LAT_C, 1, 0, "none")
        cid("cid-c-out", LAT_C, 1, 0, "out", bs_delta=-16)
        cid("cid-c-out-keyed", LAT_C, 1, 0, "out", bs_delta=-16, keyed=True)
        cid("cid-c-in", LAT_C, 1, 0, "in", bs_delta=-16)
        for off in (1, 4, 8):
            cid("cid-bytes-src%d" % off, LAT_ASM, 0, 2, "out", src_off=off)
        cid("cid-bytes-ct3", LAT_ASM, 0, 2, "out", ct_off=3)
        cid("cid-bytes-bs-1", LAT_ASM, 0, 2, "out", bs_delta=-1)
        cid("cid-bytes-bs-1-keyed", LAT_ASM, 0, 2, "out", bs_delta=-1, keyed=True)
    return rows


PASS_ROWS = _pass_rows()
PASS_GROUPS = ("dek", "cid-asm", "cid-c", "cid-bytes")

# k_pass<G, true, true, 2> with G >= 4 exists only with split_log2 > 0:
# glfsx_post_batch_device (never fuses) over two blocks at latency_wgs(0)
# with a split target T, n < T <= 2n, halves G once; T = 16 three times.
# G = 64 splits by size alone (blocks above 16 MiB).  Each call logs the DEK
# pass and the CID pass.  A last block shorter than a workgroup's span leaves
# the sub-ranges after the first empty.
SplitRow = collections.namedtuple("SplitRow", "name bs target g sl")
SPLIT_ROWS = [
    SplitRow("g4-sl1", 2 * MIB, 4, 4, 1),
    SplitRow("g8-sl1", 4 * MIB, 4, 8, 1),
    SplitRow("g16-sl1", 8 * MIB, 4, 16, 1),
    SplitRow("g32-sl1", 16 * MIB, 4, 32, 1),
    SplitRow("g64-sl1", 32 * MIB, 0, 64, 1),
    SplitRow("g4-sl3", 8 * MIB, 16, 4, 3),
]


def split_expect(row):
    grid = 2 << row.sl
    return [rec(PASS, row.g, 0, 1, 2, row.sl, grid, 2), rec(PASS, row.g, 1, 1, 2, row.sl, grid, 2)]


# k_quad through the DEK entry point in latency mode, split target 0: two
# blocks, except 16 MiB (two of them are more than 16384 chunks), which is
# posted alone.  quad_qpw gives 256 quads only above 4 MiB, where a block
# spans at least 17 workgroups: k_quad<256> without split is not reachable.
QuadRow = collections.namedtuple("QuadRow", "name bs blocks qpw sl")
QUAD_ROWS = [
    QuadRow("64k", 64 * KIB, 2, 64, 0),
    QuadRow("64k+1k", 64 * KIB + 1024, 2, 64, 1),
    QuadRow("4m", 4 * MIB, 2, 64, 6),
    QuadRow("4m+64", 4 * MIB + 64, 2, 256, 5),
    QuadRow("16m", 16 * MIB, 1, 256, 6),
]
SMALL_LENS = (1, 63, 64, 65, 1023, 1024, 1025)


def quad_expect(row, length):
    if row.blocks == 1 and length <= 64 * KIB:   # one short block alone: no split
        return rec(QUAD, 64, 0, 1, 0, 0, 1, 1)
    return rec(QUAD, row.qpw, 0, 1, 0, row.sl, row.blocks << row.sl, row.blocks)


# k_pass_dc through glfsx_post_batch (host buffers; the synchronising call
# may fuse) at latency_wgs(0) and a split target of 2n: g = 1, 2, 4 at
# split_log2 = 1.  17 whole blocks and a ragged one.
DcRow = collections.namedtuple("DcRow", "g bs fine_div")
DC_ROWS = [DcRow(1, 512 * KIB, 0), DcRow(2, MIB, 4), DcRow(4, 2 * MIB, 4)]
DC_BLOCKS = 18
DC_LISTS = 8                                 # kLists (pass_kernels.h)


def dc_lists(n, fine_div):
    """(coarse CID messages, fine CID messages) of each work list."""
    out = []
    for x in range(DC_LISTS):
        m = (n - x + DC_LISTS - 1) // DC_LISTS if n > x else 0
        f = -(-m // fine_div) if fine_div else 0
        out.append((m - f, f))
    return out


def dc_expect(row):
    items = sum((2 * (c + f) + f) << 1 for c, f in dc_lists(DC_BLOCKS, row.fine_div))
    return rec(PASS_DC, row.g, 1, 1, 2, 1, items, DC_BLOCKS, row.fine_div, items)


# k_open (the one-pass verified read, route 2): three blocks, the last ragged.
OpenRow = collections.namedtuple("OpenRow", "g bs aligned")
OPEN_ROWS = [OpenRow(g, 256 * g * KIB, a) for g in (1, 2, 4, 8) for a in (1, 0)]


def open_expect(row):
    return rec(OPEN, row.g, 1, row.aligned, 2, 0, 3, 3)


def table_kernels():
    ks = {kernel_of(r.expect) for r in PASS_ROWS}
    for r in SPLIT_ROWS:
        ks |= {kernel_of(e) for e in split_expect(r)}
    for r in QUAD_ROWS:
        ks |= {kernel_of(quad_expect(r, n)) for n in SMALL_LENS + (r.bs,)}
    ks |= {kernel_of(dc_expect(r)) for r in DC_ROWS}
    ks |= {kernel_of(open_expect(r)) for r in OPEN_ROWS}
    return ks


# ------------------------------------------------------------- the meta-test
def _sweep_program(tmp_path):
    """tests/c/launch_plan_sweep.cpp, built with the host compiler under
    AddressSanitizer and UBSan (as tests/test_host_units.py builds its
    programs): its own main, nothing loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    out = str(tmp_path / "launch_plan_sweep")
    subprocess.check_call(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-I", CSRC,
         os.path.join(ROOT, "tests", "c", "launch_plan_sweep.cpp"), "-o", out])
    return out


def _run(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "launch_plan_sweep: ok" in p.stdout
    assert p.stderr == "", p.stderr  # the sanitizers report nothing
    return p.stdout


@pytest.fixture(scope="module")
def sweep_program(tmp_path_factory):
    return _sweep_program(tmp_path_factory.mktemp("sweep"))


def reachable_kernels(program):
    """What launch_plan.h's pure functions return over a sweep of shapes,
    alignments and knob values.  The program itself fails unless that set is
    the constexpr launchable set the dispatchers instantiate."""
    return {tuple(int(x) for x in ln.split()[1:]) for ln in _run([program]).splitlines()
            if ln.startswith("K ")}


def test_table_covers_the_reachable_set(sweep_program):
    want, have = reachable_kernels(sweep_program), table_kernels()
    assert have == want, (sorted(want - have), sorted(have - want))
    assert len(want) == 60
    assert len({(r.g, r.name) for r in PASS_ROWS}) == len(PASS_ROWS)
    # every k_pass row belongs to one parametrised group
    assert all(sum(r.name.startswith(p + "-") or r.name == p for p in PASS_GROUPS) == 1
               for r in PASS_ROWS)


def test_selection_matches_the_recorded_launches(sweep_program):
    """tests/golden/launch_records.txt: what the library launched for a fixed
    list of calls (scripts/record_launches.py) before the selection moved
    into launch_plan.h.  The pure functions give exactly those records."""
    fixture = os.path.join(ROOT, "tests", "golden", "launch_records.txt")
    n = sum(1 for _ in open(fixture))
    assert n >= 200
    assert "replayed %d\n" % n in _run([sweep_program, fixture])


def test_log_hook_needs_no_device():
    """The hook reads a host-side log: it answers in a process that never
    touches the GPU, and rejects a capacity without a buffer."""
    from glfs_amd import _native as N
    n = ctypes.c_size_t(77)
    buf = (ctypes.c_uint32 * LOG_WORDS)()
    assert N.lib.glfsx_debug_pass_log(0, buf, 1, ctypes.byref(n)) == 0
    assert N.lib.glfsx_debug_pass_log(0, None, 0, None) == 0
    assert N.lib.glfsx_debug_pass_log(0, None, 1, None) == N.GLFSX_E_ARG


# ------------------------------------------------------------------- helpers
def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def log_reset(N):
    N.check(N.lib.glfsx_debug_pass_log(1, None, 0, None))


def log_take(N, cap=64):
    buf = (ctypes.c_uint32 * (LOG_WORDS * cap))()
    n = ctypes.c_size_t()
    N.check(N.lib.glfsx_debug_pass_log(1, buf, cap, ctypes.byref(n)))
    assert n.value <= cap, n.value
    return [tuple(buf[i * LOG_WORDS:(i + 1) * LOG_WORDS]) for i in range(n.value)]


@pytest.fixture
def knobs():
    """Sets latency_wgs / split_target / open_route; restores all three."""
    from glfs_amd import _native as N
    old = (N.set_latency_wgs(512), N.set_split_target(2048), N.set_open_route(0))
    N.set_latency_wgs(old[0])
    N.set_split_target(old[1])
    N.set_open_route(old[2])

    def set_(latency_wgs=None, split_target=None, open_route=None):
        if latency_wgs is not None:
            N.set_latency_wgs(latency_wgs)
        if split_target is not None:
            N.set_split_target(split_target)
        if open_route is not None:
            N.set_open_route(open_route)
    yield set_
    N.set_latency_wgs(old[0])
    N.set_split_target(old[1])
    N.set_open_route(old[2])


def to_dev(torch, b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def to_host(t):
    return bytes(t.cpu().numpy().tobytes())


def assert_same(torch, got, want, what):
    """torch.equal on the device; bytes come back only to report."""
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero().flatten()
    i = int(bad[0])
    raise AssertionError("%s: %d bytes differ, the first at %d (last at %d): got %s want %s" % (
        what, bad.numel(), i, int(bad[-1]), to_host(got[i:i + 16]).hex(),
        to_host(want[i:i + 16]).hex()))


def last_lens(g, bs):
    c = g * 1024
    lens = list(SMALL_LENS) + [c - 1, c, c + 1, 64 * c - 1, 64 * c,
                               (69 * g + g // 2) * 1024 + 199, bs - 1, bs]
    assert all(0 < n <= bs for n in lens)
    return sorted(set(lens))


class PassData:
    """The input of G's k_pass rows and its oracle values, made once.  The
    blocks end at P: the last block of every row is data[P:P + L], the one
    before it data[P - bs':P], whatever the row's block size bs'."""

    def __init__(self, torch, O, g):
        self.torch, self.O, self.g = torch, O, g
        self.bs = bs_of(g)
        self.blocks = dek_blocks_c(g)
        self.P = (self.blocks - 1) * self.bs
        self.data = O.fill_splitmix(self.blocks * self.bs, 1000 + g)
        self.dev = to_dev(torch, self.data + bytes(256))   # (room behind the last block)
        rng = random.Random(g)
        self.dek0 = bytes(rng.randrange(256) for _ in range(32))
        self.dek1 = bytes(rng.randrange(256) for _ in range(32))
        self.ct1 = O.chacha20_xor(self.data[self.P:], self.dek1)
        self.ct1_dev = to_dev(torch, self.ct1)

    def block0(self, bs):
        return self.data[self.P - bs:self.P]

    @functools.lru_cache(maxsize=None)
    def ct0_dev(self, bs):
        return to_dev(self.torch, self.O.chacha20_xor(self.block0(bs), self.dek0))

    @functools.lru_cache(maxsize=None)
    def cid0(self, bs, keyed):
        return self.O.blake3(to_host(self.ct0_dev(bs)), CID_KEY if keyed else None)

    @functools.lru_cache(maxsize=None)
    def cid1(self, length, keyed):
        return self.O.blake3(self.ct1[:length], CID_KEY if keyed else None)

    @functools.lru_cache(maxsize=None)
    def dek_of(self, start, length):
        return self.O.blake3(self.data[start:start + length], SALT)


@functools.lru_cache(maxsize=None)
def pass_data(g):
    from oracle import oracle as O
    return PassData(_torch(), O, g)


def run_pass_row(N, torch, pd, row, knobs):
    bs = pd.bs + row.bs_delta
    knobs(row.lat, 0)
    poison_refs = bytes([POISON]) * 32
    if row.blocks == 2:
        # the two blocks at 64 + src_off of a poisoned work buffer
        a = 64 + row.src_off
        work0 = torch.full((a + 2 * bs + 128,), POISON, dtype=torch.uint8, device="cuda")
        work0[a:a + 2 * bs] = pd.dev[pd.P - bs:pd.P + bs]
        work = work0.clone()
    else:
        assert row.bs_delta == 0 and row.src_off == 0 and not row.chacha
        a, work0, work = 0, pd.dev, pd.dev
    if row.ctext == "out":
        c = 64 + row.ct_off
        out = torch.empty(c + 2 * bs + 128, dtype=torch.uint8, device="cuda")
        out0 = torch.full_like(out, POISON)
    elif row.ctext == "in":
        c, out, out0 = a, work, work0
    want = out0.clone() if row.ctext in ("out", "in") else None
    for length in last_lens(pd.g, bs):
        what = "G=%d %s L=%d" % (pd.g, row.name, length)
        total = (row.blocks - 1) * bs + length
        if row.ctext in ("out", "in"):
            out.copy_(out0)
        refs0 = bytearray([POISON]) * (64 * row.blocks)
        if row.chacha:
            refs0[32:64], refs0[96:128] = pd.dek0, pd.dek1
        refs = to_dev(torch, refs0)
        torch.cuda.synchronize()
        log_reset(N)
        if row.chacha:
            N.check(N.lib.glfsx_cid_batch_device(
                work.data_ptr() + a, total, bs,
                out.data_ptr() + c if row.ctext in ("out", "in") else None,
                refs.data_ptr(), CID_KEY if row.keyed else None, None))
        else:
            N.check(N.lib.glfsx_dek_batch_device(SALT, work.data_ptr() + a, total, bs,
                                                 refs.data_ptr(), None))
        torch.cuda.synchronize()
        assert log_take(N) == [row.expect], what
        got = to_host(refs)
        if row.chacha:
            exp = (pd.cid0(bs, row.keyed) + pd.dek0 + pd.cid1(length, row.keyed) + pd.dek1)
        else:
            exp = b"".join(poison_refs + pd.dek_of(pd.P - (row.blocks - 1 - j) * bs, bs)
                           for j in range(row.blocks - 1))
            exp += poison_refs + pd.dek_of(pd.P, length)
        assert got == exp, (what, [j for j in range(0, len(exp), 32) if got[j:j + 32] != exp[j:j + 32]])
        if want is not None:
            # ctext of both blocks, the bytes around it (64 poisoned guard
            # bytes before, the rest of the buffer behind) untouched
            want.copy_(out0)
            want[c:c + bs] = pd.ct0_dev(bs)
            want[c + bs:c + bs + length] = pd.ct1_dev[:length]
            assert_same(torch, out, want, what + " ctext")
        if row.ctext != "in" and row.blocks == 2:
            assert_same(torch, work, work0, what + " source")


# ------------------------------------------------------------------- k_pass
@gpu_test
@pytest.mark.parametrize("group", PASS_GROUPS)
@pytest.mark.parametrize("g", GS)
def test_k_pass(gpu, O, knobs, g, group):
    torch = _torch()
    pd = pass_data(g)
    rows = [r for r in PASS_ROWS if r.g == g and r.name.startswith(group)]
    assert rows
    for row in rows:
        run_pass_row(gpu, torch, pd, row, knobs)


def split_lens(row):
    span = 256 * row.g * KIB
    lens = [1, 1025, row.g * 1024 + 1, span - 1, span, span + 1,
            span + (69 * row.g + row.g // 2) * 1024 + 199, row.bs - 1, row.bs]
    if row.sl > 1:
        lens += [3 * span + 5, ((1 << row.sl) - 1) * span, ((1 << row.sl) - 1) * span + 1]
    assert all(0 < n <= row.bs for n in lens)
    return sorted(set(lens))


@gpu_test
@pytest.mark.parametrize("row", SPLIT_ROWS, ids=lambda r: r.name)
def test_k_pass_split(gpu, O, knobs, row):
    """Both passes in split mode: the refs (DEK from the data, CID of the
    ctext under that DEK) and every ctext byte, out of place."""
    torch = _torch()
    N, bs = gpu, row.bs
    data = O.fill_splitmix(2 * bs, 2000 + row.g + row.sl)
    src = to_dev(torch, data + bytes(256))
    knobs(LAT_ASM, row.target)
    dek0 = O.blake3(data[:bs], SALT)
    ct0 = O.chacha20_xor(data[:bs], dek0)
    ct0_dev = to_dev(torch, ct0)
    cid0 = {None: O.blake3(ct0), CID_KEY: O.blake3(ct0, CID_KEY)}
    out = torch.empty(64 + 2 * bs + 128, dtype=torch.uint8, device="cuda")
    want = torch.empty_like(out)
    lens = split_lens(row)
    for i, length in enumerate(lens):
        key = CID_KEY if i % 2 else None     # keyed and unkeyed CIDs in turn
        what = "%s L=%d" % (row.name, length)
        out.fill_(POISON)
        refs = torch.full((128,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        log_reset(N)
        N.check(N.lib.glfsx_post_batch_device(SALT, src.data_ptr(), bs + length, bs,
                                              out.data_ptr() + 64, refs.data_ptr(), key, None))
        torch.cuda.synchronize()
        assert log_take(N) == split_expect(row), what
        dek1 = O.blake3(data[bs:bs + length], SALT)
        ct1 = O.chacha20_xor(data[bs:bs + length], dek1)
        exp = cid0[key] + dek0 + O.blake3(ct1, key) + dek1
        got = to_host(refs)
        assert got == exp, (what, [j for j in range(0, 128, 32) if got[j:j + 32] != exp[j:j + 32]])
        want.fill_(POISON)
        want[64:64 + bs] = ct0_dev
        want[64 + bs:64 + bs + length] = to_dev(torch, ct1)
        assert_same(torch, out, want, what + " ctext")


# ------------------------------------------------------------------- k_quad
@gpu_test
@pytest.mark.parametrize("row", QUAD_ROWS, ids=lambda r: r.name)
def test_k_quad(gpu, O, knobs, row):
    torch = _torch()
    N, bs = gpu, row.bs
    data = O.fill_splitmix(row.blocks * bs, 3000 + bs)
    src = to_dev(torch, data + bytes(256))
    knobs(LAT_C, 0)
    first = bs * (row.blocks - 1)
    for length in sorted(set(SMALL_LENS + (bs - 1, bs))):
        what = "%s L=%d" % (row.name, length)
        refs = torch.full((64 * row.blocks,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        log_reset(N)
        N.check(N.lib.glfsx_dek_batch_device(SALT, src.data_ptr(), first + length, bs,
                                             refs.data_ptr(), None))
        torch.cuda.synchronize()
        assert log_take(N) == [quad_expect(row, length)], what
        blocks = [data[:bs]] * (row.blocks - 1) + [data[first:first + length]]
        exp = b"".join(bytes([POISON]) * 32 + O.blake3(b, SALT) for b in blocks)
        assert to_host(refs) == exp, what


# ---------------------------------------------------------------- k_pass_dc
@gpu_test
@pytest.mark.parametrize("row", DC_ROWS, ids=lambda r: "g%d" % r.g)
def test_k_pass_dc(gpu, O, knobs, row):
    """The one-launch split post: every ref and every ctext byte, unkeyed and
    keyed, each twice back to back (the ready flags carry an epoch)."""
    N, bs = gpu, row.bs
    total = (DC_BLOCKS - 1) * bs + bs // 2 + 12345
    data = O.fill_splitmix(total, 4000 + row.g)
    knobs(LAT_ASM, 2 * DC_BLOCKS)
    expect = dc_expect(row)
    posts = [O.post(SALT, data[o:o + bs]) for o in range(0, total, bs)]
    want_ct = b"".join(c for _, c in posts)
    for key in (None, None, CID_KEY, CID_KEY):
        refs = ctypes.create_string_buffer(bytes([POISON]) * (64 * DC_BLOCKS), 64 * DC_BLOCKS)
        ct = ctypes.create_string_buffer(total)
        log_reset(N)
        N.check(N.lib.glfsx_post_batch(SALT, data, total, bs, ct, refs, key))
        log = log_take(N)
        assert log == [expect], key
        if row.g > 1:
            # from the logged counts (messages, fine_div): some work list
            # holds both a coarse and a fine CID item
            assert any(c and f for c, f in dc_lists(log[0][9], log[0][7]))
        for j, (r, c) in enumerate(posts):
            cid = O.blake3(c, key) if key else r[:32]
            assert refs.raw[64 * j:64 * j + 64] == cid + r[32:], (key, j)
        assert ct.raw == want_ct, key


# -------------------------------------------------------------------- k_open
@gpu_test
@pytest.mark.parametrize("row", OPEN_ROWS, ids=lambda r: "g%d-%s" % (r.g, "aligned" if r.aligned
                                                                      else "bytes"))
def test_k_open(gpu, O, knobs, row):
    """The one-pass verified read of what the oracle posted: clean input is
    good and decrypts to the data; one flipped ctext bit fails its block."""
    torch = _torch()
    N, bs = gpu, row.bs
    total = 2 * bs + 8191
    data = O.fill_splitmix(total, 5000 + row.g)
    posts = [O.post(SALT, data[o:o + bs]) for o in range(0, total, bs)]
    refs = to_dev(torch, b"".join(r for r, _ in posts))
    ctext = b"".join(c for _, c in posts)
    off = 0 if row.aligned else 1
    knobs(open_route=2)
    for flip in (None, bs + 77):
        ct = bytearray(bytes(64 + off) + ctext + bytes(64))
        if flip is not None:
            ct[64 + off + flip] ^= 0x20
        d_ct = to_dev(torch, ct)
        d_pt = torch.full((64 + off + total + 64,), POISON, dtype=torch.uint8, device="cuda")
        d_st = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        log_reset(N)
        N.check(N.lib.glfsx_open_batch_device(SALT, None, d_ct.data_ptr() + 64 + off, total, bs,
                                              refs.data_ptr(), d_pt.data_ptr() + 64 + off,
                                              d_st.data_ptr(), None))
        torch.cuda.synchronize()
        assert log_take(N) == [open_expect(row)], flip
        assert d_st.cpu().tolist() == ([0, 0, 0] if flip is None else [0, 3, 0])
        pt = to_host(d_pt)
        guard = bytes([POISON]) * (64 + off)
        assert pt[:64 + off] == guard and pt[64 + off + total:] == bytes([POISON]) * 64
        body = pt[64 + off:64 + off + total]
        if flip is None:
            assert body == data
        else:
            assert body[:bs] == data[:bs] and body[2 * bs:] == data[2 * bs:]
