"""Which bulk kernels a fixed list of C-ABI calls launches, one line per call:
the inputs, then the records of glfsx_debug_pass_log.

    python scripts/record_launches.py OUT

tests/golden/launch_records.txt is this script's output at the commit before
the kernel selection moved into launch_plan.h; tests/c/launch_plan_sweep.cpp
replays it on the CPU (the line format is documented there), and a run of
this script at a later commit must reproduce it byte for byte.  The list
reaches every instantiation of k_pass, k_quad, k_pass_dc and k_open and has
a call on each side of every threshold the selection names.  Data is never
initialised: only the launches matter.  Needs a GPU; takes seconds.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
DEK, CID, POST_DEV, POST_HOST, CREATE, OPEN = 1, 2, 3, 4, 5, 6
LAT_C = 1 << 31
SALT = bytes(range(7, 39))
KEY = bytes(range(101, 133))
WORDS = 10


def case(entry, n, bs, last=None, src_off=0, ct_off=0, refs_off=0, ctmode=0, flag=0, lat=512,
         split=2048, route=0):
    return (entry, n, bs, bs if last is None else last, src_off, ct_off, refs_off, ctmode, flag,
            lat, split, route)


def cases():
    out = []
    gs = (1, 2, 4, 8, 16, 32, 64)
    # every k_pass instantiation: the shapes of tests/test_gpu_pass_matrix.py
    for g in gs:
        bs = 256 * g * KIB
        out.append(case(DEK, 2, bs, bs - 5, lat=0, split=0))
        out.append(case(DEK, 64 // g + 1, bs, 1, lat=LAT_C, split=0))
        out.append(case(DEK, 2, bs, src_off=4, lat=0, split=0))
        out.append(case(DEK, 2, bs - 1, lat=0, split=0))
        out.append(case(DEK, 2, bs, refs_off=2, lat=LAT_C, split=0))     # refs not 4-aligned: no quad
        for ctmode in (0, 1, 2):
            out.append(case(CID, 2, bs, 77, ctmode=ctmode, flag=ctmode & 1, lat=0, split=0))
        out.append(case(CID, 2, bs, ctmode=0, lat=LAT_C, split=0))
        out.append(case(CID, 2, bs - 16, ctmode=1, lat=LAT_C, split=0))
        out.append(case(CID, 2, bs, ctmode=1, lat=LAT_C, split=0))       # keystream + BLAKE3 pass
        out.append(case(CID, 2, bs, src_off=8, ctmode=1, lat=0, split=0))
        out.append(case(CID, 2, bs, ct_off=3, ctmode=1, lat=0, split=0))
        out.append(case(CID, 2, bs - 1, ctmode=1, flag=1, lat=0, split=0))
    # k_pass with a split: by the target, and by size alone
    for bs, target in ((2 * MIB, 4), (4 * MIB, 4), (8 * MIB, 4), (16 * MIB, 4), (32 * MIB, 0),
                       (8 * MIB, 16)):
        out.append(case(POST_DEV, 2, bs, bs // 3, ctmode=1, lat=0, split=target))
    # the split target, either side: n << sl < target
    for target in (3, 4, 5, 8, 9):
        out.append(case(POST_DEV, 2, 2 * MIB, ctmode=1, lat=0, split=target))
    # G >= 4 without split runs form 1, with one form 2; G < 4 form 2
    for bs in (512 * KIB, MIB, 2 * MIB):
        for target in (0, 3):
            out.append(case(CID, 2, bs, ctmode=1, lat=0, split=target))
    # latency_wgs, either side, at one workgroup per block and at a split
    for lat in (1, 2, 3):
        out.append(case(DEK, 2, MIB, refs_off=2, lat=lat, split=0))
        out.append(case(CID, 2, MIB, ctmode=0, lat=lat, split=0))
        out.append(case(CID, 2, MIB, ctmode=1, lat=lat, split=0))
    for lat in (7, 8, 9):
        out.append(case(POST_DEV, 2, 4 * MIB, ctmode=1, lat=lat, split=8))
    # the latency route of the CID side needs 64-byte blocks, dense refs, a ctext
    for bs in (MIB - 64, MIB - 32):
        out.append(case(CID, 3, bs, ctmode=1))
    out.append(case(CID, 1, 4 * MIB, 4 * MIB - 3, ctmode=1))
    out.append(case(CID, 1, 4 * MIB, 100, ctmode=2))
    # k_quad: both instantiations; 4 MiB, 16 MiB and 16384 chunks, either side
    for bs, n in ((64 * KIB, 2), (64 * KIB + 1024, 2), (4 * MIB, 2), (4 * MIB + 64, 2),
                  (16 * MIB, 1), (16 * MIB + 64, 1), (8 * MIB, 2), (8 * MIB + 1024, 2),
                  (KIB, 16384), (KIB, 16385), (64 * KIB, 256), (64 * KIB, 257)):
        out.append(case(DEK, n, bs, lat=LAT_C, split=0))
        out.append(case(DEK, n, bs))
    out.append(case(DEK, 2, 64 * KIB, src_off=1, lat=LAT_C, split=0))
    out.append(case(DEK, 1, 64 * KIB, 7, lat=LAT_C, split=0))
    # k_pass_dc: G = 1, 2, 4 (tests/test_gpu_pass_matrix.py), through the host entry point
    for bs in (512 * KIB, MIB, 2 * MIB):
        out.append(case(POST_HOST, 18, bs, bs // 2 + 12345, ctmode=1, lat=0, split=36))
        out.append(case(POST_DEV, 18, bs, bs // 2 + 12345, ctmode=1, lat=0, split=36))
    # ... 5/8 of latency_wgs, either side: 36 workgroups against 57, 58 (* 5 / 8 = 35, 36)
    for lat in (56, 57, 58, 64):
        out.append(case(POST_HOST, 18, MIB, ctmode=1, lat=lat, split=36))
    # ... and at the defaults: 5/8 of 512 = 320 workgroups, kDcMinWgs = 1024
    for n in (64, 80, 81, 127, 128, 255, 256):
        out.append(case(POST_HOST, n, MIB, ctmode=1))
    for n in (100, 127, 128, 129):
        out.append(case(CREATE, n, 2 * MIB, 2 * MIB - 7, ctmode=1))
    # Create: one block, an index level, two index levels (bf = 64 at 4 KiB blocks)
    out.append(case(CREATE, 1, MIB, 12345, ctmode=1))
    out.append(case(CREATE, 1, MIB, 12345, ctmode=0))
    out.append(case(CREATE, 4, MIB, 5, ctmode=1))
    out.append(case(CREATE, 512, MIB, ctmode=0))
    out.append(case(CREATE, 2048, MIB, ctmode=1))
    out.append(case(CREATE, 4097, 4 * KIB, 1, ctmode=1))
    out.append(case(CREATE, 70000, 4 * KIB, ctmode=0))
    out.append(case(CREATE, 3, 64 * KIB, src_off=4, ctmode=1))
    # the headline shape and config 2's, device to device
    out.append(case(POST_DEV, 2048, MIB, ctmode=1))
    out.append(case(POST_DEV, 512, 2 * MIB, ctmode=1))
    out.append(case(POST_DEV, 512, 2 * MIB, ctmode=2, src_off=0))
    # k_open: every instantiation (route 2), then auto either side of 1024
    # blocks, 256 KiB blocks and 1 GiB, and the composed route
    for g in (1, 2, 4, 8):
        for off in (0, 1):
            out.append(case(OPEN, 3, 256 * g * KIB, 8191, src_off=off, ct_off=off, ctmode=1,
                            flag=1, route=2))
    out.append(case(OPEN, 3, 2 * MIB + 64, ctmode=1, flag=1, route=2))    # above k_open's blocks
    out.append(case(OPEN, 3, MIB, ctmode=1, flag=0, route=2))             # unsalted: composed
    out.append(case(OPEN, 3, MIB, ctmode=1, flag=1, route=1))
    for n, bs in ((1024, MIB), (1023, MIB), (4096, 256 * KIB), (4095, 256 * KIB),
                  (4200, 256 * KIB - 64), (1024, 512 * KIB), (2048, 512 * KIB)):
        out.append(case(OPEN, n, bs, ctmode=1, flag=1))
    out.append(case(OPEN, 1024, MIB, ctmode=0, flag=1))
    out.append(case(OPEN, 1024, MIB, ctmode=2, flag=1))
    out.append(case(OPEN, 2, 64 * KIB, ctmode=1, flag=1))
    out.append(case(OPEN, 2, 64 * KIB, ctmode=0, flag=0))
    return out


def main(path):
    import torch
    from glfs_amd import _native as N
    assert torch.cuda.is_available()
    N.set_device(0)
    old = (N.set_latency_wgs(512), N.set_split_target(2048), N.set_open_route(0))
    # the first Create under a salt also derives that salt's keys: not recorded
    warm = torch.empty(4096, dtype=torch.uint8, device="cuda")
    N.check(N.lib.glfsx_create_device(4096, None, None, warm.data_ptr(), 4096, None,
                                      ctypes.byref(N.glfsx_root()), None, None))
    lines = []
    buf = (ctypes.c_uint32 * (WORDS * 64))()
    count = ctypes.c_size_t()
    for c in cases():
        entry, n, bs, last, src_off, ct_off, refs_off, ctmode, flag, lat, split, route = c
        total = (n - 1) * bs + last
        assert 0 < last <= bs and 2 * total <= 4 * GIB
        N.set_latency_wgs(lat)
        N.set_split_target(split)
        N.set_open_route(route)
        src = torch.empty(total + 256, dtype=torch.uint8, device="cuda")
        refs = torch.empty(64 * n + 64, dtype=torch.uint8, device="cuda")
        p_src, p_refs = src.data_ptr() + src_off, refs.data_ptr() + refs_off
        dst, p_dst = None, None
        if ctmode == 1:
            dst = torch.empty(total + 256, dtype=torch.uint8, device="cuda")
            p_dst = dst.data_ptr() + ct_off
        elif ctmode == 2:
            p_dst = p_src
        key = KEY if flag else None
        torch.cuda.synchronize()
        N.check(N.lib.glfsx_debug_pass_log(1, None, 0, None))
        if entry == DEK:
            rc = N.lib.glfsx_dek_batch_device(SALT, p_src, total, bs, p_refs, None)
        elif entry == CID:
            rc = N.lib.glfsx_cid_batch_device(p_src, total, bs, p_dst, p_refs, key, None)
        elif entry == POST_DEV:
            rc = N.lib.glfsx_post_batch_device(SALT, p_src, total, bs, p_dst, p_refs, key, None)
        elif entry == POST_HOST:
            host = ctypes.create_string_buffer(total)
            h_ct = ctypes.create_string_buffer(total)
            h_refs = ctypes.create_string_buffer(64 * n)
            rc = N.lib.glfsx_post_batch(SALT, host, total, bs, h_ct, h_refs, key)
        elif entry == CREATE:
            root = N.glfsx_root()
            rc = N.lib.glfsx_create_device(bs, None, key, p_src, total, p_dst, ctypes.byref(root),
                                           None, None)
        else:
            status = torch.empty(n, dtype=torch.int32, device="cuda")
            rc = N.lib.glfsx_open_batch_device(SALT if flag else None, None, p_src, total, bs,
                                               p_refs, p_dst, status.data_ptr(), None)
        N.check(rc)
        torch.cuda.synchronize()
        N.check(N.lib.glfsx_debug_pass_log(1, buf, 64, ctypes.byref(count)))
        assert count.value <= 64, count.value
        words = list(buf[:WORDS * count.value])
        lines.append(" ".join(str(x) for x in list(c) + [count.value] + words))
        del src, refs, dst
    N.set_latency_wgs(old[0])
    N.set_split_target(old[1])
    N.set_open_route(old[2])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    kernels = {tuple(int(x) for x in ln.split()[13 + WORDS * i:18 + WORDS * i])
               for ln in lines for i in range(int(ln.split()[12]))}
    print("%d calls, %d distinct kernels" % (len(lines), len(kernels)))


# ---- the ragged passes and the one-shot classes (glfsx_debug_aux_log) ----
# tests/golden/aux_launch_records.txt is main_aux's output from a build of the
# old launchers (launch_rag_pass, launch_rag_open_pass, the one / med /
# one-open ladders) with nothing added but an append after each launch of the
# record of what that launcher had just launched, written out by hand there.
# That build was never a commit of its own (the launchers went away in the
# commit that added this function), so git cannot reproduce the fixture; what
# can be repeated is the check that matters from here on: a run of this
# function at any later commit must reproduce the file byte for byte.
# launch_plan_sweep replays it against rag_pass_recs and one_rec.  The rows
# with two requests exist for the post classes only (a Writer's Finish): no
# entry point opens several blocks in one call.  A line is one ragged pass,
#   R chunks groups large kind latency_wgs nrec <records>
# (kind: 0 the post's DEK pass, 1 its CID pass, 2 + mode the open), or one
# one-shot class launch,
#   O class n max_len nrec <records>
# (class: OneClass of one_classes.h).  The inputs are what this script asked
# for, never read back from the records.
RAG_CHUNK, RAG_A, RAG_B, ONE, MED, ONE_OPEN = 9, 10, 11, 12, 13, 14
ONE_SMALL, ONE_MED, ONE_OPEN_CLS, ONE_OPEN_SALTED = 0, 1, 2, 3


def rag_totals(lens):
    c = [max(1, -(-ln // 1024)) for ln in lens]
    return (sum(c), sum(-(-x // 256) for x in c if x > 1), sum(x > 256 for x in c))


def rag_cases():
    big = 16 * MIB
    return [
        [1000],                                  # one chunk: no merge level
        [0, 1, 1024, 5],                         # one-chunk messages only
        [1, 2000, 1024],                         # level A alone
        [256 * KIB, 1025],                       # 256 chunks: still no level B
        [256 * KIB + 1],                         # 257 chunks: both levels
        [300 * KIB, 7, 5 * MIB + 77, 2048],
        [255 * KIB, 1024],                       # 256 chunks in all: one tile
        [255 * KIB, 1025],                       # 257: two tiles
        [big] * 8,                               # 512 tiles: the default latency bound
        [big] * 8 + [1],                         # 513 tiles
    ]


def aux_take(N, buf, count):
    N.check(N.lib.glfsx_debug_aux_log(1, buf, 64, ctypes.byref(count)))
    assert count.value <= 64, count.value
    return [list(buf[WORDS * i:WORDS * i + WORDS]) for i in range(count.value)]


def main_aux(path):
    import torch
    from glfs_amd import _native as N
    assert torch.cuda.is_available()
    N.set_device(0)
    old = (N.set_latency_wgs(512), N.set_open_route(0))
    buf = (ctypes.c_uint32 * (WORDS * 64))()
    count = ctypes.c_size_t()
    lines = []

    def row(head, recs):
        lines.append(" ".join(str(x) for x in list(head) + [len(recs)] + sum(recs, [])))

    # ragged: the post's two passes and the open in its three modes
    for lens in rag_cases():
        offs, o = [], 0
        for ln in lens:
            offs.append(o)
            o += (ln + 63) & ~63
        n, tot = len(lens), rag_totals(lens)
        data = torch.empty(o + 64, dtype=torch.uint8, device="cuda")
        out = torch.empty(o + 64, dtype=torch.uint8, device="cuda")
        refs = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        do = torch.tensor(offs, dtype=torch.int64, device="cuda")
        dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
        for lat in (512, 0, 1):
            N.set_latency_wgs(lat)
            torch.cuda.synchronize()
            N.check(N.lib.glfsx_debug_aux_log(1, None, 0, None))
            N.check(N.lib.glfsx_post_ragged_device(SALT, None, data.data_ptr(), do.data_ptr(),
                                                   dl.data_ptr(), n, max(lens), out.data_ptr(),
                                                   refs.data_ptr(), None))
            torch.cuda.synchronize()
            log = aux_take(N, buf, count)
            assert all(r[0] in (RAG_CHUNK, RAG_A, RAG_B) for r in log), log
            starts = [i for i, r in enumerate(log) if r[0] == RAG_CHUNK]
            assert len(starts) == 2, log
            row(("R",) + tot + (0, lat), log[:starts[1]])
            row(("R",) + tot + (1, lat), log[starts[1]:])
            for mode in (0, 1, 2):
                N.check(N.lib.glfsx_debug_aux_log(1, None, 0, None))
                N.check(N.lib.glfsx_open_ragged_device(
                    SALT if mode == 2 else None, None, data.data_ptr(), do.data_ptr(),
                    dl.data_ptr(), n, max(lens), refs.data_ptr(),
                    out.data_ptr() if mode else None, status.data_ptr(), None))
                torch.cuda.synchronize()
                row(("R",) + tot + (2 + mode, lat), aux_take(N, buf, count))
        del data, out
    N.set_latency_wgs(512)

    # one-shot, one request: glfsx_post and glfsx_open pass the descriptor by value
    host = ctypes.create_string_buffer(4 * MIB + 64)
    h_ct = ctypes.create_string_buffer(4 * MIB + 64)
    ref = ctypes.create_string_buffer(64)
    st = ctypes.c_uint32()
    for ln in (0, 16 * KIB, 16 * KIB + 1, 64 * KIB, 64 * KIB + 1, 4 * MIB):
        N.check(N.lib.glfsx_debug_aux_log(1, None, 0, None))
        N.check(N.lib.glfsx_post(SALT, host, ln, h_ct, ref, None))
        row(("O", ONE_SMALL if ln <= 64 * KIB else ONE_MED, 1, ln), aux_take(N, buf, count))
        if ln > 64 * KIB:
            continue
        for salted in (0, 1):
            N.check(N.lib.glfsx_debug_aux_log(1, None, 0, None))
            rc = N.lib.glfsx_open(SALT if salted else None, None, ref, h_ct, ln, host,
                                  ctypes.byref(st))
            assert rc in (0, N.GLFSX_E_CORRUPT), rc      # the bytes are arbitrary
            row(("O", ONE_OPEN_SALTED if salted else ONE_OPEN_CLS, 1, ln),
                aux_take(N, buf, count))
    # two requests in one launch: a Writer's two full blocks (post_few); the
    # index node's own launch follows and is not recorded here
    sink = ctypes.cast(N.lib.glfsx_sink_count, N.POST_FN)
    for bs in (16 * KIB, 16 * KIB + 16, 64 * KIB, 64 * KIB + 16, 4 * MIB):
        data = ctypes.create_string_buffer(2 * bs)
        counts, root = (ctypes.c_uint64 * 2)(), N.glfsx_root()
        N.check(N.lib.glfsx_debug_aux_log(1, None, 0, None))
        N.check(N.lib.glfsx_create(bs, bs, None, None, data, 2 * bs, sink, ctypes.byref(counts),
                                   ctypes.byref(root)))
        log = [r for r in aux_take(N, buf, count) if r[0] in (ONE, MED, ONE_OPEN)]
        assert len(log) >= 2, log
        row(("O", ONE_SMALL if bs <= 64 * KIB else ONE_MED, 2, bs), log[:1])
    N.set_latency_wgs(old[0])
    N.set_open_route(old[1])
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d rows" % len(lines))


if __name__ == "__main__":
    if sys.argv[1] == "--aux":
        main_aux(sys.argv[2])
    else:
        main(sys.argv[1])
