"""Rate of the tree decoder against the encoder over config 4's tree: 2^20
entries ("%07d" names, type "blob", 4 KiB sizes, random roots), about 241 MB
of lines.

Device leg (default): the entries are encoded in HBM once
(glfsx_tree_encode_device), then -- after a warm-up -- REPS repetitions,
alternating in one process and timed with HIP events on one stream, of
  (a) glfsx_tree_decode_device over the lines, every column taken
  (b) glfsx_tree_encode_device over the same entries (the yardstick).
Both calls end in their one synchronisation, so the events bracket whole
calls.  The decoded columns must equal the entries.  The clock the chip
holds is bench.py's held_clock_GHz from the same session on the same box.
The per-kernel split comes from the same script under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python
scripts/tree_decode_rate.py --reps 3`, in a run of its own.

Host leg (--host, no GPU): decode_lines, read_tree_bytes and
read_tree_bytes_py over the same lines, wall time, best of --reps.

Prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_lines(n):
    import numpy as np
    from glfs_amd import _native as N
    names = np.frombuffer(b"".join(b"%07d" % i for i in range(n)), dtype=np.uint8)
    no = np.arange(n + 1, dtype=np.uint64) * 7
    types = np.frombuffer(b"blob" * n, dtype=np.uint8)
    to = np.arange(n + 1, dtype=np.uint64) * 4
    modes = np.full(n, 0o644, dtype=np.uint32)
    roots = np.random.default_rng(4).integers(0, 256, 64 * n, dtype=np.uint8)
    sizes = np.full(n, 4096, dtype=np.uint64)
    bss = np.full(n, 2 << 20, dtype=np.uint64)
    total = ctypes.c_uint64()
    p = lambda a: a.ctypes.data
    args = (n, p(names), p(no), p(modes), p(types), p(to), p(roots), p(sizes), p(bss))
    N.check(N.lib.glfsx_tree_encode(*args, None, 0, ctypes.byref(total), None))
    out = np.empty(total.value, dtype=np.uint8)
    N.check(N.lib.glfsx_tree_encode(*args, p(out), total.value, ctypes.byref(total), None))
    return out.tobytes()


def host_leg(n, reps):
    from glfs_amd import tree as T
    data = host_lines(n)

    def best(f, k):
        ts = []
        for _ in range(k):
            t0 = time.perf_counter()
            r = f()
            ts.append(time.perf_counter() - t0)
        return min(ts), r

    t_dec, c = best(lambda: T.decode_lines(data), reps)
    assert c.n == n and c.n_bad == 0
    t_ent, _ = best(lambda: T.entries_from_columns(c), 1)
    t_nat, ents = best(lambda: T.read_tree_bytes(data), 1)
    t_py, want = best(lambda: T.read_tree_bytes_py(data), 1)
    assert ents == want
    return {"what": "host leg: wall seconds over n config-4 lines", "n": n, "bytes": len(data),
            "decode_lines_s": round(t_dec, 4), "read_tree_bytes_s": round(t_nat, 3),
            "read_tree_bytes_py_s": round(t_py, 3),
            "entries_from_columns_s": round(t_ent, 3),
            "python_objects_share_of_native": round(t_ent / t_nat, 3),
            "cpus": os.cpu_count()}


def device_leg(n, reps):
    import numpy as np
    import torch
    from glfs_amd import _native as N
    if not torch.cuda.is_available() or N.device_count() < 1:
        sys.exit("tree_decode_rate.py needs a GPU (or --host)")
    N.set_device(0)
    L = N.lib
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    dev = lambda a: torch.from_numpy(a).cuda()
    names = dev(np.frombuffer(b"".join(b"%07d" % i for i in range(n)), dtype=np.uint8).copy())
    no = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 7
    types = dev(np.frombuffer(b"blob" * n, dtype=np.uint8).copy())
    to = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 4
    modes = torch.full((n,), 0o644, dtype=torch.int32, device="cuda")
    roots = torch.randint(0, 256, (64 * n,), dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), 4096, dtype=torch.int64, device="cuda")
    bss = torch.full((n,), 2 << 20, dtype=torch.int64, device="cuda")
    cap = 260 * n
    lines = torch.empty(cap, dtype=torch.uint8, device="cuda")
    total = ctypes.c_uint64()

    def encode():
        N.check(L.glfsx_tree_encode_device(n, names.data_ptr(), no.data_ptr(), modes.data_ptr(),
                                           types.data_ptr(), to.data_ptr(), roots.data_ptr(),
                                           sizes.data_ptr(), bss.data_ptr(), lines.data_ptr(), cap,
                                           None, ctypes.byref(total), sp))

    torch.cuda.synchronize()
    encode()
    length = total.value
    e = lambda k, dt: torch.empty(k, dtype=dt, device="cuda")
    o = dict(names=e(7 * n, torch.uint8), no=e(n + 1, torch.int64), modes=e(n, torch.int32),
             types=e(4 * n, torch.uint8), to=e(n + 1, torch.int64), roots=e(64 * n, torch.uint8),
             sizes=e(n, torch.int64), bss=e(n, torch.int64), status=e(n, torch.int32))
    counts = (ctypes.c_uint64 * 5)()

    def decode():
        N.check(L.glfsx_tree_decode_device(lines.data_ptr(), length, o["names"].data_ptr(), 7 * n,
                                           o["no"].data_ptr(), o["modes"].data_ptr(),
                                           o["types"].data_ptr(), 4 * n, o["to"].data_ptr(),
                                           o["roots"].data_ptr(), o["sizes"].data_ptr(),
                                           o["bss"].data_ptr(), o["status"].data_ptr(), n, counts,
                                           sp))

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        f()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(2):  # warm-up: code objects, scratch
        decode()
        encode()
    dec, enc = [], []
    for _ in range(reps):
        dec.append(timed(decode))
        enc.append(timed(encode))
    torch.cuda.synchronize()
    assert list(counts) == [n, 7 * n, 4 * n, 0, 0], list(counts)
    for k, w in (("names", names), ("no", no), ("modes", modes), ("types", types), ("to", to),
                 ("roots", roots), ("sizes", sizes), ("bss", bss)):
        assert torch.equal(o[k], w), k
    assert not bool(o["status"].any())
    med = statistics.median
    d, c = med(dec), med(enc)
    return {"what": "device leg: ms per whole call (HIP events), median of reps", "n": n,
            "line_bytes": length, "reps": reps,
            "decode_ms": round(d, 3), "decode_ms_min_max": [round(min(dec), 3), round(max(dec), 3)],
            "encode_ms": round(c, 3), "encode_ms_min_max": [round(min(enc), 3), round(max(enc), 3)],
            "decode_over_encode": round(d / c, 2),
            "decode_GBps_of_lines": round(length / d / 1e6, 1),
            "encode_GBps_of_lines": round(length / c / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host", action="store_true", help="the host leg (no GPU needed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = host_leg(args.n, min(args.reps, 3)) if args.host else device_leg(args.n, args.reps)
    out = args.out or os.path.join("profiles", "tree_decode",
                                   "host_rate.json" if args.host else "device_rate.json")
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
