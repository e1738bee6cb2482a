"""Rates of the tree-against-tree primitives and of Machine.compare's two
routes.

Primitives leg: two sides of --n entries ("%07d" names, half of them on both
sides, type "blob").  After a warm-up, REPS repetitions, alternating in one
process and timed with HIP events on one stream, of
  (a) glfsx_tree_join_device, all three outputs
  (b) one glfsx_tree_select_device of n entries (A's unmatched entries and
      B's matched ones), every column taken
against the host join (glfsx_tree_join on the job's cores, wall time) and a
Python dict join of the same names (wall time).  The device outputs must
equal the host's.

Compare leg: Machine.compare of two flat trees of 2^e entries each (half of
the names shared, half of those with equal refs) for e in --exps, on the
entry route and on the column route (COMPARE_DEVICE_MIN set above and below
every size), wall time, best of the repetitions; both routes must return the
same refs.  The crossover -- the smallest size from which the column route is
never slower -- is reported as entries of both trees together, the unit of
COMPARE_DEVICE_MIN.

The per-kernel split comes from the same script under `rocprofv3
--kernel-trace --stats --output-format csv -d <dir> -- python
scripts/tree_join_rate.py --reps 3 --exps ""`, in a run of its own.

Prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def side_columns(np, ids, roots_seed):
    n = len(ids)
    return dict(
        n=n, names=np.frombuffer(b"".join(b"%07d" % i for i in ids), dtype=np.uint8).copy(),
        name_offs=np.arange(n + 1, dtype=np.uint64) * 7, modes=np.full(n, 0o644, dtype=np.uint32),
        types=np.frombuffer(b"blob" * n, dtype=np.uint8).copy(),
        type_offs=np.arange(n + 1, dtype=np.uint64) * 4,
        roots=np.random.default_rng(roots_seed).integers(0, 256, 64 * n, dtype=np.uint8),
        sizes=np.full(n, 4096, dtype=np.uint64), block_sizes=np.full(n, 2 << 20, dtype=np.uint64),
        status=np.zeros(n, dtype=np.uint32))


COLS = ("names", "name_offs", "modes", "types", "type_offs", "roots", "sizes", "block_sizes",
        "status")


def primitives_leg(n, reps):
    import numpy as np
    import torch
    from glfs_amd import _native as N
    L = N.lib
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    ha = side_columns(np, range(n), 4)
    hb = side_columns(np, range(n // 2, n // 2 + n), 5)
    hb["roots"][:64 * (n // 4)] = ha["roots"][64 * (n // 2):64 * (n // 2 + n // 4)]  # equal refs
    struct = lambda c, ptr: N.glfsx_tree_cols(n, *[ptr(c[k]) for k in COLS])
    # host join and dict join
    sa, sb = struct(ha, lambda a: a.ctypes.data), struct(hb, lambda a: a.ctypes.data)
    am, bm, ac = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.uint8)
    host = []
    for _ in range(max(3, reps // 2)):
        t0 = time.perf_counter()
        N.check(L.glfsx_tree_join(ctypes.byref(sa), ctypes.byref(sb), am.ctypes.data,
                                  bm.ctypes.data, ac.ctypes.data))
        host.append(time.perf_counter() - t0)
    na_list = [bytes(x) for x in ha["names"].reshape(n, 7)]
    nb_list = [bytes(x) for x in hb["names"].reshape(n, 7)]
    t0 = time.perf_counter()
    ib = {k: j for j, k in enumerate(nb_list)}
    ia = {k: i for i, k in enumerate(na_list)}
    pam = [ib.get(k, -1) for k in na_list]
    pbm = [ia.get(k, -1) for k in nb_list]
    t_dict = time.perf_counter() - t0
    assert pam == am.tolist() and pbm == bm.tolist()
    # device
    da = {k: torch.from_numpy(ha[k].view(np.uint8)).cuda() for k in COLS}
    db = {k: torch.from_numpy(hb[k].view(np.uint8)).cuda() for k in COLS}
    xa, xb = struct(da, lambda t: t.data_ptr()), struct(db, lambda t: t.data_ptr())
    e = lambda k, dt: torch.empty(k, dtype=dt, device="cuda")
    d_am, d_bm, d_ac = e(n, torch.int64), e(n, torch.int64), e(n, torch.uint8)

    def join():
        N.check(L.glfsx_tree_join_device(ctypes.byref(xa), ctypes.byref(xb), d_am.data_ptr(),
                                         d_bm.data_ptr(), d_ac.data_ptr(), sp))

    torch.cuda.synchronize()
    join()
    torch.cuda.synchronize()
    assert np.array_equal(d_am.cpu().numpy(), am) and np.array_equal(d_bm.cpu().numpy(), bm)
    assert np.array_equal(d_ac.cpu().numpy(), ac)
    sel = torch.where(d_am < 0, torch.arange(n, device="cuda"), -1 - d_am).contiguous()
    o = dict(names=e(7 * n, torch.uint8), no=e(n + 1, torch.int64), modes=e(n, torch.int32),
             types=e(4 * n, torch.uint8), to=e(n + 1, torch.int64), roots=e(64 * n, torch.uint8),
             sizes=e(n, torch.int64), bss=e(n, torch.int64), status=e(n, torch.int32))
    counts = (ctypes.c_uint64 * 2)()

    def select():
        N.check(L.glfsx_tree_select_device(
            ctypes.byref(xa), ctypes.byref(xb), sel.data_ptr(), n, o["names"].data_ptr(), 7 * n,
            o["no"].data_ptr(), o["modes"].data_ptr(), o["types"].data_ptr(), 4 * n,
            o["to"].data_ptr(), o["roots"].data_ptr(), o["sizes"].data_ptr(), o["bss"].data_ptr(),
            o["status"].data_ptr(), n, counts, sp))

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        f()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b)

    torch.cuda.synchronize()
    for _ in range(2):  # warm-up: code objects, scratch
        join()
        select()
    tj, ts = [], []
    for _ in range(reps):
        tj.append(timed(join))
        ts.append(timed(select))
    torch.cuda.synchronize()
    assert list(counts) == [7 * n, 4 * n]
    idx = np.where(am < 0, np.arange(n), n + am)
    want_roots = np.concatenate([ha["roots"], hb["roots"]]).reshape(-1, 64)[idx].reshape(-1)
    assert np.array_equal(o["roots"].cpu().numpy(), want_roots)
    want_names = np.concatenate([ha["names"], hb["names"]]).reshape(-1, 7)[idx].reshape(-1)
    assert np.array_equal(o["names"].cpu().numpy(), want_names)
    med = statistics.median
    return {"what": "ms per call, median of reps (device: HIP events; host: wall)", "n_a": n,
            "n_b": n, "matching": n // 2, "reps": reps,
            "join_device_ms": round(med(tj), 3),
            "join_device_ms_min_max": [round(min(tj), 3), round(max(tj), 3)],
            "select_device_ms": round(med(ts), 3),
            "select_device_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
            "join_host_ms": round(1e3 * med(host), 2),
            "join_host_ms_min_max": [round(1e3 * min(host), 2), round(1e3 * max(host), 2)],
            "join_python_dict_ms": round(1e3 * t_dict, 1), "host_threads": min(16, os.cpu_count())}


def compare_leg(exps, reps):
    from glfs_amd import bigblob, glfs, tree as T
    m = glfs.Machine()
    src = bigblob.MemStore(m.block_size)
    r0, r1, r2 = m.post_blobs(src, [b"zero", b"one", b"two"])
    rows = []
    for e in exps:
        n = 1 << e
        x = [T.TreeEntry("%07d" % i, 0o644, r0) for i in range(n)]
        y = [T.TreeEntry("%07d" % i, 0o600, r0 if i < n // 2 + n // 4 else r1)
             for i in range(n // 2, n // 2 + n)]
        left, right = m.post_tree(src, x), m.post_tree(src, y)
        del x, y
        k = reps if e <= 14 else 1
        out = {}
        for _ in range(k):
            for route, dmin in (("entry", 1 << 62), ("column", 0)):   # alternating
                dst = bigblob.MemStore(m.block_size)
                dst.blobs = dict(src.blobs)
                glfs.Machine.COMPARE_DEVICE_MIN = dmin
                t0 = time.perf_counter()
                d = m.compare(dst, src, left, right)
                dt = time.perf_counter() - t0
                out.setdefault(route, []).append(dt)
                out.setdefault("refs", set()).add((d.left, d.right, d.both))
        assert len(out["refs"]) == 1, "the routes disagree"
        rows.append({"entries_each": n, "entries_both": 2 * n,
                     "entry_route_ms": round(1e3 * min(out["entry"]), 3),
                     "column_route_ms": round(1e3 * min(out["column"]), 3),
                     "reps": k})
        print(json.dumps(rows[-1]), flush=True)
    cross = None
    for i, r in enumerate(rows):
        if all(q["column_route_ms"] <= q["entry_route_ms"] for q in rows[i:]):
            cross = r["entries_both"]
            break
    return {"what": "Machine.compare of two flat trees, wall ms, best of reps", "sweep": rows,
            "crossover_entries_both": cross}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--exps", default="6,7,8,9,10,11,12,13,14,16,18,20",
                    help="the compare leg's sizes as exponents of 2 (empty: skip the leg)")
    ap.add_argument("--out", default=os.path.join("profiles", "join", "join_rate.json"))
    args = ap.parse_args()
    import torch
    from glfs_amd import _native as N
    if not torch.cuda.is_available() or N.device_count() < 1:
        sys.exit("tree_join_rate.py needs a GPU")
    N.set_device(0)
    res = {"primitives": primitives_leg(args.n, args.reps)}
    exps = [int(x) for x in args.exps.split(",") if x]
    if exps:
        res["compare"] = compare_leg(exps, args.reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
