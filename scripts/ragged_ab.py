"""glfsx_post_blobs_device on batches of unequal-size blobs, A/B between
builds of the library, interleaved: each build runs in its own process
(selected through GLFSX_LIB), REPS times in turn, device-resident data, ctext
to HBM, bs = 2 MiB, timed with HIP events around the whole call (its host
waits included).  Batches: 4096 x 64 KiB dense, 1024 x 1 MiB, 1 GiB of
log-uniform lengths in [1 KiB, 2 MiB] at 64-B aligned offsets, and the
control 65536 x 4 KiB (the small route, which the ragged post must not move).

usage: python scripts/ragged_ab.py [--reps 3] [--out profiles/ragged/ab.json]
                                   NAME=LIBPATH NAME=LIBPATH ...
(the first build named is the one under test, the second its parent)."""
import hashlib
import json
import math
import os
import random
import statistics
import subprocess
import sys

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
BS = 2 * MIB


def batches():
    rng = random.Random(5)
    logu = []
    while sum(logu) < GIB:
        logu.append(int(math.exp(rng.uniform(math.log(KIB), math.log(2 * MIB)))))
    return [("64KiB_x4096", [64 * KIB] * 4096, 1), ("1MiB_x1024", [MIB] * 1024, 1),
            ("loguniform_1GiB", logu, 64), ("control_4KiB_x65536", [4 * KIB] * 65536, 1)]


def worker():
    import torch
    from glfs_amd import _native as N
    N.set_device(0)
    salt = bytes(range(32))
    s = torch.cuda.Stream()
    out = {}
    for name, lens, align in batches():
        offs, o = [], 0
        for ln in lens:
            o = (o + align - 1) // align * align
            offs.append(o)
            o += ln
        total = o + 64
        d = torch.empty(total, dtype=torch.uint8, device="cuda")
        ct = torch.empty(total, dtype=torch.uint8, device="cuda")
        N.check(N.lib.glfsx_fill_splitmix_device(d.data_ptr(), 0, total // 8 * 8, 77, None))
        do = torch.tensor(offs, dtype=torch.int64, device="cuda")
        dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
        roots = torch.zeros(64 * len(lens), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ms = []
        for it in range(4):  # the first call warms up (scratch, code objects)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            N.check(N.lib.glfsx_post_blobs_device(BS, salt, None, d.data_ptr(), do.data_ptr(),
                                                  dl.data_ptr(), len(lens), max(lens),
                                                  ct.data_ptr(), roots.data_ptr(), s.cuda_stream))
            e1.record(s)
            e1.synchronize()
            if it:
                ms.append(e0.elapsed_time(e1))
        t = statistics.median(ms)
        out[name] = {"blobs": len(lens), "bytes": sum(lens), "ms": ms,
                     "gibps": sum(lens) / GIB / (t / 1e3),
                     "roots_sha256": hashlib.sha256(roots.cpu().numpy().tobytes()).hexdigest()}
        del d, ct
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    reps, path = 3, os.path.join("profiles", "ragged", "ab.json")
    while args and args[0].startswith("--"):
        if args[0] == "--reps":
            reps = int(args[1])
        elif args[0] == "--out":
            path = args[1]
        else:
            sys.exit(__doc__)
        args = args[2:]
    libs = [a.split("=", 1) for a in args]
    if len(libs) < 2:
        sys.exit(__doc__)
    runs = {name: [] for name, _ in libs}
    for r in range(reps):
        for name, lib in libs:
            env = dict(os.environ, GLFSX_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env,
                               capture_output=True, text=True, timeout=280)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode or not lines:
                print(name, "failed", p.returncode, p.stderr[-2000:], flush=True)
                sys.exit(1)
            runs[name].append(json.loads(lines[0]))
            print(r, name, {b: round(v["gibps"], 2) for b, v in runs[name][-1].items()},
                  flush=True)
    names = [n for n, _ in libs]
    table = {}
    for b in runs[names[0]][0]:
        row = {}
        for n in names:
            g = [x[b]["gibps"] for x in runs[n]]
            row[n] = {"gibps": g, "median": statistics.median(g), "spread": max(g) - min(g)}
        ctrl = {n: statistics.median([x["control_4KiB_x65536"]["gibps"] for x in runs[n]])
                for n in names}
        for n in names:
            row[n]["of_control"] = row[n]["median"] / ctrl[n]
        new, old = row[names[0]], row[names[1]]
        spread = max(new["spread"], old["spread"])
        row["new_minus_parent"] = new["median"] - old["median"]
        row["rep_spread"] = spread
        row["same_roots"] = len({x[b]["roots_sha256"] for n in names for x in runs[n]}) == 1
        table[b] = row
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"reps": reps, "builds": names, "block_size": BS, "table": table,
                   "runs": runs}, f, indent=1)
    for b, row in table.items():
        print(b, " ".join(f"{n} {row[n]['median']:.1f} (+-{row[n]['spread']:.1f}, "
                          f"{row[n]['of_control']:.2f} of control)" for n in names),
              "same roots" if row["same_roots"] else "ROOTS DIFFER", flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["--worker"]:
        worker()
    else:
        main()
