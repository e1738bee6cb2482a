"""Rate of the ragged open (glfsx_open_ragged_device) on device-resident
batches of unequal-size blobs, beside the ragged post of the same bytes in the
same run and the only route the parent build has, one glfsx_open_batch_device
call per message.  Each repetition runs every build in its own process,
interleaved (the parent's library selected through GLFSX_LIB).

Batches: 4096 x 64 KiB dense, 1024 x 1 MiB, 1 GiB of log-uniform lengths in
[1 KiB, 2 MiB] at 64-B aligned offsets, and 1 M x 4 KiB (BASELINE config 4's
blob set).  Each batch is posted once with glfsx_post_ragged_device; then,
after a warm-up call of each shape, HIP events go around enough back-to-back
calls for a window of at least 0.5 s of
  open        the ragged open with a salt, plaintext to HBM
  check       the same, check only (no plaintext buffer)
  post        glfsx_post_ragged_device of the same bytes, ctext to HBM
and, in the parent's process,
  per_message glfsx_open_batch_device once per message, over a reduced count
              (PER_MESSAGE_SAMPLE messages picked with a fixed seed) -- its
              rate is the sample's bytes over the sample's time, i.e. scaled
              per blob, not a run over the whole batch.
Every status word of the opens must be 0.  GiB/s of message bytes.

usage: python scripts/open_ragged_rate.py [--reps 3] [--out profiles/open_ragged/rate.json]
                                          [--only NAME] PARENT_LIBPATH"""
import json
import math
import os
import random
import statistics
import subprocess
import sys

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
WINDOW_S = 0.5
PER_MESSAGE_SAMPLE = 2000


def batches():
    rng = random.Random(5)
    logu = []
    while sum(logu) < GIB:
        logu.append(int(math.exp(rng.uniform(math.log(KIB), math.log(2 * MIB)))))
    return [("64KiB_x4096", [64 * KIB] * 4096, 1), ("1MiB_x1024", [MIB] * 1024, 1),
            ("loguniform_1GiB", logu, 64), ("4KiB_x1M", [4 * KIB] * (1 << 20), 1)]


def worker(kind, only):
    import torch
    from glfs_amd import _native as N
    N.set_device(0)
    L = N.lib
    salt = bytes(range(32))
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    out = {}

    def window(call):
        """GiB/s-ready seconds per call: warm up, size the loop from one timed
        call, then events around the whole loop."""
        call()
        s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call()
        e1.record(s)
        e1.synchronize()
        k = max(2, int(math.ceil(1.2 * WINDOW_S / max(e0.elapsed_time(e1) / 1e3, 1e-6))))
        e0.record(s)
        for _ in range(k):
            call()
        e1.record(s)
        e1.synchronize()
        t = e0.elapsed_time(e1) / 1e3
        return t / k, k, t

    for name, lens, align in batches():
        if only and name != only:
            continue
        offs, o = [], 0
        for ln in lens:
            o = (o + align - 1) // align * align
            offs.append(o)
            o += ln
        total, n, nbytes = o + 64, len(lens), sum(lens)
        d = torch.empty(total, dtype=torch.uint8, device="cuda")
        ct = torch.empty(total, dtype=torch.uint8, device="cuda")
        pt = torch.empty(total, dtype=torch.uint8, device="cuda")
        N.check(L.glfsx_fill_splitmix_device(d.data_ptr(), 0, total // 8 * 8, 77, None))
        do = torch.tensor(offs, dtype=torch.int64, device="cuda")
        dl = torch.tensor(lens, dtype=torch.int64, device="cuda")
        refs = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def post():
            N.check(L.glfsx_post_ragged_device(salt, None, d.data_ptr(), do.data_ptr(),
                                               dl.data_ptr(), n, max(lens), ct.data_ptr(),
                                               refs.data_ptr(), sp))

        post()
        s.synchronize()
        row = {"blobs": n, "bytes": nbytes}
        if kind == "new":
            def open_(ptext):
                def f():
                    N.check(L.glfsx_open_ragged_device(salt, None, ct.data_ptr(), do.data_ptr(),
                                                       dl.data_ptr(), n, max(lens),
                                                       refs.data_ptr(), ptext, st.data_ptr(),
                                                       sp))
                return f

            for leg, call in (("open", open_(pt.data_ptr())), ("check", open_(None)),
                              ("post", post)):
                st.fill_(-1)
                per, k, t = window(call)
                row[leg] = {"gibps": nbytes / GIB / per, "calls": k, "window_s": t}
                if leg != "post":
                    assert int(st.abs().sum().item()) == 0, (name, leg, "nonzero status")
        else:
            pick = random.Random(6).sample(range(n), min(n, PER_MESSAGE_SAMPLE))
            cb, pb, rb, sb = ct.data_ptr(), pt.data_ptr(), refs.data_ptr(), st.data_ptr()

            def per_message():
                for i in pick:
                    ln = lens[i]
                    if L.glfsx_open_batch_device(salt, None, cb + offs[i], ln,
                                                 (ln + 63) // 64 * 64, rb + 64 * i,
                                                 pb + offs[i], sb + 4 * i, sp):
                        raise RuntimeError(N.last_error())

            per_message()
            s.synchronize()
            assert int(st[torch.tensor(pick, device="cuda")].abs().sum().item()) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            per_message()
            e1.record(s)
            e1.synchronize()
            t = e0.elapsed_time(e1) / 1e3
            sample = sum(lens[i] for i in pick)
            row["per_message"] = {"gibps": sample / GIB / t, "us_per_blob": t / len(pick) * 1e6,
                                  "sampled_blobs": len(pick), "sampled_bytes": sample,
                                  "window_s": t}
        out[name] = row
        del d, ct, pt
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    reps, path, only = 3, os.path.join("profiles", "open_ragged", "rate.json"), ""
    while args and args[0].startswith("--"):
        if args[0] == "--reps":
            reps = int(args[1])
        elif args[0] == "--out":
            path = args[1]
        elif args[0] == "--only":
            only = args[1]
        else:
            sys.exit(__doc__)
        args = args[2:]
    if len(args) != 1:
        sys.exit(__doc__)
    parent = os.path.abspath(args[0])
    runs = {"new": [], "parent": []}
    for r in range(reps):
        for kind in ("new", "parent"):
            env = dict(os.environ)
            if kind == "parent":
                env["GLFSX_LIB"] = parent
            else:
                env.pop("GLFSX_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, only],
                               env=env, capture_output=True, text=True, timeout=400)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode or not lines:
                print(kind, "failed", p.returncode, p.stderr[-2000:], flush=True)
                sys.exit(1)
            runs[kind].append(json.loads(lines[0]))
            print(r, kind, {b: {k: round(v["gibps"], 2) for k, v in row.items()
                                if isinstance(v, dict)}
                            for b, row in runs[kind][-1].items()}, flush=True)
    table = {}
    for b in runs["new"][0]:
        row = {}
        for kind, legs in (("new", ("open", "check", "post")), ("parent", ("per_message",))):
            for leg in legs:
                g = [x[b][leg]["gibps"] for x in runs[kind]]
                row[leg] = {"gibps": g, "median": statistics.median(g),
                            "spread": max(g) - min(g)}
        row["per_message"]["us_per_blob"] = statistics.median(
            x[b]["per_message"]["us_per_blob"] for x in runs["parent"])
        spread = max(row[leg]["spread"] for leg in ("open", "check", "post"))
        row["run_spread"] = spread
        # the yardstick: the open's median no lower than the same run's post, less the spread
        row["open_meets_post"] = row["open"]["median"] >= row["post"]["median"] - spread
        row["check_meets_post"] = row["check"]["median"] >= row["post"]["median"] - spread
        table[b] = row
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"reps": reps, "window_s": WINDOW_S, "per_message_sample": PER_MESSAGE_SAMPLE,
                   "table": table, "runs": runs}, f, indent=1)
    for b, row in table.items():
        print(b, " ".join(f"{leg} {row[leg]['median']:.1f} (+-{row[leg]['spread']:.1f})"
                          for leg in ("open", "check", "post", "per_message")),
              f"{row['per_message']['us_per_blob']:.1f} us/blob per message,",
              "open >= post" if row["open_meets_post"] else "OPEN BELOW POST", flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:2] == ["--worker"]:
        worker(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "")
    else:
        main()
