"""Rate of the verified read (glfsx_open_batch_device) on device-resident
data: 16 GiB of splitmix plaintext at 1 MiB blocks, posted once with
glfsx_post_batch_device, then -- after a warm-up -- REPS repetitions,
interleaved in one process and timed with HIP events, of
  (a) open, route 2 (k_open)           (b) open, route 1 (composed)
  (c) glfsx_decrypt_batch_device alone (d) glfsx_post_batch_device, same bytes
and a sweep of (a) against (b) at 256 .. 16384 blocks of 1 MiB, at 512 ..
2048 blocks of 2 MiB and at 1 GiB of 256 KiB and of 64 KiB blocks.  Every
status word must be 0 and the plaintext of the timed runs equal to the input.
Prints one JSON line (medians and spreads, GiB/s of plaintext) and writes it
to --out.

usage: python scripts/open_rate.py [--gib 16] [--reps 5] [--out profiles/open/open_rate.json]"""
import argparse
import json
import os
import statistics
import sys

MIB, GIB = 1 << 20, 1 << 30
KIB = 1 << 10
SWEEP = [(MIB, k) for k in (256, 512, 1024, 2048, 4096, 16384)] + \
        [(2 * MIB, 512), (2 * MIB, 1024), (2 * MIB, 2048), (256 * KIB, 4096), (64 * KIB, 16384)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "open", "open_rate.json"))
    args = ap.parse_args()
    import torch
    from glfs_amd import _native as N
    if not torch.cuda.is_available() or N.device_count() < 1:
        sys.exit("open_rate.py needs a GPU")
    N.set_device(0)
    L = N.lib
    salt = bytes(range(32))
    total, bs = args.gib * GIB, MIB
    n = total // bs
    s = torch.cuda.Stream()
    sp = s.cuda_stream

    def buf(nbytes, dtype=torch.uint8):
        return torch.empty(nbytes, dtype=dtype, device="cuda")

    src, ct, pt = buf(total), buf(total), buf(total)
    refs, st = buf(64 * n), buf(n, torch.int32)
    N.check(L.glfsx_fill_splitmix_device(src.data_ptr(), 0, total, 2026, sp))
    N.check(L.glfsx_post_batch_device(salt, src.data_ptr(), total, bs, ct.data_ptr(),
                                      refs.data_ptr(), None, sp))
    # the sweep's other block sizes: the head of the input posted again
    ct2 = buf(max(b * k for b, k in SWEEP if b != bs))
    refs2 = buf(64 * max(k for b, k in SWEEP if b != bs))
    s.synchronize()

    def do_open(route, ctext, nbytes, block, rf):
        def f():
            N.set_open_route(route)
            N.check(L.glfsx_open_batch_device(salt, None, ctext.data_ptr(), nbytes, block,
                                              rf.data_ptr(), pt.data_ptr(), st.data_ptr(), sp))
        return f

    def do_decrypt():
        N.check(L.glfsx_decrypt_batch_device(ct.data_ptr(), total, bs, refs.data_ptr(),
                                             pt.data_ptr(), sp))

    def do_post():
        N.check(L.glfsx_post_batch_device(salt, src.data_ptr(), total, bs, ct.data_ptr(),
                                          refs.data_ptr(), None, sp))

    def checked(nbytes, blocks):
        """After an open: all status words 0, plaintext = input."""
        s.synchronize()
        if int(st[:blocks].count_nonzero()):
            sys.exit(f"non-zero status words over {blocks} blocks")
        if not torch.equal(pt[:nbytes], src[:nbytes]):
            sys.exit(f"plaintext differs from the input over {nbytes} bytes")

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        f()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run(items, reps):
        """items: {name: (f, bytes, check or None)}; reps interleaved rounds."""
        ms = {k: [] for k in items}
        for rep in range(reps + 1):              # round 0 warms up
            for k, (f, _, check) in items.items():
                st.fill_(-1)
                pt[:4096].zero_()
                torch.cuda.current_stream().synchronize()
                t = timed(f)
                if check:
                    check()
                if rep:
                    ms[k].append(t)
        out = {}
        for k, (_, nbytes, _) in items.items():
            g = [nbytes / GIB / (t / 1e3) for t in ms[k]]
            out[k] = {"gibps_median": round(statistics.median(g), 2),
                      "gibps_min": round(min(g), 2), "gibps_max": round(max(g), 2),
                      "ms": [round(t, 4) for t in ms[k]]}
        return out

    try:
        head = run({
            "open_fused": (do_open(2, ct, total, bs, refs), total, lambda: checked(total, n)),
            "open_composed": (do_open(1, ct, total, bs, refs), total, lambda: checked(total, n)),
            "decrypt": (do_decrypt, total, None),
            "post": (do_post, total, None),
        }, args.reps)
        sweep = {}
        for b, k in SWEEP:
            nb = b * k
            if nb > total:
                continue
            c, r = (ct, refs) if b == bs else (ct2, refs2)
            if b != bs:
                N.check(L.glfsx_post_batch_device(salt, src.data_ptr(), nb, b, c.data_ptr(),
                                                  r.data_ptr(), None, sp))
                s.synchronize()
            sweep[f"{b // KIB}KiB_x{k}"] = run({
                "fused": (do_open(2, c, nb, b, r), nb, lambda nb=nb, k=k: checked(nb, k)),
                "composed": (do_open(1, c, nb, b, r), nb, lambda nb=nb, k=k: checked(nb, k)),
            }, args.reps)
    finally:
        N.set_open_route(0)
    res = {"device": torch.cuda.get_device_name(0), "bytes": total, "block_size": bs,
           "reps": args.reps, "unit": "GiB/s of plaintext", "headline": head, "sweep": sweep}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
