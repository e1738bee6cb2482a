#!/usr/bin/env python3
"""Per-call latency of the one-block verified read (glfsx_open) beside what a
caller had before it, and k_one_open's own time beside k_one's.

Runs tools/openbench (built here with the host C compiler if missing): one
process, one thread, a warm-up, then --reps interleaved repetitions of
--calls calls of every variant at every size:
  (a) open    glfsx_open, route 0
  (b) batch1  glfsx_open_batch with one block of the same bytes
  (c) xor     glfsx_chacha20_xor, the unchecked get_f
  (d) post    glfsx_post of the same plaintext (k_one)
  and staged  glfsx_open under route 1 (device staging at every size)
Then, unless --no-trace, the same program once more at 4 KiB under
`rocprofv3 --kernel-trace --stats` (tracing only, no counters) for the
kernels' own durations.  Writes profiles/open/one_open.json (or --out).

The route rule the table feeds: auto takes the one-shot kernel at a size only
if (a) is at or below (b) there in the same run; the file's "route_rule"
lists the verdict per size."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "glfs_amd", "libglfsx.so")
BENCH = os.path.join(ROOT, "tools", "openbench")
SIZES = [0, 1024, 4096, 16384, 65536, 1 << 20, 2 << 20]
ONE_SHOT_MAX = 64 * 1024


def build():
    src = BENCH + ".c"
    if os.path.exists(BENCH) and os.path.getmtime(BENCH) >= os.path.getmtime(src):
        return
    subprocess.check_call(["gcc", "-O2", "-o", BENCH, src, "-I" + os.path.join(ROOT, "include"),
                           "-ldl"])


def run(args, prefix=()):
    p = subprocess.run(list(prefix) + [BENCH, LIB] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=900)
    if p.returncode:
        sys.exit(f"openbench failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    start = p.stdout.index('{"reps"')
    return json.loads(p.stdout[start:p.stdout.rindex("}") + 1])


def kernel_stats(reps, calls):
    """Durations of the one-shot kernels at 4 KiB from one traced run."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"skipped": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as d:
        run([reps, calls, 4096],
            prefix=[prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "k_one" not in name:
            continue
        short = name[name.index("k_one"):].split("(")[0]
        out[short] = {k: (float(r[k]) if k != "Calls" else int(r[k]))
                      for k in ("Calls", "AverageNs", "MinNs", "MaxNs", "StdDev", "Percentage")
                      if r.get(k) not in (None, "")}
    return out or {"skipped": "no k_one rows in the kernel stats"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open", "one_open.json"))
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.reps < 3:
        sys.exit("at least 3 interleaved repetitions")
    build()
    res = run([a.reps, a.calls] + SIZES)
    table = {}
    for r in res["results"]:
        table.setdefault(str(r["size"]), {})[r["variant"]] = {"p50_us": r["p50_us"],
                                                              "p90_us": r["p90_us"]}
    if "0" in table:
        table["0"]["batch1"] = None     # total == 0 is a no-op in glfsx_open_batch
    rule = {}
    for size, row in table.items():
        if int(size) > ONE_SHOT_MAX:
            continue
        b = row.get("batch1")
        rule[size] = {"one_shot_wins": b is None or row["open"]["p50_us"] <= b["p50_us"],
                      "open_p50_us": row["open"]["p50_us"],
                      "batch1_p50_us": b and b["p50_us"]}
    doc = {
        "what": "per-call latency, one thread, microseconds; reps interleaved in one process "
                "after a warm-up; every timed open returned status 0 and the right plaintext",
        "reps": res["reps"], "calls_per_rep": res["calls"],
        "variants": {"open": "glfsx_open route 0", "staged": "glfsx_open route 1",
                     "batch1": "glfsx_open_batch, one block", "xor": "glfsx_chacha20_xor",
                     "post": "glfsx_post"},
        "latency": table,
        "route_rule": rule,
        "kernel_ns_at_4096": {"skipped": "--no-trace"} if a.no_trace
        else kernel_stats(3, 200),
        "not_measured": ["concurrent callers' calls/s", "more than one GPU",
                         "a k_med-style one-shot open between 64 KiB and 4 MiB"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"out": a.out, "route_rule": rule,
                      "kernel_ns_at_4096": doc["kernel_ns_at_4096"]}))


if __name__ == "__main__":
    main()
