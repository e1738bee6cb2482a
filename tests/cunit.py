"""Build one stand-alone C++ test program (tests/c/<name>.cpp, its own main)
with the host compiler under AddressSanitizer and UBSan and run it as its own
process: nothing is loaded into Python and no GPU call is made.  A helper
module of the CPU tests (test_host_units, test_ragged_groups,
test_one_classes, test_tree_decode, test_writer_book), not a conftest."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build_and_run(tmp_path, name, sources=(), args=(), timeout=120):
    """tests/c/<name>.cpp plus `sources` (paths from the repository root; a
    .c file is compiled as C) into tmp_path/<name>, run with `args`.  Asserts
    exit status 0, the line "<name>: ok" and an empty stderr (the sanitizers
    report nothing); returns the program's stdout."""
    cxx = shutil.which("g++") or shutil.which("c++")
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cxx or not cc:
        pytest.fail("no host C/C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # hipError_t, hipStream_t: the HIP headers
    inc = ["-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"),
           "-I", os.path.join(ROOT, "glfs_amd", "csrc"), "-I", ROOT]
    objs = []
    for src in sources:
        if src.endswith(".c"):
            objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
            subprocess.check_call([cc, *SAN, "-c", os.path.join(ROOT, src),
                                   "-o", objs[-1]])
        else:
            objs.append(os.path.join(ROOT, src))
    out = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", *SAN, "-pthread", *inc,
                           os.path.join(ROOT, "tests", "c", name + ".cpp"), *objs, "-o", out])
    p = subprocess.run([out, *args], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert name + ": ok" in p.stdout
    assert p.stderr == "", p.stderr  # the sanitizers report nothing
    return p.stdout
