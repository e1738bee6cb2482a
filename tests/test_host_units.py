"""The units that need no GPU, as stand-alone programs built with the host
compiler under AddressSanitizer and UBSan: the host runtime's DevicePool and
job builders (glfs_amd/csrc/host.h, tests/c/host_units_test.cpp), and the
launch layer's per-stream scratch, launch plans and launch log
(stream_scratch.h, launch_plan.h, launch_log.h;
tests/c/stream_scratch_test.cpp, over a fake HIP runtime of its own).  Each runs as its own process: nothing is loaded into Python and no
GPU call is made."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # hipError_t, hipStream_t: the HIP headers
    out = str(tmp_path / name)
    subprocess.check_call(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         "-isystem", os.path.join(rocm, "include"),
         "-I", os.path.join(ROOT, "glfs_amd", "csrc"),
         os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", out])
    p = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert name + ": ok" in p.stdout
    assert p.stderr == "", p.stderr  # the sanitizers report nothing


def test_pool_and_job_builders_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "host_units_test")


def test_stream_scratch_and_launch_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "stream_scratch_test")
