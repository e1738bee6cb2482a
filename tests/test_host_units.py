"""The host runtime's HIP-free units -- DevicePool and the job builders of
glfs_amd/csrc/host.h -- as a stand-alone program (tests/c/host_units_test.cpp)
built with the host compiler under AddressSanitizer and UBSan.  It runs as
its own process: nothing is loaded into Python and no GPU call is made."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_and_job_builders_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # host.h's types come with the HIP headers
    out = str(tmp_path / "host_units_test")
    subprocess.check_call(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         "-isystem", os.path.join(rocm, "include"),
         "-I", os.path.join(ROOT, "glfs_amd", "csrc"),
         os.path.join(ROOT, "tests", "c", "host_units_test.cpp"), "-o", out])
    p = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "host_units_test: ok" in p.stdout
    assert p.stderr == "", p.stderr  # the sanitizers report nothing
