"""The grouping of glfsx_open_blobs (glfs_amd/csrc/ragged_groups.h: message
lengths -> groups of whole consecutive messages of at most 64 MiB and their
16-B aligned staging offsets) as a stand-alone program built with the host
compiler under AddressSanitizer and UBSan (tests/c/ragged_groups_test.cpp),
exactly as tests/test_host_units.py builds its two.  Nothing is loaded into
Python and no GPU call is made."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    out = str(tmp_path / name)
    subprocess.check_call(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
         "-isystem", os.path.join(rocm, "include"),
         "-I", os.path.join(ROOT, "glfs_amd", "csrc"),
         os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", out])
    p = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert name + ": ok" in p.stdout
    assert p.stderr == "", p.stderr  # the sanitizers report nothing


def test_ragged_groups_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "ragged_groups_test")
