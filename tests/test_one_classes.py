"""The layout of a batch of one-shot requests -- posts and verified reads in
their own descriptor ranges (glfs_amd/csrc/one_classes.h) -- as a stand-alone
program built with the host compiler under AddressSanitizer and UBSan
(tests/c/one_classes_test.cpp).  It runs as its own process: nothing is loaded
into Python and no GPU call is made."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_shot_batch_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler")
    name = "one_classes_test"
    out = str(tmp_path / name)
    subprocess.check_call(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "glfs_amd", "csrc"),
         os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", out])
    p = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert name + ": ok" in p.stdout
    assert p.stderr == "", p.stderr  # the sanitizers report nothing
