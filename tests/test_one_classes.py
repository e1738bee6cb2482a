"""The layout of a batch of one-shot requests -- posts and verified reads in
their own descriptor ranges (glfs_amd/csrc/one_classes.h) -- as a stand-alone
program built with the host compiler under AddressSanitizer and UBSan
(tests/c/one_classes_test.cpp, tests/cunit.py).  It runs as its own process:
nothing is loaded into Python and no GPU call is made."""
from cunit import build_and_run


def test_one_shot_batch_layout_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "one_classes_test")
