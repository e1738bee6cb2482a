"""The grouping of glfsx_open_blobs (glfs_amd/csrc/ragged_groups.h: message
lengths -> groups of whole consecutive messages of at most 64 MiB and their
16-B aligned staging offsets) and the run copier beside it (the copies between
a batch of messages and its staging, one per run contiguous on both sides) as
a stand-alone program built with the host compiler under AddressSanitizer and
UBSan (tests/c/ragged_groups_test.cpp, tests/cunit.py).  Nothing is loaded
into Python and no GPU call is made."""
from cunit import build_and_run


def test_ragged_groups_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "ragged_groups_test")
