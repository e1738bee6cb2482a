"""The join of two trees' entries by name on the host (glfsx_tree_join and
tree_join.h, which the kernel shares): the stand-alone sanitizer program, the
host join through ctypes against a Python dict, and the device entry points
without a device.  CPU-only."""
import ctypes

import numpy as np
import pytest

import tree_join_cases as J
from cunit import build_and_run


def test_tree_join_under_sanitizers(tmp_path):
    """tests/c/tree_join_test.cpp (its own main, tree.cpp compiled in) with
    AddressSanitizer and UBSan: tree_join.h's compare, lower bound and class
    and glfsx_tree_join against brute force, every column in a heap buffer of
    exactly its length."""
    build_and_run(tmp_path, "tree_join_test", timeout=300)


def host_join(N, a, b, outputs=(True, True, True)):
    ca, cb = J.columns(a), J.columns(b)
    sa, sb = J.host_struct(N, ca), J.host_struct(N, cb)
    am = np.full(len(a) + 2, 0x5A5A5A5A, dtype=np.int64)
    bm = np.full(len(b) + 2, 0x5A5A5A5A, dtype=np.int64)
    ac = np.full(len(a) + 2, 0x5A, dtype=np.uint8)
    ptr = lambda x, on, step: x.ctypes.data + step if on else None
    rc = N.lib.glfsx_tree_join(ctypes.byref(sa), ctypes.byref(sb), ptr(am, outputs[0], 8),
                               ptr(bm, outputs[1], 8), ptr(ac, outputs[2], 1))
    assert rc == 0
    for x, v in ((am, 0x5A5A5A5A), (bm, 0x5A5A5A5A), (ac, 0x5A)):
        assert x[0] == v and x[-1] == v, "guard"
    return am[1:-1], bm[1:-1], ac[1:-1]


CASES = J.special_cases() + J.size_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_join_matches_dict(case):
    from glfs_amd import _native as N
    _, a, b = case
    am, bm, ac = host_join(N, a, b)
    wam, wbm, wac = J.py_join(a, b)
    assert np.array_equal(am, wam) and np.array_equal(bm, wbm) and np.array_equal(ac, wac)


def test_host_join_big_and_threaded():
    from glfs_amd import _native as N
    _, a, b = J.big_case()
    am, bm, ac = host_join(N, a, b)
    wam, wbm, wac = J.py_join(a, b)
    assert (wam >= 0).sum() > 10000 and set(wac.tolist()) == {J.ONLY, J.TREES, J.SAME, J.DIFF}
    assert np.array_equal(am, wam) and np.array_equal(bm, wbm) and np.array_equal(ac, wac)


def test_host_join_outputs_are_nullable():
    from glfs_amd import _native as N
    a, b = J.sized(257, 255, 1)
    want = J.py_join(a, b)
    for k in range(3):
        on = tuple(i == k for i in range(3))
        got = host_join(N, a, b, on)
        assert np.array_equal(got[k], want[k])
        for i in range(3):
            if i != k:
                assert (got[i] == (0x5A if i == 2 else 0x5A5A5A5A)).all()  # untouched


def test_host_join_unsorted_side_stays_in_range():
    from glfs_amd import _native as N
    _, a, b = J.unsorted_case()
    am, bm, ac = host_join(N, a, b)
    assert ((am >= -1) & (am < len(b))).all() and ((bm >= -1) & (bm < len(a))).all()
    assert (ac <= J.DIFF).all()


def test_join_constants_match_the_header():
    import os
    import re
    from glfs_amd import _native as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "glfsx.h")).read()
    got = dict(re.findall(r"#define (GLFSX_JOIN_[A-Z]+) (\d+)u", txt))
    assert got == {"GLFSX_JOIN_ONLY": "0", "GLFSX_JOIN_TREES": str(N.GLFSX_JOIN_TREES),
                   "GLFSX_JOIN_SAME": str(N.GLFSX_JOIN_SAME), "GLFSX_JOIN_DIFF": str(N.GLFSX_JOIN_DIFF)}
    assert (N.GLFSX_JOIN_ONLY, J.ONLY, J.TREES, J.SAME, J.DIFF) == (
        0, N.GLFSX_JOIN_ONLY, N.GLFSX_JOIN_TREES, N.GLFSX_JOIN_SAME, N.GLFSX_JOIN_DIFF)


def test_device_entry_points_need_a_device():
    """glfsx_tree_join_device and glfsx_tree_select_device return
    GLFSX_E_DEVICE without a GPU before they look at an argument."""
    from glfs_amd import _native as N
    if N.device_count() > 0:
        # with a device the same calls see their null arguments
        assert N.lib.glfsx_tree_join_device(None, None, None, None, None, None) == N.GLFSX_E_ARG
        counts = (ctypes.c_uint64 * 2)()
        assert N.lib.glfsx_tree_select_device(None, None, None, 0, None, 0, None, None, None, 0,
                                              None, None, None, None, None, 0, counts,
                                              None) == N.GLFSX_E_ARG
        return
    cols = N.glfsx_tree_cols()
    counts = (ctypes.c_uint64 * 2)()
    rc = N.lib.glfsx_tree_join_device(ctypes.byref(cols), ctypes.byref(cols), 1, 1, 1, None)
    assert rc == N.GLFSX_E_DEVICE and "no HIP device" in N.last_error()
    rc = N.lib.glfsx_tree_select_device(ctypes.byref(cols), ctypes.byref(cols), 1, 4, 1, 8, 1, 1, 1,
                                        8, 1, 1, 1, 1, 1, 4, counts, None)
    assert rc == N.GLFSX_E_DEVICE and "no HIP device" in N.last_error()
    assert N.lib.glfsx_tree_join_device(None, None, None, None, None, None) == N.GLFSX_E_DEVICE
