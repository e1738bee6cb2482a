"""The Writer's bookkeeping (glfs_amd/csrc/writer_book.h: the fill cursor of
the batch being staged and the stack of index levels with the order of their
Posts) as a stand-alone program built with the host compiler under
AddressSanitizer and UBSan (tests/c/writer_book_test.cpp, tests/cunit.py),
the oracle's streaming writer (oracle/oracle.c) compiled beside it as the
reference of the Post order.  Nothing is loaded into Python and no GPU call
is made."""
from cunit import build_and_run


def test_index_stack_and_fill_cursor_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "writer_book_test", sources=["oracle/oracle.c"])
