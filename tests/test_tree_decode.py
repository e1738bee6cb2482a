"""The native decoder of tree lines on the host (glfsx_tree_decode, the
inverse of glfsx_tree_encode; grammar in glfs_amd/csrc/tree_line.h) and
tree.read_tree_bytes over it.  CPU-only."""
import ctypes
import random

import numpy as np
import pytest

import tree_decode_corpus as C
from cunit import build_and_run
from glfs_amd import _native as N, tree as T


def test_decoder_under_sanitizers(tmp_path):
    """tests/c/tree_decode_test.cpp (its own main, tree.cpp compiled in) with
    -fsanitize=address,undefined: both round trips and the negative corpus,
    each input decoded from a heap buffer of exactly its length."""
    corpus = str(tmp_path / "negative.bin")
    assert C.write_negative_corpus(corpus) > 1000
    build_and_run(tmp_path, "tree_decode_test", args=[corpus], timeout=300)


@pytest.fixture(scope="module")
def positive():
    ents = C.positive_entries()
    data, ends = T.encode_lines(ents)
    return ents, data, ends


def _no_fallback(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("read_tree_bytes fell back to the Python decoder")
    monkeypatch.setattr(T, "read_tree_bytes_py", boom)


def test_read_tree_bytes_native_equals_python(positive, monkeypatch):
    """20,000 entries of every escaping class: the decoder reports none of
    the encoder's lines (asserted on the status array), and read_tree_bytes
    builds the same list as the Python loop -- without the loop: it is
    patched to raise while the native path runs."""
    ents, data, ends = positive
    want = T.read_tree_bytes_py(data)
    assert want == C.expected_entries(ents)
    c = T.decode_lines(data)
    assert c.n == len(ents) and c.n_bad == 0 and not c.tail
    assert not c.status.any()            # the share reported is zero
    assert c.name_offs[-1] == len(c.names) and c.type_offs[-1] == len(c.types)
    _no_fallback(monkeypatch)
    assert T.read_tree_bytes(data) == want
    assert T.read_tree_bytes(data[:ends[0]]) == want[:1]   # one line
    assert T.read_tree_bytes(b"") == []
    assert T.read_tree_bytes(bytearray(data[:ends[4]])) == want[:5]


def test_encoder_lines_never_noncanonical():
    """Unsorted entries (test_native_encoder_matches_python's own order, with
    names that are not clean): ORDER and NAME bits may be set, NONCANON never,
    and the columns are the inputs."""
    rng = random.Random(11)
    ents = C.positive_entries(3000, seed=11)
    rng.shuffle(ents)
    data, _ = T.encode_lines(ents)
    c = T.decode_lines(data)
    assert c.n == len(ents) and not (c.status & N.GLFSX_TREE_NONCANON).any()
    assert (c.status & N.GLFSX_TREE_ORDER).any()
    names = [bytes(c.names[a:b]) for a, b in zip(c.name_offs[:-1], c.name_offs[1:])]
    assert names == [C.decoded_name(e.name).encode() for e in ents]
    assert c.modes.tolist() == [e.file_mode for e in ents]
    assert c.sizes.tolist() == [e.ref.root.size for e in ents]
    assert c.block_sizes.tolist() == [e.ref.root.block_size for e in ents]
    assert c.roots.tobytes() == b"".join(e.ref.root.ref.cid + e.ref.root.ref.dek for e in ents)
    types = [bytes(c.types[a:b]).decode() for a, b in zip(c.type_offs[:-1], c.type_offs[1:])]
    assert types == [e.ref.type for e in ents]


def _same_outcome(data):
    """read_tree_bytes and read_tree_bytes_py: the same list, or the same
    exception type and message."""
    try:
        want = T.read_tree_bytes_py(data)
    except Exception as e:  # noqa: BLE001 - whatever the Python loop raises
        with pytest.raises(type(e)) as got:
            T.read_tree_bytes(data)
        assert str(got.value) == str(e)
        return "raises"
    assert T.read_tree_bytes(data) == want
    return "list"


def test_negative_corpus_same_outcome_as_python():
    """Every negative input alone and between two canonical lines: flagged by
    the decoder where it must be, and read_tree_bytes ends as the Python
    loop does (an exception of the same type and text, or the same list
    where Python's decoder accepts the input)."""
    a, b = C.line(name='"a"'), C.line(name='"zz"')
    seen = set()
    for strict, x in C.negative_corpus():
        c = T.decode_lines(x)
        flagged = c.tail or bool((c.status & N.GLFSX_TREE_NONCANON).any())
        assert flagged or not strict, x
        assert c.n_bad >= (1 if flagged else 0)
        if not flagged:  # canonical after all: it is a line the encoder writes
            assert c.n == 1 and c.n_bad == 0
            assert T.encode_lines(T.read_tree_bytes_py(x))[0] == x
        seen.add(_same_outcome(x))
        if strict:
            seen.add(_same_outcome(a + x + b))
    assert seen == {"raises", "list"}


def _named(names):
    return b"".join(C.line(name=T.go_json_string(n)) for n in names)


@pytest.mark.parametrize("names,bit", [
    (["a", "a"], N.GLFSX_TREE_ORDER), (["b", "a"], N.GLFSX_TREE_ORDER),
    (["ab", "a"], N.GLFSX_TREE_ORDER), (["a", "b", "a0"], N.GLFSX_TREE_ORDER),
    (["a/"], N.GLFSX_TREE_NAME), (["a//b"], N.GLFSX_TREE_NAME), (["./a"], N.GLFSX_TREE_NAME),
    (["a/../b"], N.GLFSX_TREE_NAME), ([""], N.GLFSX_TREE_NAME), (["/a"], N.GLFSX_TREE_NAME),
    (["a/."], N.GLFSX_TREE_NAME), (["."], N.GLFSX_TREE_NAME), (["a/.."], N.GLFSX_TREE_NAME),
    ([".."], 0), (["../a"], 0), (["../../a/b"], 0), (["a", "ab", "b"], 0), (["...", "a.b"], 0),
    (["a", "a\x00"], 0),
])
def test_order_and_name_bits(names, bit):
    data = _named(names)
    c = T.decode_lines(data)
    assert c.n == len(names) and not (c.status & N.GLFSX_TREE_NONCANON).any()
    got = 0
    for s in c.status.tolist():
        got |= s
    assert got == bit
    assert c.n_bad == int((c.status != 0).sum())
    assert _same_outcome(data) == ("raises" if bit else "list")


def test_name_rule_equals_clean_path():
    """The NAME bit's rule (no cleaned string is built) against
    tree.clean_path over a generated corpus: every string of up to 6 symbols
    over {a, ., /}, and random longer ones."""
    import itertools
    names = ["".join(p) for k in range(0, 7) for p in itertools.product("a./", repeat=k)]
    rng = random.Random(3)
    parts = ["a", ".", "..", "...", "", "b.c", ".a", "a.", "..a", "/", "é"]
    names += ["/".join(rng.choice(parts) for _ in range(rng.randrange(1, 6))) for _ in range(3000)]
    names = sorted(set(names))
    data = _named(names)
    c = T.decode_lines(data)
    assert c.n == len(names)
    for name, s in zip(names, c.status.tolist()):
        assert not s & N.GLFSX_TREE_NONCANON
        valid = name != "" and T.clean_path(name) == name
        assert bool(s & N.GLFSX_TREE_NAME) == (not valid), name


def test_capacities_and_counts_only():
    data = _named(["a", "b", "c"]) + b"tail"
    counts = (ctypes.c_uint64 * 5)()
    buf = np.frombuffer(data, dtype=np.uint8)
    nul = [None, 0, None, None, None, 0, None, None, None, None, None]
    assert N.lib.glfsx_tree_decode(buf.ctypes.data, len(data), *nul, 0, counts) == 0
    assert list(counts) == [3, 3, 12, 1, 1]
    status = np.full(5, 0xA5A5A5A5, dtype=np.uint32)
    args = [None, 0, None, None, None, 0, None, None, None, None]
    rc = N.lib.glfsx_tree_decode(buf.ctypes.data, len(data), *args, status.ctypes.data, 2, counts)
    assert rc == N.GLFSX_E_ARG and list(counts) == [3, 3, 12, 1, 1]
    assert (status == 0xA5A5A5A5).all()       # nothing written
    rc = N.lib.glfsx_tree_decode(buf.ctypes.data, len(data), *args, status.ctypes.data, 3, counts)
    assert rc == 0 and status.tolist() == [0, 0, 0, 0xA5A5A5A5, 0xA5A5A5A5]
    assert N.lib.glfsx_tree_decode(None, 0, *nul, 0, counts) == 0 and list(counts) == [0] * 5
    assert N.lib.glfsx_tree_decode(buf.ctypes.data, 4, *nul, 0, None) == N.GLFSX_E_ARG


def test_device_decoder_fails_cleanly_without_gpu():
    """glfsx_tree_decode_device returns GLFSX_E_DEVICE without a GPU before
    any argument is looked at (in the style of
    test_device_entry_points_fail_cleanly_without_gpu)."""
    if N.device_count() > 0:
        pytest.skip("GPU present")
    counts = (ctypes.c_uint64 * 5)(7, 7, 7, 7, 7)
    rc = N.lib.glfsx_tree_decode_device(1, 64, 1, 8, 1, 1, 1, 8, 1, 1, 1, 1, 1, 4, counts, None)
    assert rc == N.GLFSX_E_DEVICE and "no HIP device" in N.last_error()
    assert list(counts) == [7] * 5
    assert N.lib.glfsx_tree_decode_device(None, 0, None, 0, None, None, None, 0, None, None,
                                          None, None, None, 0, None, None) == N.GLFSX_E_DEVICE
