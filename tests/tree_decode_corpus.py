"""Inputs shared by the tree-decoder tests (tests/test_tree_decode.py on the
CPU, tests/c/tree_decode_test.cpp under the sanitizers, and
tests/test_gpu_tree_decode.py): the positive corpus of
test_native_encoder_matches_python in tree order, and the negative corpus --
inputs that are not what glfsx_tree_encode writes."""
import json
import random
import struct

from glfs_amd import bigblob, glfs, tree as T

POOL = ["plain", "<a&b>", "\n\r\t\b\f\x00\x1f\x7f", " x ", "é日本\U0001F600",
        "bad\udc80\udcff", "q\"b\\s", "", "%07d" % 5, "\udced\udca0\udc80"]


def decoded_name(name: str) -> str:
    """What a name reads back as: the encoder writes each byte of invalid
    UTF-8 as the escape of U+FFFD (encoding/json), so that is what any
    decoder of the line returns."""
    return json.loads(T.go_json_string(name))


def positive_entries(n=20000, seed=7, long_names=False):
    """Entries as test_native_encoder_matches_python builds them (every
    escaping class), in a tree's order: ascending by the bytes the names
    decode to, no duplicates.  long_names: the 300-2,000-byte names of
    test_tree_encode_device_vs_host, too long for a workgroup's LDS image."""
    rng = random.Random(seed)
    ents, seen = [], set()
    for i in range(n):
        name = rng.choice(POOL) + str(i) + rng.choice(POOL)
        if long_names and i % 700 == 3:
            name = "L" * rng.randrange(300, 2000) + name
        ty = rng.choice(["blob", "tree", "t<&>", " "])
        r = glfs.Ref(ty, bigblob.Root(bigblob.Ref(rng.randbytes(32), rng.randbytes(32)),
                                      rng.randrange(1 << 62), rng.choice([128, 2 << 20])))
        key = decoded_name(name).encode()
        if key not in seen:
            seen.add(key)
            ents.append((key, T.TreeEntry(name, rng.choice([0o644, T.MODE_TREE, 0]), r)))
    ents.sort(key=lambda p: p[0])
    return [e for _, e in ents]


def expected_entries(ents):
    """The entries as they read back (names through decoded_name)."""
    return [T.TreeEntry(decoded_name(e.name), e.file_mode, e.ref) for e in ents]


CID, DEK = "0123456789abcdef" * 4, "fedcba9876543210" * 4


def line(name='"plain"', mode="420", ty='"blob"', cid=CID, dek=DEK, size="9",
         bs="2097152", end="\n") -> bytes:
    """One line from its fields' JSON texts (a canonical one by default)."""
    s = ('{"name":' + name + ',"mode":' + mode + ',"ref":{"type":' + ty + ',"cid":"' + cid
         + '","dek":"' + dek + '","size":' + size + ',"blockSize":' + bs + "}}" + end)
    return s.encode("utf-8", "surrogateescape")


def raw(b: bytes) -> str:
    return b.decode("utf-8", "surrogateescape")


def listed_noncanonical():
    """Every non-canonical form the grammar names, one input each."""
    q = lambda s: '"' + s + '"'
    cases = [line(name=q(s)) for s in (
        "a\\/b", "\\u0041", "\\u003C", "\\ud83d\\ude00", "a<b", "a>b", "a&b", "a\x01b", "a\x7f\x1fb",
        raw(b"a\x80b"), raw(b"\xc0\xaf"), raw(b"\xe0\x80\xaf"), raw(b"\xed\xa0\x80"),
        raw(b"\xf5\x80\x80\x80"), raw(b"\xf4\x90\x80\x80"), raw(b"ab\xe6\x97"), raw(b"\xe2\x80\xa8"),
        raw(b"\xe2\x80\xa9"), "\\u0008", "\\u000a", "\\u007f", "\\u001F", "\\u0020", "\\uFFFD",
        "\\ufffe", "\\x41", "\\a", "\\", "\\u00", "a\tb")]
    cases += [line(ty=q(s)) for s in ("a<b", "\\/", raw(b"\xff"))]
    base = line().decode()
    cases += [
        base.replace('"name":', '"name": ').encode(),        # a space after a colon
        base.replace(',"mode"', ', "mode"').encode(),
        base.replace('"size":9,"blockSize":2097152', '"blockSize":2097152,"size":9').encode(),
        base.replace('{"name":"plain","mode":420', '{"mode":420,"name":"plain"').encode(),
        base.replace("}}", ',"x":1}}').encode(),               # an extra field
        base.replace("}}", "}} ").encode(),
        base.replace("}}", "}}}").encode(),
        b" " + base.encode(),
        line(cid=CID.upper()), line(dek=DEK.upper()), line(cid=CID[:63]), line(cid=CID + "0"),
        line(dek=DEK[:63]), line(dek=DEK + "a"), line(cid=CID[:63] + "g"), line(cid=CID[:63] + "/"),
        line(cid=CID[:63] + ":"), line(cid=CID[:63] + "`"), line(dek="G" + DEK[1:]),
        b"\n",                                               # a blank line
        line(end="\r\n"), line(end=""), line(end="\n\n"), line() + b"x",
        line(mode="4294967296"), line(mode="0420"), line(mode="-1"), line(mode="+1"),
        line(mode="1.0"), line(mode="1e3"), line(mode=""), line(mode="00"),
        line(size="18446744073709551616"), line(size="99999999999999999999"),
        line(size="184467440737095516150"), line(size="01"), line(size="-0"),
        line(bs="18446744073709551616"), line(bs="02097152"), line(bs=""),
        line(name="plain"), line(name="null"), line(mode='"420"'),
        b"{}\n", b"[]\n", b'{"name":"a"}\n',
    ]
    return cases


def negative_corpus():
    """(strict, bytes) pairs.  strict: the input cannot be what the encoder
    writes, so the decoder must flag it (a line of it NONCANON, or a tail).
    Not strict: a single-byte substitution that may spell another canonical
    line ('0' for a digit, 'A' in a name, a backslash before an 'n'); the
    decoder must flag it or decode it to columns that encode to the same
    bytes."""
    base = line()
    out = [(True, c) for c in listed_noncanonical()]
    out += [(True, base[:k]) for k in range(1, len(base))]     # every byte prefix
    for sub, strict in ((b'"', False), (b"\\", False), (b"\n", True), (b"0", False),
                        (b"A", False), (b"\x80", True), (b"\x00", True)):
        for k in range(len(base)):
            if base[k:k + 1] != sub:
                out.append((strict, base[:k] + sub + base[k + 1:]))
    return out


def write_negative_corpus(path) -> int:
    """The records tests/c/tree_decode_test.cpp reads: u32 length, u8 strict,
    the bytes."""
    cases = negative_corpus()
    with open(path, "wb") as f:
        for strict, b in cases:
            f.write(struct.pack("<IB", len(b), strict) + b)
    return len(cases)
