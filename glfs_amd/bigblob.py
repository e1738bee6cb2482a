"""Python mirror of the reference's bigblob write-path interface.

Reference: bigblob/machine.go, bigblob/blob.go, bigblob/ref.go, bigblob/index.go
(blobcache/glfs, Go).  Same names (snake_case), same argument meaning, same
error behaviour (Panic where Go panics, StoreError where Go returns the store
error).  Everything below is a thin ctypes call into libglfsx.so; the hashing
and encryption run in the gfx950 kernels.
"""
from __future__ import annotations

import ctypes
import io
import os
import stat
import time
from collections import OrderedDict
from dataclasses import dataclass
from typing import BinaryIO, Optional, Protocol, Union

from . import _native as N
from ._native import GlfsxError, Panic, StoreError  # noqa: F401  (re-exported)

DEK_SIZE = 32          # ref.go:16
CID_SIZE = 32          # blobcache.CIDSize [ext]
REF_SIZE = CID_SIZE + DEK_SIZE  # ref.go:52
MAX_REF_SIZE = REF_SIZE         # index.go:6
KIND_DATA, KIND_INDEX = 0, 1
KIND_COPY = 2  # a blob copied by Sync (its kind is not known to the copier)


@dataclass(frozen=True)
class Ref:
    """ref.go:54-57: Ref{CID, DEK}; binary form CID || DEK (ref.go:77-82)."""
    cid: bytes
    dek: bytes

    def marshal_binary(self) -> bytes:
        return self.cid + self.dek

    @staticmethod
    def from_bytes(x: bytes) -> "Ref":
        """ref.go:59-75 RefFromBytes."""
        if len(x) < REF_SIZE:
            raise ValueError(f"too small to be ref len={len(x)}")
        return Ref(bytes(x[:CID_SIZE]), bytes(x[CID_SIZE:REF_SIZE]))

    def to_json(self) -> dict:
        return {"cid": self.cid.hex(), "dek": self.dek.hex()}


@dataclass(frozen=True)
class Root:
    """blob.go:17-21 Root{Ref, Size, BlockSize}."""
    ref: Ref
    size: int
    block_size: int

    def equals(self, other: "Root") -> bool:  # blob.go:27-29
        return (self.size == other.size and self.block_size == other.block_size
                and self.ref == other.ref)


class WO(Protocol):
    """The write-only store boundary (bcsdk.WO, [ext]): MaxSize + Post.
    post() receives the ctext and the GPU-computed ref (CID || DEK)."""

    def max_size(self) -> int: ...

    def post(self, ctext: bytes, ref: bytes, kind: int) -> None: ...


def _salt_arg(salt: Optional[bytes]) -> Optional[bytes]:
    if salt is None:
        return None
    if len(salt) != 32:
        raise ValueError("salt must be 32 bytes")
    return bytes(salt)


def derive_key(salt: bytes, data: bytes, out_len: int = 32) -> bytes:
    """ref.go:152-161 DeriveKey(out, salt, input): BLAKE3 keyed with salt,
    first out_len XOF bytes (GPU)."""
    out = ctypes.create_string_buffer(max(out_len, 1))
    data = data if isinstance(data, (bytes, memoryview)) else bytes(data)
    N.check(N.lib.glfsx_derive_key(out, out_len, _salt_arg(salt), data, len(data)))
    return out.raw[:out_len]


def depth(size: int, block_size: int) -> int:
    """blob.go:256-264."""
    return N.lib.glfsx_depth(size, block_size)


def branching_factor(block_size: int) -> int:
    """blob.go:266-268."""
    return N.lib.glfsx_branching_factor(block_size)


def _make_post_cb(store: Optional[WO]):
    """(post function, error list, post_ctx) for the C-ABI.  A NativeStore
    is passed as its C function (no Python per Post)."""
    if store is None:
        return N.POST_FN(0), None, None
    native = getattr(store, "native_post", None)
    if native is not None:
        return native[0], [], native[1]
    errors: list = []

    def cb(_ctx, kind, ref, ctext, n):
        try:
            ct = ctypes.string_at(ctext, n) if n else b""
            store.post(ct, ctypes.string_at(ref, REF_SIZE), kind)
            return 0
        except Exception as e:  # surfaced as StoreError
            errors.append(e)
            return 1

    return N.POST_FN(cb), errors, None


class Writer:
    """blob.go:71-83 Writer (NewWriter/Write/Finish)."""

    def __init__(self, machine: "Machine", store: WO, salt: Optional[bytes],
                 cid_key: Optional[bytes] = None, strict: bool = False):
        self._cb, self._errors, ctx = _make_post_cb(store)
        err = ctypes.c_int(0)
        self._w = N.lib.glfsx_writer_new(machine.block_size, store.max_size(),
                                         _salt_arg(salt), cid_key, self._cb, ctx,
                                         ctypes.byref(err))
        if not self._w:
            N.check(err.value)
        self._strict = bool(strict)
        if strict:
            # blob.go:120-133 error timing: every Write returns after the
            # Posts of the blocks it completed were delivered
            N.check(N.lib.glfsx_writer_set_strict(self._w, 1))

    def _raise(self, rc: int):
        if rc == N.GLFSX_E_STORE and self._errors:
            raise StoreError(rc, repr(self._errors[0])) from self._errors[0]
        N.check(rc, (N.lib.glfsx_writer_error(self._w) or b"").decode(errors="replace"))

    def write_device(self, d_ptr: int, n: int, stream=None) -> int:
        """Write n bytes already in HBM (device pointer), ordered after the
        work on `stream` (a hipStream_t handle or None)."""
        rc = N.lib.glfsx_writer_write_device(self._w, d_ptr, n, stream)
        if rc:
            self._raise(rc)
        return n

    def write_ctext(self, ctext, refs: bytes, block_size: int) -> int:
        """Write the plaintext of data blocks given as ciphertext (decrypted
        on the GPU with each ref's DEK; the plaintext never leaves the
        device).  ctext: block j at j*block_size, the last block short."""
        if hasattr(ctext, "ctypes"):   # a numpy array: pass its memory as is
            buf, n = ctext.ctypes.data, ctext.nbytes
        elif isinstance(ctext, bytes):
            buf, n = ctext, len(ctext)
        else:
            mv = memoryview(ctext).cast("B")
            n = len(mv)
            buf = (ctypes.c_char * n).from_buffer(mv) if not mv.readonly else bytes(mv)
        rc = N.lib.glfsx_writer_write_ctext(self._w, buf, n, block_size, bytes(refs))
        if rc:
            self._raise(rc)
        return n

    def write_ctext_blocks(self, addrs, total: int, refs: bytes, block_size: int) -> int:
        """write_ctext with ciphertext block j at address addrs[j] (memory
        the caller keeps alive for the call, e.g. a NativeStore's blobs)."""
        arr = (ctypes.c_void_p * max(len(addrs), 1))(*addrs)
        rc = N.lib.glfsx_writer_write_ctext_blocks(self._w, arr, len(addrs), total, block_size,
                                                   bytes(refs))
        if rc:
            self._raise(rc)
        return total

    def flush(self) -> None:
        """Deliver the Posts of every complete block written so far."""
        rc = N.lib.glfsx_writer_flush(self._w)
        if rc:
            self._raise(rc)

    def write(self, data) -> int:
        """blob.go:120-133 (any bytes-like object; not copied on the way)."""
        if isinstance(data, bytes):
            buf, n = data, len(data)
        else:
            mv = memoryview(data).cast("B")
            n = len(mv)
            buf = (ctypes.c_char * n).from_buffer(mv) if not mv.readonly else bytes(mv)
        rc = N.lib.glfsx_writer_write(self._w, buf, n)
        if rc:
            self._raise(rc)
        return n

    def read_from(self, r) -> int:
        """io.ReaderFrom (io.Copy in Create/Concat, blob.go:213,341, uses it).
        A regular file (an *os.File, an io.ReaderAt) is read from its current
        position to its end by several threads at once straight into the
        writer's pinned staging (glfsx_writer_read_fd), then positioned after
        what was read; any other stream goes r.readinto() straight into the
        staging (glfsx_writer_reserve / glfsx_writer_commit), no second copy.
        Strict writer (the Go binding's default, integration/go/gpu.go
        ReadFrom): the call's batches are pipelined and their Posts delivered
        before it returns, so a store error comes back from this call -- where
        the reference's io.Copy returns it -- after the same Posts."""
        if not self._strict:
            return self._read_from(r)
        N.check(N.lib.glfsx_writer_set_strict(self._w, 0))
        try:
            got = self._read_from(r)
        finally:
            N.check(N.lib.glfsx_writer_set_strict(self._w, 1))
            rc = N.lib.glfsx_writer_flush(self._w)
            if rc:
                self._raise(rc)   # a store error before the reader's own
        return got

    def _read_from(self, r) -> int:
        fd = _regular_fd(r)
        if fd is not None:
            pos = r.tell()
            got = self.read_fd(fd, pos)
            r.seek(pos + got)
            return got
        total = 0
        buf, cap = ctypes.c_void_p(), ctypes.c_uint64()
        while True:
            rc = N.lib.glfsx_writer_reserve(self._w, ctypes.byref(buf), ctypes.byref(cap))
            if rc:
                self._raise(rc)
            view = (ctypes.c_char * cap.value).from_address(buf.value)
            n = r.readinto(memoryview(view).cast("B"))
            rc = N.lib.glfsx_writer_commit(self._w, n or 0)
            if rc:
                self._raise(rc)
            if n is None:
                # a non-blocking stream with nothing ready yet: not the end
                # of the input (io.Copy goes on after a (0, nil) Read)
                time.sleep(0.0005)
                continue
            total += n
            if n == 0:
                return total

    def read_fd(self, fd: int, offset: int = 0, n: int = (1 << 64) - 1) -> int:
        """n bytes (default: to the end) of file descriptor fd from `offset`
        into the writer, pread by several threads at once
        (glfsx_writer_read_fd; the descriptor's own offset is not used).
        Returns the bytes taken."""
        got = ctypes.c_uint64()
        rc = N.lib.glfsx_writer_read_fd(self._w, fd, offset, n, ctypes.byref(got))
        if rc:
            self._raise(rc)
        return got.value

    def read_at(self, read_at, offset: int = 0, n: int = (1 << 64) - 1) -> int:
        """io.ReaderAt route (glfsx_writer_read_at): read_at(buf: memoryview,
        off: int) -> bytes read (0 at the end), called from several threads
        at once on disjoint ranges.  Returns the bytes taken."""
        def cb(_ctx, buf, ln, off):
            try:
                return int(read_at(memoryview((ctypes.c_char * ln).from_address(buf)).cast("B"),
                                   off))
            except Exception:
                return -5   # EIO
        fn = N.READ_AT_FN(cb)
        got = ctypes.c_uint64()
        rc = N.lib.glfsx_writer_read_at(self._w, fn, None, offset, n, ctypes.byref(got))
        if rc:
            self._raise(rc)
        return got.value

    def finish(self) -> Root:
        """blob.go:135-150."""
        r = N.glfsx_root()
        rc = N.lib.glfsx_writer_finish(self._w, ctypes.byref(r))
        if rc:
            self._raise(rc)
        return Root(Ref.from_bytes(bytes(r.ref)), r.size, r.block_size)

    def close(self) -> None:
        if self._w:
            N.lib.glfsx_writer_free(self._w)
            self._w = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _regular_fd(r) -> Optional[int]:
    """The descriptor of a seekable regular file behind r, or None.

    Only a plain file object qualifies: an io.FileIO, or a buffered reader
    whose raw stream is one (what open(p, "rb") returns), so that tell() is
    a byte offset into the descriptor's file.  A wrapper that transforms
    the bytes (gzip / bz2 / lzma files, whose fileno() is the compressed
    file's and whose tell() is a decompressed position) reads through
    readinto instead."""
    raw = r
    if isinstance(r, (io.BufferedReader, io.BufferedRandom)):
        raw = r.raw
    if type(raw) is not io.FileIO:
        return None
    try:
        if not r.seekable():
            return None
        fd = r.fileno()
        return fd if stat.S_ISREG(os.fstat(fd).st_mode) else None
    except (OSError, ValueError, io.UnsupportedOperation):
        return None


def _copy(w, r: Union[bytes, bytearray, memoryview, BinaryIO]) -> None:
    """io.Copy: a bytes-like source is one Write (bytes.Reader is a WriterTo);
    a stream with readinto goes through the Writer's ReadFrom (read straight
    into the staging), any other stream in 32 KiB pieces."""
    if isinstance(r, (bytes, bytearray, memoryview)):
        w.write(r)
        return
    if hasattr(r, "readinto"):
        w.read_from(r)
        return
    while True:
        piece = r.read(32 * 1024)
        if not piece:
            return
        w.write(piece)


class Machine:
    """bigblob/machine.go:32-55.  block_size 0 = the store's MaxSize."""

    def __init__(self, block_size: int = 0, cache_size: int = 64):
        if block_size < 0:  # machine.go:24 WithBlockSize panics
            raise Panic(N.GLFSX_E_ARG, str(block_size))
        self.block_size = block_size
        self.cache_size = cache_size
        # machine.go:36 getF LRU, keyed by Ref.Key() (= BLAKE3(CID||DEK) in
        # the reference; the 64-B ref itself identifies the same entry).  An
        # entry is (plaintext, checks): None for an unchecked read, else the
        # (cid_key, level salt) it passed glfsx_open under
        self._cache: "OrderedDict[bytes, tuple]" = OrderedDict()
        self._salts: dict = {}   # blob salt -> (indexSalt, rawSalt)

    # ------------------------------------------------------------ read side
    def _level_salts(self, salt: Optional[bytes]) -> tuple:
        """blob.go:99-101: (indexSalt, rawSalt) of a blob's salt, derived once
        per Machine and salt (derive_key is a GPU call); (None, None) for no
        salt."""
        if salt is None:
            return None, None
        salt = _salt_arg(salt)
        got = self._salts.get(salt)
        if got is None:
            if len(self._salts) >= 64:
                self._salts.clear()
            got = self._salts[salt] = (derive_key(salt, b"index"), derive_key(salt, b"raw"))
        return got

    def get_f(self, store, ref: Ref, salt: Optional[bytes] = None,
              cid_key: Optional[bytes] = None) -> bytes:
        """ref.go:113-126 getF: fetch the ctext by CID, decrypt with the DEK
        (ChaCha20 on the GPU), cache the plaintext.  With salt (the level's
        salt as post took it: rawSalt or indexSalt) or cid_key (the store's)
        the block goes through glfsx_open instead: its bytes must hash to the
        CID (keyed by cid_key) and, when salt is given, its plaintext to the
        DEK; a bad block raises ErrCorrupt and never enters the cache, and a
        cached plaintext serves a checked read only if it passed the same
        checks."""
        key = ref.marshal_binary()
        checked = salt is not None or cid_key is not None
        want = (cid_key, _salt_arg(salt)) if checked else None
        hit = self._cache.get(key)
        if hit is not None:
            have = hit[1]
            if not checked or (have is not None and have[0] == want[0]
                               and want[1] in (None, have[1])):
                self._cache.move_to_end(key)
                return hit[0]
        if checked:
            data = open_block(store.get(ref.cid), ref, salt, cid_key)
        else:
            data = crypto_xor(ref.dek, store.get(ref.cid))
        if self.cache_size > 0:
            self._cache[key] = (data, want)
            self._cache.move_to_end(key)
            if len(self._cache) > self.cache_size:
                self._cache.popitem(last=False)
        return data

    def get_piece(self, store, root: Ref, bf: int, level: int, block_index: int,
                  salt: Optional[bytes] = None, cid_key: Optional[bytes] = None) -> Ref:
        """blob.go:53-69 getPiece: walk index nodes down to the block's ref.
        Index nodes must be exactly bf*64 bytes (newIndexUsing).  With salt
        (the blob's, as Create took it) or cid_key every node on the way is
        checked under DeriveKey(salt, "index") (get_f); a bad node raises
        ErrCorrupt with its level."""
        index_salt = self._level_salts(salt)[0]
        while level > 0:
            try:
                data = self.get_f(store, root, index_salt, cid_key)
            except ErrCorrupt as e:
                raise e.at_level(level) from None
            if len(data) != bf * MAX_REF_SIZE:
                raise ValueError("data is not correct size for index")
            span = bf ** (level - 1)
            i = block_index // span
            root = Ref.from_bytes(data[i * MAX_REF_SIZE:(i + 1) * MAX_REF_SIZE])
            block_index %= span
            level -= 1
        return root

    def read_at(self, store, x: Root, offset: int, n: int, salt: Optional[bytes] = None,
                cid_key: Optional[bytes] = None) -> tuple:
        """blob.go:31-51 ReadAt: at most ONE block per call (quirk kept).
        Returns (data, eof) where eof mirrors the io.EOF the reference
        returns when the read ends exactly at Size.  With salt (the blob's) or
        cid_key the index nodes and the data block are checked as they are
        read (get_piece, get_f): the data block under DeriveKey(salt, "raw"),
        the empty blob under the index salt; ErrCorrupt carries the bad
        blob's CID and level."""
        level = depth(x.size, x.block_size)
        bf = branching_factor(x.block_size)
        block_index, rel = divmod(offset, x.block_size)
        ref = self.get_piece(store, x.ref, bf, level, block_index, salt, cid_key)
        index_salt, raw_salt = self._level_salts(salt)
        try:
            data = self.get_f(store, ref, index_salt if x.size == 0 else raw_salt, cid_key)
        except ErrCorrupt as e:
            raise e.at_level(0) from None
        if rel > len(data):  # Go slices data[relOffset:] and panics
            raise Panic(N.GLFSX_E_ARG, "slice bounds out of range")
        out = data[rel:rel + n]
        return out, offset + len(out) == x.size

    def new_reader(self, store, root: Root, salt: Optional[bytes] = None,
                   cid_key: Optional[bytes] = None) -> "Reader":
        """io.go:23-30 (salt / cid_key: a Reader whose every read is checked,
        see read_at)."""
        return Reader(self, store, root, salt, cid_key)

    def traverse(self, store, root: Root, enter, exit, salt: Optional[bytes] = None,
                 cid_key: Optional[bytes] = None) -> None:
        """traverse.go:18-52: pre-order Enter(cid) -> bool (False skips the
        subtree), post-order Exit(level, ref).  Children stop at the first
        all-zero CID.  With salt (the blob's) or cid_key every index node is
        checked as it is read (get_f under DeriveKey(salt, "index"))."""
        if root.block_size == 0:
            raise ValueError("block size cannot be zero")
        self._traverse(store, root.block_size, depth(root.size, root.block_size),
                       root.ref, enter, exit, self._level_salts(salt)[0], cid_key)

    def _traverse(self, store, bs, level, x: Ref, enter, exit, index_salt=None,
                  cid_key=None) -> None:
        if not enter(x.cid):
            return
        if level > 0:
            try:
                data = self.get_f(store, x, index_salt, cid_key)
            except ErrCorrupt as e:
                raise e.at_level(level) from None
            if len(data) != bs:
                raise ValueError("data is not correct size for index")
            for i in range(bs // MAX_REF_SIZE):
                r2 = Ref.from_bytes(data[i * MAX_REF_SIZE:(i + 1) * MAX_REF_SIZE])
                if r2.cid == bytes(CID_SIZE):
                    break
                self._traverse(store, bs, level - 1, r2, enter, exit, index_salt, cid_key)
        exit(level, x)

    def sync(self, dst, src, x: Root, fn=None, verify: bool = False,
             cid_key: Optional[bytes] = None) -> None:
        """blob.go:270-315 Sync: nothing to do if dst has the root CID;
        otherwise call fn(reader), then copy every reachable blob, children
        before their index node (the reference's post-order).  The index
        levels are read one batched GPU decrypt per level.

        verify: the reference's copyBlob ends in dst.Post, which re-hashes the
        bytes (blob.go:307-315); a pre-hashed dst does not.  With verify every
        blob's CID (keyed by cid_key) is checked on the GPU before it is
        handed to dst -- index nodes in the level walk, data blocks in
        batches of at most 64 MiB, CID only, no plaintext -- and the bytes
        posted are the bytes checked.  A mismatch raises ErrCorrupt and
        nothing more is posted; the post order is unchanged."""
        if exists_unit(dst, x.ref.cid):
            return
        if fn is not None:
            fn(self.new_reader(src, x))
        nodes: dict = {}   # cid -> checked ctext of the index nodes
        batch: dict = {}   # the same for the data blocks of the current batch
        if verify:
            levels = _tree_levels(src.get, x, None, cid_key, _check=True, _keep=nodes)
        else:
            levels = _tree_levels(src.get, x)
        bf = branching_factor(x.block_size)
        data = levels[-1]
        per = max(1, SYNC_VERIFY_BYTES // max(x.block_size, 1))

        def copy(ref: Ref, k: int, j: int) -> None:
            if not verify:
                return copy_blob(dst, src, ref)
            if k + 1 < len(levels):
                ct = nodes[ref.cid]
            else:
                if ref.cid not in batch:   # the next batch: check it first
                    part = data[j:j + per]
                    cts = [src.get(r.cid) for r in part]
                    try:
                        open_level(cts, part, x.block_size, None, cid_key, want_ptext=False)
                    except ErrCorrupt as e:
                        raise ErrCorrupt(j + e.index, e.cid, e.status, 0) from None
                    batch.clear()
                    batch.update((r.cid, c) for r, c in zip(part, cts))
                ct = batch[ref.cid]
            dst.post(ct, ref.cid + bytes(DEK_SIZE), KIND_COPY)

        def emit(k: int, j: int) -> None:
            if k + 1 < len(levels):
                for c in range(j * bf, min((j + 1) * bf, len(levels[k + 1]))):
                    emit(k + 1, c)
            copy(levels[k][j], k, j)

        if x.size == 0:
            if verify:
                _check_empty(x.ref, None, cid_key, src.get(x.ref.cid))
            copy_blob(dst, src, x.ref)
        else:
            emit(0, 0)

    def verify(self, store, root: Root, salt: Optional[bytes] = None,
               cid_key: Optional[bytes] = None) -> int:
        """fsck of root's tree: every reachable blob's bytes must hash to the
        CID they are stored under (keyed by cid_key), and -- when the salt
        the blob was created with is given -- every blob's plaintext to its
        ref's DEK.  One batched GPU call per index level, the data level in
        batches of at most 64 MiB without plaintext.  Returns the number of
        blobs checked; raises ErrCorrupt (with the blob's CID and level)."""
        if root.size == 0:
            _check_empty(root.ref, salt, cid_key, store.get(root.ref.cid))
            return 1
        levels = _tree_levels(store.get, root, salt, cid_key, _check=True)
        raw = derive_key(salt, b"raw") if salt is not None else None
        data, bs = levels[-1], root.block_size
        per = max(1, SYNC_VERIFY_BYTES // bs)
        for j in range(0, len(data), per):
            part = data[j:j + per]
            try:
                open_level([store.get(r.cid) for r in part], part, bs, raw, cid_key,
                           want_ptext=False)
            except ErrCorrupt as e:
                raise ErrCorrupt(j + e.index, e.cid, e.status, 0) from None
        return sum(len(lv) for lv in levels)

    def populate(self, store, root: Root, dst, salt: Optional[bytes] = None,
                 cid_key: Optional[bytes] = None) -> None:
        """blob.go:317-331 Populate: add every reachable CID that dst lacks
        (Enter skips subtrees dst already has; Exit adds).  salt / cid_key:
        the index nodes are checked as traverse reads them."""
        self.traverse(store, root, lambda cid: not exists_unit(dst, cid),
                      lambda level, ref: dst.add(ref.cid), salt, cid_key)

    def post(self, store: WO, salt: Optional[bytes], data: bytes,
             cid_key: Optional[bytes] = None) -> Ref:
        """ref.go:98-111 post: DEK = DeriveKey(salt, ptext), ctext =
        ChaCha20(DEK) ^ ptext, CID = the store's hash of ctext -- all on the
        GPU -- then store.Post(ctext).  A store error propagates."""
        data = bytes(data)
        ref = ctypes.create_string_buffer(REF_SIZE)
        ct = ctypes.create_string_buffer(max(len(data), 1))
        N.check(N.lib.glfsx_post(_salt_arg(salt) or bytes(32), data, len(data), ct, ref,
                                 cid_key))
        store.post(ct.raw[:len(data)], ref.raw, KIND_DATA)
        return Ref.from_bytes(ref.raw)

    def new_writer(self, store: WO, salt: Optional[bytes] = None,
                   cid_key: Optional[bytes] = None, strict: bool = False) -> Writer:
        """blob.go:85-114 (strict: the reference's per-Write error timing)."""
        return Writer(self, store, salt, cid_key, strict)

    def concat(self, store, block_size: int, salt: Optional[bytes], *roots: Root) -> Root:
        """blob.go:333-345."""
        return _concat(self, store, block_size, salt, roots)

    def create(self, store: WO, salt: Optional[bytes], r,
               cid_key: Optional[bytes] = None) -> Root:
        """blob.go:209-217."""
        w = self.new_writer(store, salt, cid_key)
        try:
            _copy(w, r)
            return w.finish()
        finally:
            w.close()


def _gather(store, refs, size: int):
    """The blobs of `refs`, concatenated into one uninitialised buffer of
    `size` bytes (straight from a NativeStore's memory when possible)."""
    import numpy as np
    out = np.empty(size, dtype=np.uint8)
    base, off = out.ctypes.data, 0
    direct = hasattr(store, "get_into")
    for ref in refs:
        if direct:
            off += store.get_into(ref.cid, base + off, size - off)
        else:
            c = store.get(ref.cid)
            if off + len(c) > size:
                raise ValueError("blob larger than its root says")
            out[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
            off += len(c)
    if off != size:
        raise ValueError(f"blob read {off} bytes, root says {size}")
    return out


def _concat(machine: "Machine", store, block_size: int, salt, roots, cid_key=None) -> Root:
    """blob.go:333-345 Concat: every root's bytes, in order, through a new
    Writer.  The index levels are read with one batched decrypt per level;
    the data blocks go to the Writer as ciphertext and are decrypted on the
    GPU right into its staging (glfsx_writer_write_ctext), so the plaintext
    never crosses PCIe.  Like the reference, the `block_size` argument is
    ignored: the writer uses the machine's block size (quirk recorded in
    SURVEY's appendix)."""
    w = machine.new_writer(store, salt, cid_key)
    try:
        for r in roots:
            if r.size == 0:
                continue
            data_refs = _tree_levels(store.get, r)[-1]
            if r.block_size % 64:
                w.write(read_all(store, r))
                continue
            refs = b"".join(x.marshal_binary() for x in data_refs)
            if hasattr(store, "addr"):   # blocks straight from the store's memory
                addrs, got = [], 0
                for i, x in enumerate(data_refs):
                    a, n = store.addr(x.cid)
                    want = r.block_size if i + 1 < len(data_refs) else \
                        r.size - r.block_size * (len(data_refs) - 1)
                    if n != want:
                        raise ValueError(f"block {i} has {n} bytes, the root says {want}")
                    addrs.append(a)
                    got += n
                w.write_ctext_blocks(addrs, got, refs, r.block_size)
                continue
            ct = _gather(store, data_refs, r.size)
            w.write_ctext(ct, refs, r.block_size)
        return w.finish()
    finally:
        w.close()


class Reader:
    """io.go:15-54 Reader: Read / ReadAt / Seek over a Root (each call reads
    from at most one block, as the reference's ReadAt does).  With salt (the
    blob's, as Create took it) or cid_key (the store's) every block and index
    node a read touches is checked (Machine.read_at) and a bad one raises
    ErrCorrupt instead of coming back as data."""
    SEEK_SET, SEEK_CUR, SEEK_END = 0, 1, 2

    def __init__(self, machine: Machine, store, root: Root, salt: Optional[bytes] = None,
                 cid_key: Optional[bytes] = None):
        self.o, self.store, self.root, self.offset = machine, store, root, 0
        self.salt, self.cid_key = salt, cid_key

    def read_at(self, n: int, at: int) -> tuple:
        return self.o.read_at(self.store, self.root, at, n, self.salt, self.cid_key)

    def read(self, n: int = -1) -> bytes:
        """Python io semantics on top of ReadAt: returns b"" at EOF; n < 0
        reads to the end (block by block)."""
        if self.offset >= self.root.size:
            return b""
        if n < 0:
            parts = []
            while self.offset < self.root.size:
                parts.append(self.read(self.root.size - self.offset))
            return b"".join(parts)
        data, _ = self.o.read_at(self.store, self.root, self.offset, n, self.salt, self.cid_key)
        self.offset += len(data)
        return data

    def seek(self, offset: int, whence: int = 0) -> int:
        if whence == self.SEEK_SET:
            self.offset = offset
        elif whence == self.SEEK_CUR:
            self.offset += offset
        elif whence == self.SEEK_END:
            self.offset = self.root.size + offset
        else:
            raise Panic(N.GLFSX_E_ARG, "invalid whence")
        return self.offset


def exists_unit(store, cid: bytes) -> bool:
    """machine.go:86-92 ExistsUnit."""
    return bool(store.exists(cid))


def copy_blob(dst, src, ref: Ref) -> None:
    """blob.go:306-315 copyBlob: Get the ctext from src, Post it to dst.
    The destination is a pre-hashed store (its Post takes the CID with the
    bytes), so the copy keeps the CID the source holds."""
    ct = src.get(ref.cid)
    dst.post(ct, ref.cid + bytes(DEK_SIZE), KIND_COPY)


class CIDSet:
    """A minimal AddExister (machine.go:81-84): Exists + Add over CIDs."""

    def __init__(self):
        self.cids: set = set()

    def exists(self, cid: bytes) -> bool:
        return cid in self.cids

    def add(self, cid: bytes) -> None:
        self.cids.add(cid)


class ErrNotFound(KeyError):
    """blobcache.ErrNotFound{CID} [ext]: Get of a CID the store lacks."""

    def __init__(self, cid: bytes):
        super().__init__(f"blob not found: {cid.hex()}")
        self.cid = cid


class ErrCorrupt(GlfsxError):
    """A blob failed the verified read (glfsx_open_batch): its bytes do not
    hash to the CID it was fetched under (status & 1), or its plaintext is
    not the one its ref's DEK was derived from (status & 2).  index: the
    blob's position in the batch or level it was checked in; level: its tree
    level (0 = data blocks) when known."""

    def __init__(self, index: int, cid: bytes, status: int, level: Optional[int] = None):
        what = {1: "CID", 2: "DEK", 3: "CID and DEK"}.get(status, f"status {status}")
        where = "" if level is None else f" at level {level}"
        super().__init__(N.GLFSX_E_CORRUPT,
                         f"blob {bytes(cid).hex()} (index {index}{where}) failed its "
                         f"{what} check")
        self.index, self.cid, self.status, self.level = index, bytes(cid), status, level

    def at_level(self, level: int) -> "ErrCorrupt":
        return ErrCorrupt(self.index, self.cid, self.status, level)


class NativeStore:
    """The native store of the C-ABI (glfsx_store_*, include/glfsx.h): an
    in-memory content-addressed store whose Post takes the GPU-computed CID
    (mode "trust": a pre-hashed Post; verify_every=k re-hashes every k-th
    Post on the host) or re-hashes every ctext on the host as blobcache's
    MemStore.Post does behind ref.go:103 (mode "hash").  The Writer hands it
    its Posts as a C function pointer: no Python per Post."""

    def __init__(self, max_size: int, mode: str = "trust", verify_every: int = 0,
                 keep_data: bool = True, cid_key: Optional[bytes] = None):
        m = {"trust": N.GLFSX_STORE_TRUST, "hash": N.GLFSX_STORE_HASH}[mode]
        self._max = max_size
        self._s = N.lib.glfsx_store_new(max_size, m, verify_every, int(keep_data), cid_key)
        if not self._s:
            raise N.GlfsxError(N.GLFSX_E_UNSUPPORTED,
                               "host BLAKE3 (libclang-cpp.so) unavailable for a hashing store")
        self.native_post = (ctypes.cast(N.lib.glfsx_store_post, N.POST_FN),
                            ctypes.c_void_p(self._s))

    def max_size(self) -> int:
        return self._max

    def post(self, ctext: bytes, ref: bytes, kind: int = KIND_DATA) -> None:
        rc = N.lib.glfsx_store_post(self._s, kind, ref, ctext, len(ctext))
        if rc:
            raise StoreError(rc, (N.lib.glfsx_store_error(self._s) or b"").decode())

    def exists(self, cid: bytes) -> bool:
        return bool(N.lib.glfsx_store_exists(self._s, bytes(cid)))

    def get(self, cid: bytes) -> bytes:
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        if N.lib.glfsx_store_get(self._s, bytes(cid), ctypes.byref(p), ctypes.byref(n)):
            raise ErrNotFound(bytes(cid))
        return ctypes.string_at(p, n.value) if n.value else b""

    def addr(self, cid: bytes):
        """(address, length) of the blob in the store's own memory, valid
        until the store is freed (glfsx_store_get)."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        if N.lib.glfsx_store_get(self._s, bytes(cid), ctypes.byref(p), ctypes.byref(n)):
            raise ErrNotFound(bytes(cid))
        return p.value or 0, n.value

    def get_into(self, cid: bytes, dst_addr: int, cap: int) -> int:
        """Copy the blob straight from the store's memory to dst_addr (at
        most cap bytes); returns its length."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        if N.lib.glfsx_store_get(self._s, bytes(cid), ctypes.byref(p), ctypes.byref(n)):
            raise ErrNotFound(bytes(cid))
        if n.value > cap:
            raise ValueError("blob larger than the destination")
        if n.value:
            ctypes.memmove(dst_addr, p, n.value)
        return n.value

    def stats(self) -> dict:
        posts, nbytes, hashed = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        blobs = N.lib.glfsx_store_stats(self._s, ctypes.byref(posts), ctypes.byref(nbytes),
                                        ctypes.byref(hashed))
        return {"blobs": blobs, "posts": posts.value, "bytes": nbytes.value,
                "rehashed": hashed.value}

    def __len__(self) -> int:
        return self.stats()["blobs"]

    def close(self) -> None:
        if self._s:
            N.lib.glfsx_store_free(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MemStore:
    """In-memory stand-in for blobcache's schema.MemStore [ext].  It keeps
    (CID -> ctext) as posted by the GPU path (a pre-hashed Post: the CID was
    computed on the device).  Tests re-verify every CID with the oracle."""

    def __init__(self, max_size: int):
        self._max = max_size
        self.blobs: dict[bytes, bytes] = {}
        self.log: list[tuple[int, bytes, int]] = []  # (kind, ref, len)

    def max_size(self) -> int:
        return self._max

    def post(self, ctext: bytes, ref: bytes, kind: int = KIND_DATA) -> None:
        if len(ctext) > self._max:
            raise ValueError(f"blob too large {len(ctext)} > {self._max}")
        self.blobs[ref[:CID_SIZE]] = ctext
        self.log.append((kind, ref, len(ctext)))

    def __len__(self) -> int:
        return len(self.blobs)

    def exists(self, cid: bytes) -> bool:
        return cid in self.blobs

    def get(self, cid: bytes) -> bytes:
        try:
            return self.blobs[cid]
        except KeyError:
            raise ErrNotFound(cid) from None

    def delete(self, cids) -> None:
        for cid in cids:
            self.blobs.pop(cid, None)


def crypto_xor(dek: bytes, data: bytes) -> bytes:
    """ref.go:137-144 cryptoXOR (ChaCha20, zero nonce, counter 0) on the GPU;
    self-inverse, so it is also getF's decrypt (ref.go:122)."""
    data = bytes(data)
    out = ctypes.create_string_buffer(max(len(data), 1))
    N.check(N.lib.glfsx_chacha20_xor(bytes(dek), data, out, len(data)))
    return out.raw[:len(data)]


def open_block(ctext, ref: Ref, salt: Optional[bytes], cid_key: Optional[bytes] = None,
               want_ptext: bool = True) -> bytes:
    """getF with its checks for one block (glfsx_open; ref.go:113-126): ctext
    must hash to ref's CID (keyed by cid_key) and, when salt is given (the
    level's salt as post took it), its plaintext to ref's DEK.  One launch up
    to 64 KiB.  Returns the plaintext (b"" when want_ptext is false); raises
    ErrCorrupt(0, cid, status)."""
    ctext = bytes(ctext)
    out = ctypes.create_string_buffer(max(len(ctext), 1)) if want_ptext else None
    st = ctypes.c_uint32(0)
    rc = N.lib.glfsx_open(_salt_arg(salt), cid_key, ref.marshal_binary(), ctext, len(ctext),
                          out, ctypes.byref(st))
    if rc == N.GLFSX_E_CORRUPT:
        raise ErrCorrupt(0, ref.cid, st.value)
    N.check(rc)
    return out.raw[:len(ctext)] if want_ptext else b""


def decrypt_level(ctexts, refs, block_size: int) -> list:
    """getF (ref.go:113-126) for the blobs of one tree level at once: every
    ctext but the last is exactly block_size bytes (index nodes; a blob's
    data blocks), decrypted with its ref's DEK in ONE batched GPU call
    (glfsx_decrypt_batch).  Returns the plaintexts in order."""
    n = len(ctexts)
    if n == 0:
        return []
    if any(len(c) != block_size for c in ctexts[:-1]) or len(ctexts[-1]) > block_size \
            or block_size % 64:
        return [crypto_xor(r.dek, c) for r, c in zip(refs, ctexts)]
    data = b"".join(ctexts)
    rb = b"".join(r.marshal_binary() for r in refs)
    out = ctypes.create_string_buffer(max(len(data), 1))
    N.check(N.lib.glfsx_decrypt_batch(data, len(data), block_size, rb, out))
    raw = out.raw
    return [raw[i * block_size:i * block_size + len(c)] for i, c in enumerate(ctexts)]


SYNC_VERIFY_BYTES = 64 << 20   # data blocks checked per batch (sync, verify)


def _open_call(salt, cid_key, data, total: int, block_size: int, rb: bytes, out):
    """One glfsx_open_batch call; returns None, or (index, status) of the
    first bad block."""
    n = -(-total // block_size)
    st = (ctypes.c_uint32 * n)()
    rc = N.lib.glfsx_open_batch(_salt_arg(salt), cid_key, data, total, block_size, rb, out,
                                st, None)
    if rc == N.GLFSX_E_CORRUPT:
        i = next(i for i in range(n) if st[i])
        return i, st[i]
    N.check(rc)
    return None


def _empty_status(ref: Ref, level_salt: Optional[bytes], cid_key: Optional[bytes]) -> int:
    """The status word of a blob of no bytes (nothing to hash on the device):
    its ref must be what posting b"" under the level's salt gives."""
    got = ctypes.create_string_buffer(REF_SIZE)
    N.check(N.lib.glfsx_post(_salt_arg(level_salt) or bytes(32), b"", 0,
                             ctypes.create_string_buffer(1), got, cid_key))
    return (N.GLFSX_BAD_CID if got.raw[:CID_SIZE] != ref.cid else 0) | \
        (N.GLFSX_BAD_DEK if level_salt is not None and got.raw[CID_SIZE:] != ref.dek else 0)


def _check_empty(ref: Ref, salt: Optional[bytes], cid_key: Optional[bytes],
                 stored: Optional[bytes] = None) -> None:
    """The empty blob (blob.go:120-206: one post of no bytes under the index
    salt of the blob's salt); stored: what the store holds under its CID."""
    status = _empty_status(ref, derive_key(salt, b"index") if salt is not None else None,
                           cid_key)
    if stored:   # bytes under the CID of no bytes
        status |= N.GLFSX_BAD_CID
    if status:
        raise ErrCorrupt(0, ref.cid, status, 0)


def open_level(ctexts, refs, block_size: int, salt: Optional[bytes],
               cid_key: Optional[bytes] = None, want_ptext: bool = True) -> list:
    """decrypt_level with the checks: every ctext must hash to its ref's CID
    (keyed by cid_key) and, when salt is given (the level's salt as post took
    it: rawSalt or indexSalt), its plaintext to its ref's DEK -- one
    glfsx_open_batch call for a uniform level, one call per blob otherwise.
    Returns the plaintexts in order (an empty list when want_ptext is
    false); raises ErrCorrupt for the first bad blob."""
    n = len(ctexts)
    if n == 0:
        return []
    uniform = not (any(len(c) != block_size for c in ctexts[:-1])
                   or len(ctexts[-1]) > block_size or len(ctexts[-1]) == 0 or block_size % 64)
    outs = []
    if uniform:
        data = b"".join(ctexts)
        rb = b"".join(r.marshal_binary() for r in refs)
        out = ctypes.create_string_buffer(len(data)) if want_ptext else None
        bad = _open_call(salt, cid_key, data, len(data), block_size, rb, out)
        if bad:
            raise ErrCorrupt(bad[0], refs[bad[0]].cid, bad[1])
        if want_ptext:
            raw = out.raw
            outs = [raw[i * block_size:i * block_size + len(c)] for i, c in enumerate(ctexts)]
        return outs
    for i, (r, c) in enumerate(zip(refs, ctexts)):
        c = bytes(c)
        if len(c) == 0:
            status = _empty_status(r, salt, cid_key)
            if status:
                raise ErrCorrupt(i, r.cid, status)
            outs.append(b"")
            continue
        out = ctypes.create_string_buffer(len(c)) if want_ptext else None
        bad = _open_call(salt, cid_key, c, len(c), -(-len(c) // 64) * 64, r.marshal_binary(), out)
        if bad:
            raise ErrCorrupt(i, r.cid, bad[1])
        if want_ptext:
            outs.append(out.raw)
    return outs if want_ptext else []


def open_blobs(ctexts, refs, salt: Optional[bytes], cid_key: Optional[bytes] = None,
               want_ptext: bool = True):
    """open_level's checks over blobs of any mix of lengths (each at most
    16 MiB, the empty one included) in ONE glfsx_open_blobs call: salt is the
    level's salt as post took it (None: no DEK check), the same for every
    blob.  Returns (ptexts, statuses): the plaintexts in order (an empty list
    when want_ptext is false) and a status word per blob -- GLFSX_BAD_CID |
    GLFSX_BAD_DEK, 0 for a good one.  Never raises for a bad blob; the
    plaintext of a bad blob is not to be used."""
    n = len(ctexts)
    if n == 0:
        return [], []
    lens = [len(c) for c in ctexts]
    offs, pos = [], 0
    for ln in lens:
        offs.append(pos)
        pos += ln
    data = b"".join(bytes(c) for c in ctexts)
    rb = b"".join(r.marshal_binary() for r in refs)
    if len(rb) != REF_SIZE * n:
        raise ValueError("open_blobs needs one ref per ctext")
    out = ctypes.create_string_buffer(max(pos, 1)) if want_ptext else None
    st = (ctypes.c_uint32 * n)()
    rc = N.lib.glfsx_open_blobs(_salt_arg(salt), cid_key, data or b"\0",
                                (ctypes.c_uint64 * n)(*offs), (ctypes.c_uint64 * n)(*lens), n,
                                rb, out, st, None)
    if rc != N.GLFSX_E_CORRUPT:
        N.check(rc)
    ptexts = []
    if want_ptext:
        raw = out.raw
        ptexts = [raw[o:o + ln] for o, ln in zip(offs, lens)]
    return ptexts, list(st)


def _tree_levels(get, root: Root, salt: Optional[bytes] = None,
                 cid_key: Optional[bytes] = None, *, _check: bool = False,
                 _keep: Optional[dict] = None) -> list:
    """The refs of every level of root's tree, top (the root) first, data
    blocks last: each index level is fetched with get(cid) and decrypted in
    one batch (blob.go:53-69 getPiece's walk, level by level).  With a salt
    (the blob's, as Create took it) or a cid_key the index nodes go through
    open_level -- CID checked, and DEK under DeriveKey(salt, "index") when
    the salt is given -- and a bad node raises ErrCorrupt with its level;
    with neither, nothing is checked.  (_check: check CIDs even with neither;
    _keep: a dict that receives cid -> ctext of every index node.)"""
    bs = root.block_size
    bf = branching_factor(bs)
    lvl = depth(root.size, bs)
    n0 = -(-root.size // bs)
    levels = [[root.ref]]
    checked = _check or salt is not None or cid_key is not None
    index_salt = derive_key(salt, b"index") if salt is not None and lvl > 0 else None
    for k in range(lvl, 0, -1):
        refs = levels[-1]
        cts = [get(r.cid) for r in refs]
        if checked:
            try:
                nodes = open_level(cts, refs, bs, index_salt, cid_key)
            except ErrCorrupt as e:
                raise e.at_level(k) from None
        else:
            nodes = decrypt_level(cts, refs, bs)
        if _keep is not None:
            _keep.update((r.cid, c) for r, c in zip(refs, cts))
        want = -(-n0 // bf ** (k - 1))          # refs at level k-1
        child = []
        for node in nodes:
            if len(node) != bf * MAX_REF_SIZE:
                raise ValueError("data is not correct size for index")
            take = min(bf, want - len(child))
            child += [Ref.from_bytes(node[i * 64:(i + 1) * 64]) for i in range(take)]
        levels.append(child)
    return levels


def read_all(store, root: Root, salt: Optional[bytes] = None,
             cid_key: Optional[bytes] = None) -> bytes:
    """Read side (blob.go:31-69 ReadAt/getPiece, ref.go:113-126 getF) of a
    whole blob: the index levels and then all data blocks, each level one
    batched GPU decrypt (the data level straight into the output buffer).
    With the blob's salt (or the store's cid_key) every blob on the way is
    checked as it is decrypted (index levels: open_level; the data level:
    glfsx_open_batch under DeriveKey(salt, "raw")) and corrupt bytes raise
    ErrCorrupt instead of being returned; with neither, nothing is checked."""
    checked = salt is not None or cid_key is not None
    if root.size == 0:
        if checked:
            _check_empty(root.ref, salt, cid_key)
        return b""
    bs = root.block_size
    data_refs = _tree_levels(store.get, root, salt, cid_key)[-1]
    raw = derive_key(salt, b"raw") if salt is not None else None
    if bs % 64:
        if checked:
            return b"".join(open_level([store.get(r.cid) for r in data_refs], data_refs, bs,
                                       raw, cid_key))
        return b"".join(crypto_xor(r.dek, store.get(r.cid)) for r in data_refs)
    ct = _gather(store, data_refs, root.size)
    out = bytearray(root.size)
    rb = b"".join(r.marshal_binary() for r in data_refs)
    obuf = (ctypes.c_char * len(out)).from_buffer(out)
    try:
        if checked:
            bad = _open_call(raw, cid_key, ct.ctypes.data, len(ct), bs, rb, obuf)
            if bad:
                raise ErrCorrupt(bad[0], data_refs[bad[0]].cid, bad[1], 0)
        else:
            N.check(N.lib.glfsx_decrypt_batch(ct.ctypes.data, len(ct), bs, rb, obuf))
    finally:
        del obuf
    return bytes(out)
