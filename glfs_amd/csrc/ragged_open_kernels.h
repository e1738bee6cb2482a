// ragged_open_kernels.h -- the verified read over messages of unequal length
// in throughput form: ROArgs, the chunk pass (rag_open_chunk, k_rag_open_chunk)
// and the two merge levels (k_rag_open_merge_a, k_rag_open_merge_b).
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

// k_open's checks (open_kernels.h) in the ragged post's structure
// (ragged_kernels.h): the plan is the post's own (k_rag_count / k_rag_prefix
// with lo = ~0, so every message of at most hi bytes is selected; with MARK
// the count kernel gives every other message the status GLFSX_BAD_CID), the
// work is handed out by flattened chunk, and every hand-off is a kernel
// boundary on the stream:
//   k_rag_open_chunk    one lane per chunk: one pass over the chunk's ctext,
//                       both chains; a one-chunk message is finished here
//                       (ROOT on both chains, the whole status word), every
//                       other chunk's two CVs go to cvs, 64 B per chunk (CID
//                       then DEK);
//   k_rag_open_merge_a  one workgroup per group of 256 consecutive chunks of
//                       a message: its CID tree, then its DEK tree over the
//                       same LDS; ROOT, the compare with the ref and the
//                       status word here for a message of at most 256 chunks,
//                       else both group CVs go to gcv, 64 B per group;
//   k_rag_open_merge_b  one workgroup per message of more than 256 chunks:
//                       its <= 64 group CVs of each tree, ROOT, compare,
//                       status.
// Exactly one thread writes a message's status word, whole: no atomics and no
// pre-zeroing.  MODE: 2 = both chains (salted; ptext nullable), 1 = the CID
// chain and the keystream (no salt, ptext set: bit 1 is never set), 0 = the
// CID chain alone (no salt, no ptext).
struct ROArgs {
  RArgs r;  // src: the ctext; ctext: the ptext (nullable, may be src); key,
            // base: the CID's; refs: read only; cvs, gcv: 16 words per item
  uint32_t salt[8];
  uint32_t *status;  // one word per message
};

// One chunk of mode 1 or 0: open_subtree<1>'s block loop without the DEK
// chain (and without the keystream when !KS).
template <bool KS, bool ALIGNED, int A>
__device__ __forceinline__ void rag_open_cid_chunk(
    uint32_t (&ccv)[8], const uint8_t *cmsg, uint8_t *pmsg, uint64_t len, uint32_t chunk,
    bool whole, const uint32_t (&ckey)[8], uint32_t cbase, const uint32_t (&dek)[8]) {
  const uint64_t coff = uint64_t(chunk) << 10;
  const uint64_t rem = len - coff;
  const uint32_t clen = rem < 1024 ? uint32_t(rem) : 1024u;
  const uint32_t nb = clen ? (clen + 63) >> 6 : 1u;
#pragma unroll
  for (int i = 0; i < 8; ++i) ccv[i] = ckey[i];
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t boff = b << 6;
    const uint32_t avail = clen - boff;
    const uint32_t blen = avail < 64 ? avail : 64u;
    uint32_t m[16];
    load_block<ALIGNED>(m, cmsg + coff + boff, avail);
    uint32_t fl = 0;
    if (b == 0) fl |= kChunkStart;
    if (b + 1 == nb) {
      fl |= kChunkEnd;
      if (whole) fl |= kRoot;
    }
    b3_compress<A>(ccv, m, chunk, 0u, blen, cbase | fl);
    if constexpr (KS) {
      uint32_t x[16];
      chacha_block<A>(x, dek, (chunk << 4) + b);
#pragma unroll
      for (int i = 0; i < 16; ++i) m[i] ^= x[i];
      store_block<ALIGNED>(pmsg + coff + boff, m, avail);  // no byte past avail
    }
  }
}

// Flattened chunk x for the calling lane (nothing when x >= a.r.total), as
// rag_chunk: every load and store inside the chunk's own bytes of
// [off, off + len).
template <int MODE, int A>
__device__ __forceinline__ void rag_open_chunk(const ROArgs &a, uint64_t x) {
  if (x >= a.r.total) return;
  uint64_t i, cb;
  rag_find<0>(a.r, x, i, cb);
  const uint32_t k = uint32_t(x - cb);  // the chunk's number in its message
  const uint64_t off = a.r.offs[i], len = a.r.lens[i];
  const uint32_t C = rag_chunks(len);
  const uint8_t *cmsg = a.r.src + off;
  uint8_t *pmsg = (MODE > 0 && a.r.ctext) ? a.r.ctext + off : nullptr;
  const uint8_t *ref = a.r.refs + i * 64;
  uint32_t ckey[8], salt[8], dek[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    ckey[w] = a.r.key[w];
    salt[w] = a.salt[w];
  }
  if constexpr (MODE > 0) {
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(ref + 32);
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = dp[w];
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = 0;
  }
  const bool aligned = ((reinterpret_cast<uintptr_t>(cmsg) |
                         reinterpret_cast<uintptr_t>(pmsg)) & 15) == 0;
  uint32_t ccv[8], dcv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (MODE == 2) {
    if (aligned)
      open_subtree<1, true, A>(ccv, dcv, cmsg, pmsg, len, k, 1u, C == 1, ckey, a.r.base, salt,
                               dek);
    else
      open_subtree<1, false, A>(ccv, dcv, cmsg, pmsg, len, k, 1u, C == 1, ckey, a.r.base, salt,
                                dek);
  } else {
    if (aligned)
      rag_open_cid_chunk<MODE == 1, true, A>(ccv, cmsg, pmsg, len, k, C == 1, ckey, a.r.base,
                                             dek);
    else
      rag_open_cid_chunk<MODE == 1, false, A>(ccv, cmsg, pmsg, len, k, C == 1, ckey, a.r.base,
                                              dek);
  }
  if (C == 1) {
    uint32_t st = digest_differs(ccv, ref);
    if constexpr (MODE == 2) st |= digest_differs(dcv, ref + 32) << 1;
    a.status[i] = st;
  } else {
    uint4 *q = reinterpret_cast<uint4 *>(a.r.cvs + x * 16);
    q[0] = make_uint4(ccv[0], ccv[1], ccv[2], ccv[3]);
    q[1] = make_uint4(ccv[4], ccv[5], ccv[6], ccv[7]);
    if constexpr (MODE == 2) {
      q[2] = make_uint4(dcv[0], dcv[1], dcv[2], dcv[3]);
      q[3] = make_uint4(dcv[4], dcv[5], dcv[6], dcv[7]);
    }
  }
}

template <int MODE, int A>
__global__ __launch_bounds__(256) void k_rag_open_chunk(ROArgs a) {
  const uint64_t tiles = (a.r.total + 255) >> 8;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)  // uniform
    rag_open_chunk<MODE, A>(a, (tile << 8) | threadIdx.x);
}

// The tree of the cnt (<= 256) CVs at src + 16 t words (t < cnt) over lds;
// on return thread 0 holds its top in p.  Ends with the barrier that lets
// the next tree, or the next item, rewrite lds.
__device__ __forceinline__ void rag_open_tree(uint32_t *lds, const uint32_t *src, uint32_t cnt,
                                              uint32_t t, const uint32_t (&key)[8],
                                              uint32_t base, bool root, uint32_t (&p)[8]) {
  if (t < cnt) {
    const uint4 *q = reinterpret_cast<const uint4 *>(src + uint64_t(t) * 16);
    const uint4 v0 = q[0], v1 = q[1];
    lds[t * 8 + 0] = v0.x; lds[t * 8 + 1] = v0.y; lds[t * 8 + 2] = v0.z; lds[t * 8 + 3] = v0.w;
    lds[t * 8 + 4] = v1.x; lds[t * 8 + 5] = v1.y; lds[t * 8 + 6] = v1.z; lds[t * 8 + 7] = v1.w;
  }
  __syncthreads();
  tree_reduce_q(lds, cnt, t, key, base, root, p);
  __syncthreads();  // thread 0 has read the top
}

// Thread 0 of the workgroup that reached ROOT: the whole status word, or both
// CVs to the 64-B slot at dst.
template <bool DEK>
__device__ __forceinline__ void rag_open_finish(const ROArgs &a, uint64_t i, bool root,
                                                const uint32_t (&c)[8], const uint32_t (&d)[8],
                                                uint32_t *dst) {
  if (root) {
    const uint8_t *ref = a.r.refs + i * 64;
    uint32_t st = digest_differs(c, ref);
    if constexpr (DEK) st |= digest_differs(d, ref + 32) << 1;
    a.status[i] = st;
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) dst[w] = c[w];
    if constexpr (DEK) {
#pragma unroll
      for (int w = 0; w < 8; ++w) dst[8 + w] = d[w];
    }
  }
}

// Merge level A: workgroup g merges group g's <= 256 chunk CVs of each tree.
template <bool DEK>
__global__ __launch_bounds__(256) void k_rag_open_merge_a(ROArgs a) {
  __shared__ uint32_t lds[256 * 8];
  const uint32_t t = threadIdx.x;
  uint32_t ckey[8], salt[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    ckey[w] = a.r.key[w];
    salt[w] = a.salt[w];
  }
  for (uint64_t g = blockIdx.x; g < a.r.total; g += gridDim.x) {  // uniform
    uint64_t i, gb;
    rag_find<1>(a.r, g, i, gb);
    const uint32_t C = rag_chunks(a.r.lens[i]);
    const uint32_t c0 = uint32_t(g - gb) * 256u;
    const uint32_t cnt = min(256u, C - c0);
    const uint32_t *src = a.r.cvs + (rag_base<0>(a.r, i) + c0) * 16;
    const bool root = C <= 256u;
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0}, d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rag_open_tree(lds, src, cnt, t, ckey, a.r.base, root, c);
    if constexpr (DEK) rag_open_tree(lds, src + 8, cnt, t, salt, kKeyed, root, d);
    if (t == 0) rag_open_finish<DEK>(a, i, root, c, d, a.r.gcv + g * 16);
  }
}

// Merge level B: workgroup b merges the <= 64 group CVs of each tree of the
// b-th message of more than 256 chunks.
template <bool DEK>
__global__ __launch_bounds__(256) void k_rag_open_merge_b(ROArgs a) {
  __shared__ uint32_t lds[256 * 8];
  const uint32_t t = threadIdx.x;
  uint32_t ckey[8], salt[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    ckey[w] = a.r.key[w];
    salt[w] = a.salt[w];
  }
  for (uint64_t b = blockIdx.x; b < a.r.total; b += gridDim.x) {  // uniform
    uint64_t i, bb;
    rag_find<2>(a.r, b, i, bb);
    const uint32_t C = rag_chunks(a.r.lens[i]);
    const uint32_t ng = (C + 255u) >> 8;  // <= 64 (kMaxRaggedLen)
    const uint32_t *src = a.r.gcv + rag_base<1>(a.r, i) * 16;
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0}, d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rag_open_tree(lds, src, ng, t, ckey, a.r.base, true, c);
    if constexpr (DEK) rag_open_tree(lds, src + 8, ng, t, salt, kKeyed, true, d);
    if (t == 0) rag_open_finish<DEK>(a, i, true, c, d, nullptr);
  }
}
