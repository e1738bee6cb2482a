// open_kernels.h -- the verified read: k_open (CID check, decrypt and DEK
// check of a block in one pass over its ctext) and k_open_compare (the last
// step of the composed route).
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

// Read side with the checks content addressing gives (bigblob/ref.go:113-126
// getF; blob.go:307-315 copyBlob's dst.Post re-hash): block j of n is intact
// iff BLAKE3(ctext_j) == refs[j][0:32] (keyed when the store is keyed), and
// its ref matches its plaintext iff
//   keyed-BLAKE3(salt, ChaCha20(refs[j][32:64]) ^ ctext_j) == refs[j][32:64].
// The inverse of the write path's two passes; the DEK is known up front, so
// one pass reads each 64-B block once, compresses it into the CID chain,
// XORs the keystream, compresses the result into the DEK chain and stores
// the plaintext once.
struct OArgs {
  const uint8_t *ctext;
  uint8_t *ptext;       // nullable (no stores); may equal ctext
  uint64_t n, bs, last_len;
  const uint8_t *refs;  // dense, 64 B per block, 4-B aligned
  uint32_t *status;     // one word per block: bit 0 CID, bit 1 DEK mismatch
  uint32_t salt[8];
  uint32_t cid_key[8];
  uint32_t cid_base;    // kKeyed or 0
};

// One full 64-B block of k_open with the ctext words in m: the CID chain
// takes them as loaded, the DEK chain after the keystream; m leaves as
// plaintext.
template <int A>
__device__ __forceinline__ void open_block(uint32_t (&ccv)[8], uint32_t (&dcv)[8],
                                           uint32_t (&m)[16], uint32_t chunk, uint32_t b,
                                           uint32_t cfl, uint32_t dfl,
                                           const uint32_t (&dek)[8]) {
  b3_compress<A>(ccv, m, chunk, 0u, 64u, cfl);
  {
    uint32_t x[16];
    chacha_block<A>(x, dek, (chunk << 4) + b);
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] ^= x[i];
  }
  b3_compress<A>(dcv, m, chunk, 0u, 64u, dfl);
}

// Fast path (as lane_subtree_full<G, true, true>): the lane's G chunks are
// full, the pointers 16-B aligned and the whole wave is here.  The ctext
// arrives by buffer_load ... lds into the wave's swizzled 8 KiB image
// (sbase), one pair of 64-B blocks per lane and step; the lane takes its pair
// out block by block, writes the plaintext back into the same slots, the
// wave stores 8 whole 128-B lines per instruction, and the next pair is
// issued after the stores (the image is shared by landing and leaving data).
// pmsg == nullptr: no write-back and no stores.  Never `whole`: a block of
// at most G chunks leaves lanes 1.. of its wave without chunks.
template <int G, int A>
__device__ __forceinline__ void open_subtree_full(
    uint32_t (&ccv)[8], uint32_t (&dcv)[8], const uint8_t *cmsg, uint8_t *pmsg,
    uint32_t first, const uint32_t (&ckey)[8], uint32_t cbase,
    const uint32_t (&salt)[8], const uint32_t (&dek)[8], uint32_t sbase, uint32_t len) {
  constexpr int D = ilog2(G);
  constexpr uint32_t NB = 16u * G;
  uint32_t cstk[D > 0 ? D : 1][8], dstk[D > 0 ? D : 1][8];
  uint32_t cdepth = 0, ddepth = 0;
  const uint32_t l = threadIdx.x & 63u, r = l >> 3, pc = l & 7u;
  const uint32_t wa = sbase + (l << 7) + (img_swz(l) << 4);
  const uint32_t rb = sbase + (r << 7) + ((pc ^ img_swz(r)) << 4);
  // voffset of (line r of this wave's 8-line group 0, piece pc): lane l's
  // data starts at chunk `first` of the block and lane 0's at first - l*G
  const uint32_t vo = ((first + (r - l) * uint32_t(G)) << 10) + (pc << 4);
  // wave-uniform descriptors over the block: every line of a fast wave lies
  // inside [0, len)
  const __amdgpu_buffer_rsrc_t rsrc_st =
      __builtin_amdgcn_make_buffer_rsrc(pmsg, 0, pmsg ? len : 0u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_ld = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t *>(cmsg), 0, len, 0x00020000);
  const uint32_t sb = __builtin_amdgcn_readfirstlane(sbase);
  const uint32_t lo0 = vo - (pc << 4) + ((pc ^ img_swz(r)) << 4);
  auto issue = [&](uint32_t s) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsrc_ld, (__attribute__((address_space(3))) void *)(uintptr_t)(sb + 1024u * k),
          16, (k & 1) ? (lo0 ^ 64u) : lo0, ((8u * k * uint32_t(G)) << 10) + 128u * s,
          0, 0);
  };
  issue(0);
  for (uint32_t jj = 0; jj < uint32_t(G); ++jj) {
    const uint32_t chunk = first + jj;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ccv[i] = ckey[i];
      dcv[i] = salt[i];
    }
    for (uint32_t pp = 0; pp < 8; ++pp) {
      const uint32_t blk = jj * 16 + 2 * pp;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this pair has landed
#pragma unroll
      for (uint32_t half = 0; half < 2; ++half) {
        const uint32_t w = opaque(wa);
        u32x4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          v[i] = *reinterpret_cast<const lds_u32x4 *>(w ^ ((4u * half + uint32_t(i)) << 4));
        uint32_t m[16] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                          v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w};
        uint32_t fl = 0;
        if (half == 0 && pp == 0) fl |= kChunkStart;
        if (half == 1 && pp == 7) fl |= kChunkEnd;
        open_block<A>(ccv, dcv, m, chunk, 2 * pp + half, cbase | fl, kKeyed | fl, dek);
        if (pmsg) stage_half(wa, half, m);  // wave-uniform
      }
      if (pmsg) {
        // lane l stores piece pc of line 8k + r (see lane_subtree_full)
        const uint32_t r0 = opaque(rb), r1 = r0 ^ 64u, v0 = vo + blk * 64u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const u32x4 v = *reinterpret_cast<const lds_u32x4 *>(
              ((k & 1) ? r1 : r0) + 1024u * k);
          __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_st, v0,
              (8u * k * uint32_t(G)) << 10, 0);
        }
      }
      if (blk + 2 < NB) {  // the image is free again: next pair
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        issue(blk / 2 + 1);
      }
    }
    const bool last = jj + 1 == uint32_t(G);
    lane_merge<D, A>(ccv, cstk, cdepth, jj, last, false, ckey, cbase);
    lane_merge<D, A>(dcv, dstk, ddepth, jj, last, false, salt, kKeyed);
  }
}

// Generic path (as lane_subtree): a ragged tail chunk, a partial last 64-B
// block, unaligned pointers.  The CID chain takes the block zero-filled with
// block_len = avail; the plaintext words are masked beyond avail before the
// DEK compression and the store, which writes no byte past the block.
template <int G, bool ALIGNED, int A>
__device__ __forceinline__ void open_subtree(
    uint32_t (&ccv)[8], uint32_t (&dcv)[8], const uint8_t *cmsg, uint8_t *pmsg,
    uint64_t len, uint32_t first, uint32_t n_my, bool whole,
    const uint32_t (&ckey)[8], uint32_t cbase, const uint32_t (&salt)[8],
    const uint32_t (&dek)[8]) {
  constexpr int D = ilog2(G);
  uint32_t cstk[D > 0 ? D : 1][8], dstk[D > 0 ? D : 1][8];
  uint32_t cdepth = 0, ddepth = 0;
  for (uint32_t jj = 0; jj < n_my; ++jj) {
    const uint32_t chunk = first + jj;
    const uint64_t coff = uint64_t(chunk) << 10;
    const uint64_t rem = len - coff;
    const uint32_t clen = rem < 1024 ? uint32_t(rem) : 1024u;
    const uint32_t nb = clen ? (clen + 63) >> 6 : 1u;
    const bool last = jj + 1 == n_my;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ccv[i] = ckey[i];
      dcv[i] = salt[i];
    }
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
        if (whole && n_my == 1) fl |= kRoot;
      }
      b3_compress<A>(ccv, m, chunk, 0u, blen, cbase | fl);
      {
        uint32_t x[16];
        chacha_block<A>(x, dek, (chunk << 4) + b);
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] ^= x[i];
      }
      if (avail < 64) mask_tail(m, avail);
      if (pmsg) store_block<ALIGNED>(pmsg + coff + boff, m, avail);
      b3_compress<A>(dcv, m, chunk, 0u, blen, kKeyed | fl);
    }
    lane_merge<D, A>(ccv, cstk, cdepth, jj, last, whole, ckey, cbase);
    lane_merge<D, A>(dcv, dstk, ddepth, jj, last, whole, salt, kKeyed);
  }
}

// 1 when the 8 words differ from the 32 bytes at p (4-B aligned).
__device__ __forceinline__ uint32_t digest_differs(const uint32_t (&w)[8], const uint8_t *p) {
  const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= w[i] ^ q[i];
  return d ? 1u : 0u;
}

// One 256-lane workgroup per block (of at most 256 G chunks), lane t owning
// chunks [tG, tG + G) as in k_pass with split_log2 == 0; each lane carries
// the CID and the DEK chaining values and their stacks, and the workgroup
// merges the two trees one after the other over the same LDS area.  LDS as
// k_pass: [0, 8 KiB) CV tree, then 4 waves x 8 KiB of staging -- 40 KiB, so
// four workgroups per CU need at most 128 VGPRs: G <= 4 is held to that
// (G = 4 took 129 unasked and fits 128 without a spill); G = 8, with two
// three-deep CV stacks, takes 145 and runs three per CU.
template <int G, bool ALIGNED, int A = 2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(G <= 4 ? 4 : 3)))
void k_open(OArgs a) {
  __shared__ uint4 lds_u4[512 + kStage];
  uint32_t *lds = reinterpret_cast<uint32_t *>(lds_u4);
  const uint64_t j = blockIdx.x;
  const uint64_t len = (j + 1 == a.n) ? a.last_len : a.bs;
  const uint8_t *cmsg = a.ctext + j * a.bs;
  uint8_t *pmsg = a.ptext ? a.ptext + j * a.bs : nullptr;
  const uint8_t *ref = a.refs + j * 64;
  const uint32_t t = threadIdx.x;

  uint32_t ckey[8], salt[8], dek[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ckey[i] = a.cid_key[i];
    salt[i] = a.salt[i];
    dek[i] = __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t *>(ref + 32)[i]);
  }
  const uint32_t C = len ? uint32_t((len + 1023) >> 10) : 1u;
  const bool whole = C <= uint32_t(G);
  const uint32_t first = t * G;
  const uint32_t n_my = first < C ? min(uint32_t(G), C - first) : 0u;
  uint32_t ccv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dcv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool fast = ALIGNED && n_my == uint32_t(G) && len >= (uint64_t(first) + G) << 10;
  // staged stores write other lanes' lines: only when the whole wave is fast
  const bool wave_fast = ALIGNED && __ballot(fast) == ~0ull;
  if (wave_fast) {
    if constexpr (ALIGNED)
      open_subtree_full<G, A>(ccv, dcv, cmsg, pmsg, first, ckey, a.cid_base, salt, dek,
                              lds_offset(lds_u4 + 512 + (t >> 6) * 512), uint32_t(len));
  } else if (n_my) {
    open_subtree<G, ALIGNED, A>(ccv, dcv, cmsg, pmsg, len, first, n_my, whole, ckey,
                                a.cid_base, salt, dek);
  }
  uint32_t st = 0;
  if (!whole) {  // uniform: depends on len only
    const uint32_t active = (C + G - 1) / G;
    if (t < active) {
#pragma unroll
      for (int i = 0; i < 8; ++i) lds[t * 8 + i] = ccv[i];
    }
    __syncthreads();
    tree_merge(lds, active, t, ckey, a.cid_base, true, ccv);
    if (t == 0) st = digest_differs(ccv, ref);
    __syncthreads();  // thread 0 has read the CID root
    if (t < active) {
#pragma unroll
      for (int i = 0; i < 8; ++i) lds[t * 8 + i] = dcv[i];
    }
    __syncthreads();
    tree_merge(lds, active, t, salt, kKeyed, true, dcv);
  } else if (t == 0) {  // lane 0 holds both root outputs
    st = digest_differs(ccv, ref);
  }
  if (t == 0) a.status[j] = st | (digest_differs(dcv, ref + 32) << 1);
}

// The composed route's last step: got[j] = CID || DEK as recomputed by the
// passes (64 B per block), refs[j] as claimed.
__global__ __launch_bounds__(256) void k_open_compare(const uint8_t *got, const uint8_t *refs,
                                                      uint32_t *status, uint64_t n,
                                                      uint32_t salted) {
  const uint64_t j = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x;
  if (j >= n) return;
  const uint32_t *g = reinterpret_cast<const uint32_t *>(got + j * 64);
  const uint32_t *r = reinterpret_cast<const uint32_t *>(refs + j * 64);
  uint32_t dc = 0, dd = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    dc |= g[i] ^ r[i];
    dd |= g[8 + i] ^ r[8 + i];
  }
  status[j] = (dc ? 1u : 0u) | ((salted && dd) ? 2u : 0u);
}
