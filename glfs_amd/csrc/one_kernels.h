// one_kernels.h -- one-shot posts, a whole message per workgroup (one_*,
// k_one, k_one_v) or per few workgroups (med_*, k_med_dek, k_med_cid and
// their by-value forms).
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

// ---- One-shot posts: a whole message of <= kMaxOneLen bytes per workgroup ----
// The message is staged once into LDS (zero padded to 64 B), then
//   DEK  : quad i hashes chunk i from the image (k_quad's quad layout, the
//          16 blocks' LDS addresses are immediates), the quads' CVs merge
//          pairwise through `tslot` (left-complete tree, ROOT at the top);
//   ctext: lane t makes keystream block t (+ k * lanes) with the DEK and XORs
//          it into the image in place (tail bytes masked: the image past len
//          stays zero, as BLAKE3's last block needs), then stores it out;
//   CID  : the same quad hash over the image, now ctext.
// QUADS = 16 (one wave: messages <= 16 KiB) or 64 (four waves).
// Messages of up to kMaxMedLen bytes span several such workgroups (64 KiB
// each) in two launches, k_med_dek and k_med_cid (below).

// The one-shot image's 16-B granules are swizzled per 1 KiB chunk: granule
// g sits at g ^ ((g >> 6) & 3), i.e. word w of a chunk c's block at word
// w ^ 4 (c & 3) of that block.  The quads of a 32-lane LDS group read the
// same word of their chunks (1 KiB apart, so one bank unswizzled: 4-way at
// 4 KiB, 8-way at 16 KiB and up); swizzled it is 2-way at most.  Every
// access to the image goes through img_g.
__device__ __forceinline__ uint32_t img_g(uint32_t g) { return g ^ ((g >> 6) & 3u); }

// Quad `quad` hashes chunk `quad` of the image (len bytes from the image
// start; chunk counter ctr0 + quad); root: the image is the whole message.
__device__ __forceinline__ void one_chunks(uint32_t &cl, uint32_t &ch, uint32_t img,
                                           uint32_t len, uint32_t ctr0, bool root,
                                           uint32_t kq_lo, uint32_t kq_hi, uint32_t ivq,
                                           uint32_t base, uint32_t q, uint32_t quad,
                                           const uint32_t (&rel)[28]) {
  const uint32_t C = len ? (len + 1023) >> 10 : 1u;
  cl = kq_lo;
  ch = kq_hi;
  if (quad < C) {
    const uint32_t clen = min(len - min(len, quad << 10), 1024u);
    const uint32_t nb = clen ? (clen + 63) >> 6 : 1u;
    // the chunk's 28 word addresses once (opaque to the optimiser, which
    // otherwise rebuilt each from the lane's offset with an add per read);
    // block b's reads carry its 64 b as the instruction offset
    uint32_t addr[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) {
      addr[k] = img + (quad << 10) + (rel[k] ^ (16u * (quad & 3u)));  // (img_g)
      asm volatile("" : "+v"(addr[k]));
    }
    uint32_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = *reinterpret_cast<lds_word>(addr[k]);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      if (uint32_t(b) < nb) {
        const uint32_t blen = min(clen - min(clen, 64u * b), 64u);
        uint32_t fl = base;
        if (b == 0) fl |= kChunkStart;
        if (uint32_t(b) + 1 == nb) {
          fl |= kChunkEnd;
          if (root && C == 1) fl |= kRoot;
        }
        const uint32_t dq = qsel(q, ctr0 + quad, 0u, blen, fl);
        uint32_t ab[28], nxt[4];
#pragma unroll
        for (int k = 0; k < 28; ++k) ab[k] = addr[k] + 64u * b;
        // the next block's round-0 words (this block's again after the last)
        const uint32_t nb_off = uint32_t(b) + 1 < nb ? 64u * (b + 1) : 64u * b;
#pragma unroll
        for (int k = 0; k < 4; ++k) nxt[k] = addr[k] + nb_off;
        quad_compress_m<true>(cl, ch, ivq, dq, ab, m, nxt);
      }
    }
  }
}

// Pairwise merge of the `count` CVs held by quads 0..count-1 (left-complete
// tree) through the parent slots at ts; ROOT on the top parent if root.
// Every thread of the workgroup calls it (count is uniform).
__device__ __forceinline__ void one_tree(uint32_t &cl, uint32_t &ch, uint32_t count,
                                         bool root, uint32_t ts, uint32_t *passbuf,
                                         uint32_t kq_lo, uint32_t kq_hi, uint32_t ivq,
                                         uint32_t base, uint32_t q, uint32_t quad,
                                         const uint32_t (&rel)[28]) {
  while (count > 1) {  // uniform
    const uint32_t half = count >> 1, odd = count & 1u;
    __syncthreads();  // the previous level's slots have been read
    if (quad < count) {
      if (odd && quad == count - 1) {
        passbuf[q] = cl;
        passbuf[4 + q] = ch;
      } else {
        // left child: words 0-7 of the parent's slot, right child: 8-15
        const uint32_t sa = ts + ((quad >> 1) << 6) + ((quad & 1u) << 5) + 4u * q;
        *reinterpret_cast<__attribute__((address_space(3))) uint32_t *>(sa) = cl;
        *reinterpret_cast<__attribute__((address_space(3))) uint32_t *>(sa + 16u) = ch;
      }
    }
    __syncthreads();
    if (quad < half) {
      const uint32_t fl = base | kParent | ((root && count == 2) ? kRoot : 0u);
      cl = kq_lo;
      ch = kq_hi;
      const uint32_t dq = qsel(q, 0u, 0u, 64u, fl);
      uint32_t addr[28];
#pragma unroll
      for (int k = 0; k < 28; ++k) addr[k] = ts + (quad << 6) + rel[k];
      quad_compress(cl, ch, ivq, dq, addr);
    } else if (odd && quad == half) {
      cl = passbuf[q];
      ch = passbuf[4 + q];
    }
    count = half + odd;
  }
}

// BLAKE3 (keyed when base has kKeyed) of the image as a whole message, or as
// the subtree of chunks [ctr0, ctr0 + chunks) when !root.  Result in quad 0:
// lane q holds words q (cl) and 4+q (ch).
__device__ __forceinline__ void one_hash(uint32_t &cl, uint32_t &ch, uint32_t img,
                                         uint32_t ts, uint32_t *passbuf,
                                         uint32_t len, const uint32_t (&key)[8],
                                         uint32_t base, uint32_t q, uint32_t quad,
                                         const uint32_t (&rel)[28], uint32_t ctr0 = 0,
                                         bool root = true) {
  const uint32_t kq_lo = qsel(q, key[0], key[1], key[2], key[3]);
  const uint32_t kq_hi = qsel(q, key[4], key[5], key[6], key[7]);
  const uint32_t ivq = qsel(q, kIV[0], kIV[1], kIV[2], kIV[3]);
  one_chunks(cl, ch, img, len, ctr0, root, kq_lo, kq_hi, ivq, base, q, quad, rel);
  const uint32_t C = len ? (len + 1023) >> 10 : 1u;
  one_tree(cl, ch, C, root, ts, passbuf, kq_lo, kq_hi, ivq, base, q, quad, rel);
}

// Stage bytes [0, len) of a message into the image, zero padded to a whole
// 64-B block (one block when empty): bytes at and past `present` read as
// zero (an index node posted from its refs alone).  dcopy (nullable): the
// staged image is also stored there (the medium path's device copy).
// Every lane's loads are issued before any is waited for: the source is
// the caller's pinned staging, one PCIe round trip (~1.7 us) per wave of
// loads, which a loop that waits per iteration paid 4x at 4 KiB and 16x at
// 16 KiB.  padded <= IT x LANES x 16 B (k_one<16>: 16 KiB, k_one<64> and a
// k_med span: 64 KiB; k_one_open's salted forms have twice the lanes and
// IT = 8).
template <int LANES, int IT = 16>
__device__ __forceinline__ void one_stage(uint4 *img_u4, const uint8_t *src, uint32_t len,
                                          uint32_t present, uint8_t *dcopy) {
  const uint32_t padded = len ? (len + 63) & ~63u : 64u;
  const uint32_t have = min(len, present);
  uint4 v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const uint32_t p = (threadIdx.x + uint32_t(i) * LANES) * 16u;
    v[i] = make_uint4(0, 0, 0, 0);
    if (p + 16u <= have) v[i] = *reinterpret_cast<const uint4 *>(src + p);
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const uint32_t p = (threadIdx.x + uint32_t(i) * LANES) * 16u;
    if (p < padded) {
      if (p < have && p + 16u > have) {  // the one partial granule
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; p + k < have; ++k) w[k >> 2] |= uint32_t(src[p + k]) << (8 * (k & 3));
        v[i] = make_uint4(w[0], w[1], w[2], w[3]);
      }
      img_u4[img_g(p >> 4)] = v[i];
      if (dcopy) *reinterpret_cast<uint4 *>(dcopy + p) = v[i];
    }
  }
}

// ChaCha20 (key dek, block counter kb0 + local block) XOR of the image's
// first len bytes in place; the tail is masked so the image past len stays
// zero.
template <int LANES>
__device__ __forceinline__ void one_xor(uint4 *img_u4, uint32_t len, const uint32_t (&dek)[8],
                                        uint32_t kb0) {
  const uint32_t nks = (len + 63) >> 6;
  for (uint32_t kb = threadIdx.x; kb < nks; kb += LANES) {
    uint32_t x[16];
    chacha_block<0>(x, dek, kb0 + kb);
    const uint32_t avail = min(len - kb * 64u, 64u);
    if (avail < 64) mask_tail(x, avail);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint4 v = img_u4[img_g(kb * 4 + i)];
      v.x ^= x[4 * i];
      v.y ^= x[4 * i + 1];
      v.z ^= x[4 * i + 2];
      v.w ^= x[4 * i + 3];
      img_u4[img_g(kb * 4 + i)] = v;
    }
  }
}

// Store the image's first len bytes to dst (16-B aligned).
template <int LANES>
__device__ __forceinline__ void one_store(const uint4 *img_u4, uint8_t *dst, uint32_t len) {
  for (uint32_t p = threadIdx.x * 16u; p < len; p += LANES * 16u) {
    const uint4 v = img_u4[img_g(p >> 4)];
    if (p + 16u <= len) {
      *reinterpret_cast<uint4 *>(dst + p) = v;
    } else {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      for (uint32_t i = 0; p + i < len; ++i) dst[p + i] = uint8_t(w[i >> 2] >> (8 * (i & 3)));
    }
  }
}

// The descriptor, staged into LDS by one load per word, all issued at once
// (round 6).  It lives in pinned host memory, and reading its fields where
// they are used made each group of them a PCIe round trip (~1.7 us) on the
// post's critical path: round 5's k_one waited for the salt words after the
// message, then for the CID key, the output pointers, the flag and the
// sequence number (s_load ... s_waitcnt pairs in the code object).
// D: OneDesc, or k_one_open's OneOpenDesc.
template <class D>
__device__ __forceinline__ const D *one_desc(D *s, const D *g) {
  constexpr uint32_t kW = sizeof(D) / 4;
  static_assert(sizeof(D) % 4 == 0 && kW <= 64, "wave 0 stages the descriptor");
  if (threadIdx.x < kW)
    reinterpret_cast<uint32_t *>(s)[threadIdx.x] =
        reinterpret_cast<const uint32_t *>(g)[threadIdx.x];
  __syncthreads();
  return s;
}

// The post's results (ctext, ref) are in the caller's staging: every lane's
// stores are done, then one release store of the descriptor's sequence
// number into its flag (pinned host memory) tells the waiting caller, with
// no stream query (OneDesc::flag; nullable).
template <class D>
__device__ __forceinline__ void one_signal(const D *dp) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && dp->flag)
    __hip_atomic_store(dp->flag, dp->seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Phase timing of k_one (A/B variant builds only: GLFSX_ONE_TIMING=1,
// scripts/one_trace.py): workgroup 0 adds s_memrealtime ticks since its
// start at each phase boundary.
#if GLFSX_ONE_TIMING
__device__ unsigned long long g_one_t[16];
#define ONE_T(i)                                                                        \
  do {                                                                                  \
    if (blockIdx.x == 0 && threadIdx.x == 0)                                            \
      __hip_atomic_fetch_add(&g_one_t[i],                                               \
                             (unsigned long long)(__builtin_amdgcn_s_memrealtime() - t0), \
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);               \
  } while (0)
#else
#define ONE_T(i) \
  do {           \
  } while (0)
#endif

// The body of a one-shot post (k_one, k_one_v).  V: dp is the descriptor
// itself (a kernel argument); otherwise the launch's array in pinned host
// memory, staged by one_desc.
template <int QUADS, bool V>
__device__ __forceinline__ void one_run(const OneDesc *g) {
#if GLFSX_ONE_TIMING
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
#endif
  __shared__ uint4 img_u4[QUADS * 64];       // the message, then its ctext
  __shared__ uint4 ts_u4[QUADS / 2 * 4];     // parent inputs of the merge
  __shared__ uint32_t passbuf[8];
  __shared__ uint32_t s_dek[8];
  constexpr int kLanes = QUADS * 4;
  const OneDesc *dp;
  if constexpr (V) {
    dp = g;
  } else {
    __shared__ OneDesc s_desc;
    dp = one_desc(&s_desc, g + blockIdx.x);
  }
  const uint32_t len = dp->len;
  const uint32_t tid = threadIdx.x, q = tid & 3u, quad = tid >> 2;
  const uint32_t img = lds_offset(img_u4), ts = lds_offset(ts_u4);
  ONE_T(0);
  one_stage<kLanes>(img_u4, dp->src, len, dp->present, nullptr);
  uint32_t rel[28];
  quad_addrs(rel, 0u, q);
  __syncthreads();
  ONE_T(1);
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = dp->salt[i];
  uint32_t cl, ch;
#if GLFSX_ONE_TIMING  // one_hash with a stamp between its chunks and its merges
  {
    const uint32_t kq_lo = qsel(q, key[0], key[1], key[2], key[3]);
    const uint32_t kq_hi = qsel(q, key[4], key[5], key[6], key[7]);
    const uint32_t ivq = qsel(q, kIV[0], kIV[1], kIV[2], kIV[3]);
    one_chunks(cl, ch, img, len, 0u, true, kq_lo, kq_hi, ivq, kKeyed, q, quad, rel);
    ONE_T(6);
    one_tree(cl, ch, len ? (len + 1023) >> 10 : 1u, true, ts, passbuf, kq_lo, kq_hi, ivq,
             kKeyed, q, quad, rel);
  }
#else
  one_hash(cl, ch, img, ts, passbuf, len, key, kKeyed, q, quad, rel);
#endif
  if (quad == 0) {  // lanes 0-3: DEK words q and 4+q
    s_dek[q] = cl;
    s_dek[4 + q] = ch;
  }
  __syncthreads();
  ONE_T(2);
  uint32_t dek[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) dek[i] = s_dek[i];
  one_xor<kLanes>(img_u4, len, dek, 0u);
  __syncthreads();
  ONE_T(3);
  if (dp->ctext) one_store<kLanes>(img_u4, dp->ctext, len);  // drains during the CID
  uint32_t ckey[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ckey[i] = dp->cid_key[i];
#if GLFSX_ONE_TIMING
  {
    const uint32_t cb = dp->cid_keyed ? kKeyed : 0u;
    const uint32_t kq_lo = qsel(q, ckey[0], ckey[1], ckey[2], ckey[3]);
    const uint32_t kq_hi = qsel(q, ckey[4], ckey[5], ckey[6], ckey[7]);
    const uint32_t ivq = qsel(q, kIV[0], kIV[1], kIV[2], kIV[3]);
    one_chunks(cl, ch, img, len, 0u, true, kq_lo, kq_hi, ivq, cb, q, quad, rel);
    ONE_T(7);
    one_tree(cl, ch, len ? (len + 1023) >> 10 : 1u, true, ts, passbuf, kq_lo, kq_hi, ivq, cb,
             q, quad, rel);
  }
#else
  one_hash(cl, ch, img, ts, passbuf, len, ckey, dp->cid_keyed ? kKeyed : 0u, q, quad, rel);
#endif
  if (quad == 0) {
    uint32_t *r = reinterpret_cast<uint32_t *>(dp->ref);
    r[q] = cl;
    r[4 + q] = ch;
    r[8 + q] = dek[q];
    r[12 + q] = dek[4 + q];
  }
  ONE_T(4);
  one_signal(dp);
  ONE_T(5);
#if GLFSX_ONE_TIMING
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // shader clock over the kernel: [13] / [14]
    const uint64_t c1 = __builtin_amdgcn_s_memtime(), t1 = __builtin_amdgcn_s_memrealtime();
    __hip_atomic_fetch_add(&g_one_t[13], (unsigned long long)(c1 - c0), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&g_one_t[14], (unsigned long long)(t1 - t0), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&g_one_t[15], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#endif
}

template <int QUADS>
__global__ __launch_bounds__(QUADS * 4) void k_one(const OneDesc *descs) {
  one_run<QUADS, false>(descs);
}

// A launch of one post (the common case of a caller posting alone): the
// descriptor travels as the kernel argument, so its fields are read from the
// kernarg segment instead of one PCIe round trip to pinned host memory ahead
// of everything else (round 6).
template <int QUADS>
__global__ __launch_bounds__(QUADS * 4) void k_one_v(const OneDesc d) {
  one_run<QUADS, true>(&d);
}

// ---- Medium one-shot posts (kMaxOneLen < len <= kMaxMedLen) ----
// Workgroup s of a message owns its 64 KiB span s (64 chunks, one per quad).
// k_med_dek stages the span from the caller's staging (pinned host memory)
// into LDS and into the descriptor's device copy, hashes its subtree and
// publishes the CV; the message's last-arriving workgroup merges the W CVs
// (ROOT on top) into the DEK.  k_med_cid reads the span back from the device
// copy, XORs the keystream in, stores the ctext to the caller's staging and
// hashes the CID the same way.  Same cross-XCD protocol as the split passes
// (publish_cv / arrive_last / load_cv_word); the counter is left at zero.
// Grid: n x wmax workgroups; workgroups past a message's span exit at once.
__device__ __forceinline__ void med_publish_merge(uint32_t &cl, uint32_t &ch, const OneDesc *dp,
                                                  uint32_t sidx, uint32_t W, uint32_t ts,
                                                  uint32_t *passbuf, uint32_t *flag,
                                                  const uint32_t (&key)[8], uint32_t base,
                                                  uint32_t q, uint32_t quad,
                                                  const uint32_t (&rel)[28], bool *last) {
  const uint32_t tid = threadIdx.x;
  if (quad == 0) {  // lanes 0-3 of wave 0: one store instruction per word pair
    __hip_atomic_store(dp->cvs + sidx * 8 + q, cl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(dp->cvs + sidx * 8 + 4 + q, ch, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  *last = arrive_last(dp->cnt, W, tid, flag);
  if (!*last) return;
  const uint32_t kq_lo = qsel(q, key[0], key[1], key[2], key[3]);
  const uint32_t kq_hi = qsel(q, key[4], key[5], key[6], key[7]);
  const uint32_t ivq = qsel(q, kIV[0], kIV[1], kIV[2], kIV[3]);
  if (quad < W) {
    cl = load_cv_word(dp->cvs + quad * 8 + q);
    ch = load_cv_word(dp->cvs + quad * 8 + 4 + q);
  }
  one_tree(cl, ch, W, true, ts, passbuf, kq_lo, kq_hi, ivq, base, q, quad, rel);
  if (tid == 0) *dp->cnt = 0;
}

// V: g is the descriptor itself (a kernel argument, one message); else the
// launch's array (as one_run)
template <bool V>
__device__ __forceinline__ void med_dek_run(const OneDesc *g, uint32_t wmax) {
  __shared__ uint4 img_u4[64 * 64];
  __shared__ uint4 ts_u4[32 * 4];
  __shared__ uint32_t passbuf[8];
  __shared__ uint32_t s_flag;
  const OneDesc *dp;
  if constexpr (V) {
    dp = g;
  } else {
    __shared__ OneDesc s_desc;
    dp = one_desc(&s_desc, g + blockIdx.x / wmax);
  }
  const uint32_t sidx = blockIdx.x % wmax;
  const uint32_t len = dp->len;
  const uint32_t W = (len + 65535u) >> 16;
  if (sidx >= W) return;  // uniform: past this message's spans
  const uint32_t off = sidx << 16, slen = min(len - off, 65536u);
  const uint32_t present = dp->present > off ? dp->present - off : 0u;
  const uint32_t tid = threadIdx.x, q = tid & 3u, quad = tid >> 2;
  const uint32_t img = lds_offset(img_u4), ts = lds_offset(ts_u4);
  one_stage<256>(img_u4, dp->src + off, slen, present, dp->dmsg + off);
  uint32_t rel[28];
  quad_addrs(rel, 0u, q);
  __syncthreads();
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = dp->salt[i];
  uint32_t cl, ch;
  one_hash(cl, ch, img, ts, passbuf, slen, key, kKeyed, q, quad, rel, sidx << 6, false);
  bool last;
  med_publish_merge(cl, ch, dp, sidx, W, ts, passbuf, &s_flag, key, kKeyed, q, quad, rel,
                    &last);
  if (last && quad == 0) {
    dp->dek[q] = cl;
    dp->dek[4 + q] = ch;
    uint32_t *r = reinterpret_cast<uint32_t *>(dp->ref);
    r[8 + q] = cl;
    r[12 + q] = ch;
  }
}

template <bool V>
__device__ __forceinline__ void med_cid_run(const OneDesc *g, uint32_t wmax) {
  __shared__ uint4 img_u4[64 * 64];
  __shared__ uint4 ts_u4[32 * 4];
  __shared__ uint32_t passbuf[8];
  __shared__ uint32_t s_flag;
  const OneDesc *dp;
  if constexpr (V) {
    dp = g;
  } else {
    __shared__ OneDesc s_desc;
    dp = one_desc(&s_desc, g + blockIdx.x / wmax);
  }
  const uint32_t sidx = blockIdx.x % wmax;
  const uint32_t len = dp->len;
  const uint32_t W = (len + 65535u) >> 16;
  if (sidx >= W) return;
  const uint32_t off = sidx << 16, slen = min(len - off, 65536u);
  const uint32_t tid = threadIdx.x, q = tid & 3u, quad = tid >> 2;
  const uint32_t img = lds_offset(img_u4), ts = lds_offset(ts_u4);
  // the device copy holds the span zero padded to 64 B (k_med_dek)
  const uint32_t padded = (slen + 63) & ~63u;
  {
    // all loads in flight at once (see one_stage).  Zero-initialised: left
    // partly unassigned, the array stayed in scratch -- each load waited for
    // and spilled before the next was issued (the code object of rounds 5-6)
    uint4 v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t p = (tid + uint32_t(i) * 256u) * 16u;
      v[i] = make_uint4(0, 0, 0, 0);
      if (p < padded) v[i] = *reinterpret_cast<const uint4 *>(dp->dmsg + off + p);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t p = (tid + uint32_t(i) * 256u) * 16u;
      if (p < padded) img_u4[img_g(p >> 4)] = v[i];
    }
  }
  uint32_t dek[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) dek[i] = dp->dek[i];
  uint32_t rel[28];
  quad_addrs(rel, 0u, q);
  __syncthreads();
  one_xor<256>(img_u4, slen, dek, sidx << 10);
  __syncthreads();
  if (dp->ctext) one_store<256>(img_u4, dp->ctext + off, slen);
  uint32_t ckey[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ckey[i] = dp->cid_key[i];
  const uint32_t base = dp->cid_keyed ? kKeyed : 0u;
  uint32_t cl, ch;
  one_hash(cl, ch, img, ts, passbuf, slen, ckey, base, q, quad, rel, sidx << 6, false);
  // this span's ctext is in the caller's staging before the span counts in
  // (the last workgroup signals the caller): the stores are done, and a
  // system-scope release writes back what this XCD's L2 holds of them --
  // the staging may be non-coherent host memory, and the last workgroup's
  // own release covers only its XCD
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0 && dp->flag) __threadfence_system();
  bool last;
  med_publish_merge(cl, ch, dp, sidx, W, ts, passbuf, &s_flag, ckey, base, q, quad, rel,
                    &last);
  if (last && quad == 0) {
    uint32_t *r = reinterpret_cast<uint32_t *>(dp->ref);
    r[q] = cl;
    r[4 + q] = ch;
  }
  if (last) one_signal(dp);
}

__global__ __launch_bounds__(256) void k_med_dek(const OneDesc *descs, uint32_t wmax) {
  med_dek_run<false>(descs, wmax);
}
__global__ __launch_bounds__(256) void k_med_cid(const OneDesc *descs, uint32_t wmax) {
  med_cid_run<false>(descs, wmax);
}
// One medium post, its descriptor as the kernel argument (k_one_v)
__global__ __launch_bounds__(256) void k_med_dek_v(const OneDesc d, uint32_t wmax) {
  med_dek_run<true>(&d, wmax);
}
__global__ __launch_bounds__(256) void k_med_cid_v(const OneDesc d, uint32_t wmax) {
  med_cid_run<true>(&d, wmax);
}
