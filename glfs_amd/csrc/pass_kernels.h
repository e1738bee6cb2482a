// pass_kernels.h -- the bulk passes of the write path: KArgs, split-mode
// publication, lane_merge, the LDS staging image and its swizzle, full_block,
// pair_pipelined, lane_subtree / lane_subtree_full, DcConst / DcState,
// pass_body, and the kernels k_pass and k_pass_dc.
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

constexpr int ilog2(int g) { return g <= 1 ? 0 : 1 + ilog2(g / 2); }

struct KArgs {
  const uint8_t *src;
  uint8_t *ctext;
  uint64_t stride, msg_len, last_len, n;
  uint8_t *refs;
  uint64_t ref_bf, ref_stride;
  uint32_t key[8];
  uint32_t base;     // kKeyed or 0
  uint32_t out_off;  // byte offset of the 32-byte result inside the ref slot
  // split mode (few messages): 2^split_log2 workgroups per message, each over
  // 256*G consecutive chunks; their subtree CVs go to scratch (8 words per
  // workgroup) and the message's last-arriving workgroup (per-message
  // arrival counter in cnt, zero between launches) finishes the tree.
  // split_log2 == 0: one workgroup per message, no scratch.
  uint32_t split_log2;
  uint32_t *scratch;
  uint32_t *cnt;
  // the clock probe's two counters on this launch's device (g_clk), or
  // nullptr: probing is off until the process first calls clock_probe
  unsigned long long *clk;
};

// Split mode: thread 0 publishes this workgroup's subtree CV and counts it
// in; returns true in every thread of the workgroup that arrives last for
// its message, which then merges all W CVs.  The workgroups of a message
// run on different XCDs, whose L2s are not coherent with each other.  An
// agent-scope release fence would write back the whole L2 of the issuing
// XCD per workgroup (measured: +50 us per 1 GiB split pass); instead the CV
// words are agent-scope atomic stores (written through to the coherence
// point), the wave waits for them to complete, and only then increments the
// counter (an agent-scope atomic, performed device-wide); the last
// workgroup reads the CVs with agent-scope atomic loads.
__device__ __forceinline__ void publish_cv(uint32_t *dst, const uint32_t (&cv)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
    __hip_atomic_store(dst + i, cv[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t load_cv_word(const uint32_t *src) {
  return __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool arrive_last(uint32_t *cnt, uint32_t W,
                                            uint32_t t, uint32_t *flag) {
  if (t == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the CV stores are done
    const uint32_t old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
    *flag = old + 1 == W;
  }
  __syncthreads();
  return *flag != 0;
}

// Merge step after the last block of local chunk jj: pop/parent/push on the
// lane's CV stack (eager merges = ctz(jj+1); final merges empty the stack).
template <int D, int A = 2>
__device__ __forceinline__ void lane_merge(uint32_t (&cv)[8],
                                           uint32_t (&stk)[D > 0 ? D : 1][8],
                                           uint32_t &depth, uint32_t jj,
                                           bool last, bool whole,
                                           const uint32_t (&key)[8],
                                           uint32_t base) {
  if constexpr (D > 0) {
    const uint32_t merges = last ? depth : uint32_t(__builtin_ctz(jj + 1));
    for (uint32_t i = 0; i < merges; ++i) {
      uint32_t m[16];
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        m[w] = stk[0][w];
        m[8 + w] = cv[w];
        cv[w] = key[w];
      }
#pragma unroll
      for (int d = 0; d + 1 < D; ++d)
#pragma unroll
        for (int w = 0; w < 8; ++w) stk[d][w] = stk[d + 1][w];
      --depth;
      const uint32_t fl =
          base | kParent | ((whole && last && depth == 0) ? kRoot : 0u);
      b3_compress<A>(cv, m, 0u, 0u, 64u, fl);
    }
    if (!last) {
#pragma unroll
      for (int d = D - 1; d > 0; --d)
#pragma unroll
        for (int w = 0; w < 8; ++w) stk[d][w] = stk[d - 1][w];
#pragma unroll
      for (int w = 0; w < 8; ++w) stk[0][w] = cv[w];
      ++depth;
    }
  }
}

// One full 64-B block of the fast path: (ChaCha20 keystream XOR, ctext
// store,) BLAKE3 compression.
// LDS staging of ctext: each wave owns 64 lines x 128 B; lane c puts 16-B piece p of its current 128-B line at byte
// c*128 + ((p ^ ((c>>1)&7)) << 4) (conflict-free ds_write_b128 in 8-lane
// groups and ds_read_b128 in its 16-lane groups), then the wave stores 8 full
// lines per buffer_store_dwordx4 instead of 64 sixteenths of lines.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;

__device__ __forceinline__ uint32_t lds_offset(const void *p) {
  return uint32_t(reinterpret_cast<uintptr_t>(
      (const __attribute__((address_space(3))) void *)p));
}

// opaque to the optimiser: keeps per-piece addresses from being hoisted
// into 8-16 loop-invariant VGPRs (1 v_xor each instead)
__device__ __forceinline__ uint32_t opaque(uint32_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

// Staging-image swizzle: row L (one lane's pair of blocks, 128 B) keeps its
// 16-B piece p in slot p ^ img_swz(L).  The three access patterns must be
// conflict-free: the lane's own ds_write_b128 (groups of 8 consecutive
// lanes, 32 banks), its ds_read_b128 of its own row, and the store path's
// ds_read_b128 of (row 8k + l/8, piece l%8) (groups of 16 lanes, 64 banks;
// MI355X_MICROARCH.md LDS).  The plainer (L >> 1) & 7 gave pairs of lanes
// the same slot in the write groups: a 2-way conflict on every staged store
// (SQ_LDS_BANK_CONFLICT 8.3 cycles per ds_write_b128).  The store path uses
// img_swz(8k + r) = img_swz(r) ^ ((k & 1) << 2).
__device__ __forceinline__ uint32_t img_swz(uint32_t L) {
  return ((L >> 1) & 3u) | (((L ^ (L >> 3)) & 1u) << 2);
}

template <bool CHACHA, bool STAGE = false, int A = 2>
__device__ __forceinline__ void full_block(uint32_t (&cv)[8], const uint4 &w0,
                                           const uint4 &w1, const uint4 &w2,
                                           const uint4 &w3, uint32_t chunk,
                                           uint32_t b, uint32_t fl,
                                           const uint32_t (&dek)[8],
                                           uint4 *out, uint32_t wa = 0,
                                           uint32_t half = 0) {
  uint32_t m[16] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w,
                    w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
  if constexpr (CHACHA) {
    uint32_t x[16];
    chacha_block<A>(x, dek, (chunk << 4) + b);
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] ^= x[i];
    if (STAGE) {  // LDS staging: wa = this lane's swizzled line address
      wa = opaque(wa);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<lds_u32x4 *>(wa ^ ((4u * half + q) << 4)) =
            u32x4{m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]};
    } else if (out) {
      out[0] = make_uint4(m[0], m[1], m[2], m[3]);
      out[1] = make_uint4(m[4], m[5], m[6], m[7]);
      out[2] = make_uint4(m[8], m[9], m[10], m[11]);
      out[3] = make_uint4(m[12], m[13], m[14], m[15]);
    }
  }
  b3_compress<A>(cv, m, chunk, 0u, 64u, fl);
}

// GLFSX_PIPE: the pair's second keystream block is computed interleaved
// with the first block's compression (two independent ARX streams in one
// region instead of strict phases); same instructions, same results.
#ifndef GLFSX_PIPE
#define GLFSX_PIPE 1
#endif
#define CDR_A(x)                     \
  CQR_A(x[0], x[4], x[8], x[12]);    \
  CQR_A(x[1], x[5], x[9], x[13]);    \
  CQR_A(x[2], x[6], x[10], x[14]);   \
  CQR_A(x[3], x[7], x[11], x[15]);   \
  CQR_A(x[0], x[5], x[10], x[15]);   \
  CQR_A(x[1], x[6], x[11], x[12]);   \
  CQR_A(x[2], x[7], x[8], x[13]);    \
  CQR_A(x[3], x[4], x[9], x[14]);

// one BLAKE3 G and one ChaCha20 quarter-round, step by step (the two
// have the same add / xor-rotate shape): two independent chains per step
#define GQ_A(a, b, c, d, mx, my, e, f, g, h)                  \
  a = add3_a(a, b, (mx)); e = add_a(e, f);                    \
  d = rotr_a<16>(xor_a(d, a)); h = rotr_a<16>(xor_a(h, e));   \
  c = add_a(c, d); g = add_a(g, h);                           \
  b = rotr_a<12>(xor_a(b, c)); f = rotr_a<20>(xor_a(f, g));   \
  a = add3_a(a, b, (my)); e = add_a(e, f);                    \
  d = rotr_a<8>(xor_a(d, a)); h = rotr_a<24>(xor_a(h, e));    \
  c = add_a(c, d); g = add_a(g, h);                           \
  b = rotr_a<7>(xor_a(b, c)); f = rotr_a<25>(xor_a(f, g));

// BLAKE3 round R of v fused with one ChaCha20 double round of x
template <int R>
__device__ __forceinline__ void gq_round(uint32_t (&v)[16], const uint32_t (&m)[16],
                                         uint32_t (&x)[16]) {
  constexpr const int *s = kSched.s[R];
  GQ_A(v[0], v[4], v[8], v[12], m[s[0]], m[s[1]], x[0], x[4], x[8], x[12]);
  GQ_A(v[1], v[5], v[9], v[13], m[s[2]], m[s[3]], x[1], x[5], x[9], x[13]);
  GQ_A(v[2], v[6], v[10], v[14], m[s[4]], m[s[5]], x[2], x[6], x[10], x[14]);
  GQ_A(v[3], v[7], v[11], v[15], m[s[6]], m[s[7]], x[3], x[7], x[11], x[15]);
  GQ_A(v[0], v[5], v[10], v[15], m[s[8]], m[s[9]], x[0], x[5], x[10], x[15]);
  GQ_A(v[1], v[6], v[11], v[12], m[s[10]], m[s[11]], x[1], x[6], x[11], x[12]);
  GQ_A(v[2], v[7], v[8], v[13], m[s[12]], m[s[13]], x[2], x[7], x[8], x[13]);
  GQ_A(v[3], v[4], v[9], v[14], m[s[14]], m[s[15]], x[3], x[4], x[9], x[14]);
}

__device__ __forceinline__ void stage_half(uint32_t wa, uint32_t half,
                                           const uint32_t (&m)[16]) {
  wa = opaque(wa);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<lds_u32x4 *>(wa ^ ((4u * half + q) << 4)) =
        u32x4{m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]};
}

// Both blocks of a pair in the LDS-staged CID pass (asm ARX form):
// ChaCha(a); then BLAKE3(a) interleaved round by round with ChaCha(b);
// then BLAKE3(b).
template <int A>
__device__ __forceinline__ void pair_pipelined(
    uint32_t (&cv)[8], const uint4 &a0, const uint4 &a1, const uint4 &a2,
    const uint4 &a3, const uint4 &b0, const uint4 &b1, const uint4 &b2,
    const uint4 &b3, uint32_t chunk, uint32_t blk, uint32_t fla, uint32_t flb,
    const uint32_t (&dek)[8], uint32_t wa) {
  constexpr uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u,
                     c3 = 0x6b206574u;
  uint32_t m[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w,
                    a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
  const uint32_t ctr_a = (chunk << 4) + blk;
  {
    uint32_t x[16];
    chacha_block<A>(x, dek, ctr_a);
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] ^= x[i];
  }
  stage_half(wa, 0, m);
  // block b's keystream state, round 1 in C (key-only quarter-rounds hoist)
  const uint32_t ctr_b = ctr_a + 1;
  uint32_t x[16] = {c0, c1, c2, c3, dek[0], dek[1], dek[2], dek[3],
                    dek[4], dek[5], dek[6], dek[7], ctr_b, 0u, 0u, 0u};
  CQR(x[0], x[4], x[8], x[12]);
  CQR(x[1], x[5], x[9], x[13]);
  CQR(x[2], x[6], x[10], x[14]);
  CQR(x[3], x[7], x[11], x[15]);
  CQR(x[0], x[5], x[10], x[15]);
  CQR(x[1], x[6], x[11], x[12]);
  CQR(x[2], x[7], x[8], x[13]);
  CQR(x[3], x[4], x[9], x[14]);
  // BLAKE3(a): round 0 alone (C form, IV literals), rounds 1-6 step by
  // step with ChaCha(b)'s double rounds 2-7, then ChaCha(b)'s last three
  uint32_t v[16] = {cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7],
                    kIV[0], kIV[1], kIV[2], kIV[3], chunk, 0u, 64u, fla};
  b3_round<0, true>(v, m);
  if constexpr (A == 2) {
#define GQ_IL(R)                             \
  half_il<false, R, true, true>(v, m, x);    \
  half_il<true, R, true, true>(v, m, x);
    GQ_IL(1) GQ_IL(2) GQ_IL(3) GQ_IL(4) GQ_IL(5) GQ_IL(6)
#undef GQ_IL
    for (int i = 0; i < 3; ++i) {
      half_il<false, 0, false, true>(v, m, x);
      half_il<true, 0, false, true>(v, m, x);
    }
  } else {
    gq_round<1>(v, m, x);
    gq_round<2>(v, m, x);
    gq_round<3>(v, m, x);
    gq_round<4>(v, m, x);
    gq_round<5>(v, m, x);
    gq_round<6>(v, m, x);
    CDR_A(x);
    CDR_A(x);
    CDR_A(x);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) cv[i] = v[i] ^ v[i + 8];
  x[0] += c0;
  x[1] += c1;
  x[2] += c2;
  x[3] += c3;
#pragma unroll
  for (int i = 0; i < 8; ++i) x[4 + i] += dek[i];
  x[12] += ctr_b;
  uint32_t mb[16] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w,
                     b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
#pragma unroll
  for (int i = 0; i < 16; ++i) mb[i] ^= x[i];
  stage_half(wa, 1, mb);
  b3_compress<A>(cv, mb, chunk, 0u, 64u, flb);
}

// Fast path: the lane's G chunks are all full (16*G consecutive 64-B blocks,
// 16-B aligned).  Blocks go in pairs through two named register buffers: the
// odd block's loads are issued before the even block is compressed and the
// next even block's before the odd one, so HBM latency is covered and no
// buffer is copied on the loop back-edge.  Chunk-start / chunk-end flags and
// the chaining-value reset are per-chunk (scalar), not per-block selects.
// cst: bytes the staged ctext stores may write from cmsg (0: none -- the
// stores fall outside the buffer descriptor and are dropped; default: clen).
template <int G, bool CHACHA, bool STAGE = false, int A = 2>
__device__ __forceinline__ void lane_subtree_full(
    uint32_t (&cv)[8], const uint8_t *msg, uint8_t *cmsg, uint32_t first,
    bool whole, const uint32_t (&key)[8], uint32_t base,
    const uint32_t (&dek)[8], uint32_t sbase = 0, uint32_t clen = 0,
    uint32_t cbase = 0, uint32_t cst = ~0u) {
  constexpr int D = ilog2(G);
  constexpr uint32_t NB = 16u * G;
  uint32_t stk[D > 0 ? D : 1][8];
  uint32_t depth = 0;
  const uint4 *q = reinterpret_cast<const uint4 *>(msg + (uint64_t(first) << 10));
  uint4 *cq = cmsg ? reinterpret_cast<uint4 *>(cmsg + (uint64_t(first) << 10))
                   : nullptr;
  // LDS staging (STAGE: sbase = this wave's 8 KiB, the whole wave is on
  // this path).  CHACHA: ctext staged for full-line stores.  !CHACHA (DEK
  // pass): plaintext loaded by buffer_load ... lds, 8 full lines per
  // instruction, one pair of blocks ahead, into the same swizzled image.
  // CHACHA: the image is shared by the plaintext pair (landing) and the
  // ctext pair (leaving: the lane takes its pair out, writes the ctext pair
  // back into the same slots, the wave stores full lines), so the next pair
  // is issued after the stores
  uint4 a0, a1, a2, a3;
  if constexpr (!STAGE) {
    a0 = q[0];
    a1 = q[1];
    a2 = q[2];
    a3 = q[3];
  }
  const uint32_t l = threadIdx.x & 63u, r = l >> 3, pc = l & 7u;
  const uint32_t wa = STAGE ? sbase + (l << 7) + (img_swz(l) << 4) : 0u;
  const uint32_t wst = CHACHA ? wa : 0u;  // full_block's staging target
  const uint32_t rb = sbase + (r << 7) + ((pc ^ img_swz(r)) << 4);
  // store voffset of (line r of this wave's 8-line group 0, piece pc); lane
  // l's data starts at chunk `first` of msg and lane 0's at first - l*G
  // (k_pass: first = t*G; k_small: msg = the wave's base, first = l*G)
  const uint32_t vo = ((first + (r - l) * uint32_t(G)) << 10) + (pc << 4);
  // wave-uniform descriptors (msg / cmsg, clen uniform over the wave)
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      CHACHA ? cmsg : const_cast<uint8_t *>(msg), 0, STAGE ? (cst == ~0u ? clen : cst) : 0u,
      0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_ld = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t *>(msg), 0, STAGE ? clen : 0u, 0x00020000);
  const uint32_t sb = __builtin_amdgcn_readfirstlane(sbase);
  // STAGE: source of (line 8k+r, image slot pc) = piece pc ^ swizzle(8k+r)
  const uint32_t lo0 = vo - (pc << 4) + ((pc ^ img_swz(r)) << 4);
  auto issue = [&](uint32_t s) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsrc_ld, (__attribute__((address_space(3))) void *)(uintptr_t)(sb + 1024u * k),
          16, (k & 1) ? (lo0 ^ 64u) : lo0, ((8u * k * uint32_t(G)) << 10) + 128u * s,
          0, 0);
  };
  if constexpr (STAGE) issue(0);
  for (uint32_t jj = 0; jj < uint32_t(G); ++jj) {
    // absolute chunk index (BLAKE3 chunk counter, ChaCha block counter / 16);
    // msg points at chunk cbase of the message
    const uint32_t chunk = cbase + first + jj;
#pragma unroll
    for (int i = 0; i < 8; ++i) cv[i] = key[i];
    for (uint32_t pp = 0; pp < 8; ++pp) {
      const uint32_t blk = jj * 16 + 2 * pp;
      uint4 b0, b1, b2, b3;
      if constexpr (STAGE) {
        // this pair's lines have landed; take them, then refill the image
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        u32x4 v[8];
        const uint32_t w = opaque(wa);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          v[i] = *reinterpret_cast<const lds_u32x4 *>(w ^ (uint32_t(i) << 4));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (!CHACHA && blk + 2 < NB) issue(blk / 2 + 1);
        a0 = make_uint4(v[0].x, v[0].y, v[0].z, v[0].w);
        a1 = make_uint4(v[1].x, v[1].y, v[1].z, v[1].w);
        a2 = make_uint4(v[2].x, v[2].y, v[2].z, v[2].w);
        a3 = make_uint4(v[3].x, v[3].y, v[3].z, v[3].w);
        b0 = make_uint4(v[4].x, v[4].y, v[4].z, v[4].w);
        b1 = make_uint4(v[5].x, v[5].y, v[5].z, v[5].w);
        b2 = make_uint4(v[6].x, v[6].y, v[6].z, v[6].w);
        b3 = make_uint4(v[7].x, v[7].y, v[7].z, v[7].w);
      } else {
        const uint4 *nb = q + 4 * (blk + 1);
        b0 = nb[0];
        b1 = nb[1];
        b2 = nb[2];
        b3 = nb[3];
      }
      constexpr bool stg = CHACHA && STAGE;
      // (the other branch is the same template as the latency-mode C-form
      // pass, which tests/test_gpu_parity.py::test_arx_forms_vs_oracle runs)
      if constexpr (GLFSX_PIPE && stg && A) {
        uint32_t fb = base;
        if (pp == 7) fb |= kChunkEnd | ((whole && G == 1) ? kRoot : 0u);
        pair_pipelined<A>(cv, a0, a1, a2, a3, b0, b1, b2, b3, chunk, 2 * pp,
                       base | (pp == 0 ? kChunkStart : 0u), fb, dek, wst);
      } else {
      full_block<CHACHA, stg, A>(cv, a0, a1, a2, a3, chunk, 2 * pp,
                         base | (pp == 0 ? kChunkStart : 0u), dek,
                         cq && !stg ? cq + 4 * blk : nullptr, wst, 0);
      if (!STAGE && blk + 2 < NB) {
        const uint4 *na = q + 4 * (blk + 2);
        a0 = na[0];
        a1 = na[1];
        a2 = na[2];
        a3 = na[3];
      }
      uint32_t fl = base;
      if (pp == 7) fl |= kChunkEnd | ((whole && G == 1) ? kRoot : 0u);
      full_block<CHACHA, stg, A>(cv, b0, b1, b2, b3, chunk, 2 * pp + 1, fl, dek,
                         cq && !stg ? cq + 4 * (blk + 1) : nullptr, wst, 1);
      }
      if (stg) {
        // lane l stores piece pc of line 8k + r: each store instruction
        // writes 8 whole 128-B lines.  Line 8k+r's slot for pc is
        // rb ^ ((k&1) << 6) + k*1024 (the swizzle's bit 2 is k's parity).
        const uint32_t r0 = opaque(rb), r1 = r0 ^ 64u, v0 = vo + blk * 64u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const u32x4 v = *reinterpret_cast<const lds_u32x4 *>(
              ((k & 1) ? r1 : r0) + 1024u * k);
          __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, v0,
              (8u * k * uint32_t(G)) << 10, 0);
        }
        if (blk + 2 < NB) {  // the image is free again: next pair
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          issue(blk / 2 + 1);
        }
      }
    }
    lane_merge<D, A>(cv, stk, depth, jj, jj + 1 == uint32_t(G), whole, key, base);
  }
}

// Lane-local subtree over chunks [first, first+n_my) of one message: returns
// its chaining value in cv (or the root output when `whole`: this lane holds
// the entire message).  Eager merges after chunk jj = ctz(jj+1), final merges
// right to left: the same tree as BLAKE3's incremental hasher.
template <int G, bool CHACHA, bool ALIGNED, int A = 2>
__device__ __forceinline__ void lane_subtree(
    uint32_t (&cv)[8], const uint8_t *msg, uint8_t *cmsg, uint64_t len,
    uint32_t first, uint32_t n_my, bool whole, const uint32_t (&key)[8],
    uint32_t base, const uint32_t (&dek)[8], uint32_t cbase = 0) {
  constexpr int D = ilog2(G);
  uint32_t stk[D > 0 ? D : 1][8];
  uint32_t depth = 0;
  for (uint32_t jj = 0; jj < n_my; ++jj) {
    const uint32_t lchunk = first + jj;           // within msg[0, len)
    const uint32_t chunk = cbase + lchunk;        // counter: absolute index
    const uint64_t coff = uint64_t(lchunk) << 10;
    const uint64_t rem = len - coff;
    const uint32_t clen = rem < 1024 ? uint32_t(rem) : 1024u;
    const uint32_t nb = clen ? (clen + 63) >> 6 : 1u;
    const bool last = jj + 1 == n_my;
#pragma unroll
    for (int i = 0; i < 8; ++i) cv[i] = key[i];
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t boff = b << 6;
      const uint32_t avail = clen - boff;
      uint32_t m[16];
      load_block<ALIGNED>(m, msg + coff + boff, avail);
      if constexpr (CHACHA) {
        uint32_t x[16];
        chacha_block<A>(x, dek, (chunk << 4) + b);
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] ^= x[i];
        if (avail < 64) mask_tail(m, avail);
        if (cmsg) store_block<ALIGNED>(cmsg + coff + boff, m, avail);
      }
      uint32_t fl = base;
      if (b == 0) fl |= kChunkStart;
      if (b + 1 == nb) {
        fl |= kChunkEnd;
        if (whole && n_my == 1) fl |= kRoot;
      }
      b3_compress<A>(cv, m, chunk, 0u, avail < 64 ? avail : 64u, fl);
    }
    lane_merge<D, A>(cv, stk, depth, jj, last, whole, key, base);
  }
}

// One lane writes the 32-byte result (CID or DEK) into its ref slot.  The
// slot is 16-B aligned for dense refs; index-node slots (node*bs + 64*i) may
// not be when bs % 16 != 0.
__device__ __forceinline__ void store_digest(uint8_t *dst, const uint32_t (&w)[8]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
  if ((a & 15) == 0) {
    uint4 *q = reinterpret_cast<uint4 *>(dst);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
  } else if ((a & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<uint32_t *>(dst)[i] = w[i];
  } else {
#pragma unroll
    for (int i = 0; i < 32; ++i) dst[i] = uint8_t(w[i >> 2] >> (8 * (i & 3)));
  }
}

// Pairwise merge of the k subtree CVs in lds[0 .. 8k) (all but the last are
// perfect subtrees of one power-of-two size, so this is BLAKE3's left-complete
// tree); the last parent gets ROOT when `root`.  Every thread of the block
// calls it; on return thread 0 holds the result in p (p = its own value on
// entry when k == 1).  Four lanes per parent compression (quad layout, as
// k_quad): tree_reduce_q, defined after quad_compress (quad_kernels.h).
// pass_body calls it through tree_merge: the compiler inlines in the order
// in which functions are first named, and naming tree_reduce_q in pass_body
// itself allocates registers in k_pass / k_pass_dc differently (one more
// instruction per kernel), so dropping this forwarder is a change to the
// device code, to be made and measured as one.
__device__ __forceinline__ void tree_reduce_q(uint32_t *lds, uint32_t k, uint32_t t,
                              const uint32_t (&key)[8], uint32_t base, bool root,
                              uint32_t (&p)[8]);
__device__ __forceinline__ void tree_merge(uint32_t *lds, uint32_t k, uint32_t t,
                                           const uint32_t (&key)[8], uint32_t base,
                                           bool root, uint32_t (&p)[8]) {
  tree_reduce_q(lds, k, t, key, base, root, p);
}

#if GLFSX_WGTIME
// Phase timestamps per workgroup of the bulk passes (A/B diagnostics only,
// tools/build_variant.sh wgtime "-DGLFSX_WGTIME=1"): [start, chunks done,
// subtree done, end, HW_ID, XCC_ID, k_pass_dc entry, item fetched, DEK wait
// over (k_pass_dc CID items), 7 spare]; DEK pass at [0, 4096), CID pass at
// [4096, 8192).  s_memrealtime: 100 MHz.
__device__ uint64_t g_wgtime[8192][16];
__device__ __forceinline__ void wgt(bool chacha, uint32_t bid, int slot) {
  const uint32_t b = bid + (chacha ? 4096u : 0u);  // the pass's own workgroup number
  if (threadIdx.x == 0 && b < 8192) {
    g_wgtime[b][slot] = __builtin_amdgcn_s_memrealtime();
    if (slot == 0) {
      g_wgtime[b][4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
      g_wgtime[b][5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
  }
}
#define WGT(bid, slot) wgt(CHACHA, bid, slot)
#else
#define WGT(bid, slot) (void)0
#endif

// A: the ARX form (b3_arx.h); 0, the compiler's form, issues faster when a
// launch leaves a SIMD one or two waves.
// One LDS array of uint4: [0, 8 KiB) CV tree, then kStage = 4 waves x 8 KiB
// of staging (ctext in the CHACHA pass, plaintext in the DEK pass): 40 KiB,
// 4 WGs per CU
constexpr int kStage = 4 * 512;

// State of a fused split launch (k_pass_dc).  Per (device, stream), in
// device memory (DcConst), read where it is used -- as kernel arguments
// these words would stay live in SGPRs through the whole body (the DEK/CID
// bodies then spilled SGPRs: 4 -> 33 at G = 2):
//  - ready[j] = epoch once message j's DEK is published (flags are never
//    reset: each launch has a new epoch, zero is never one);
//  - lists: two banks of kLists work-list counters, one per 128-B line
//    (k_pass_dc); launch e uses bank e & 1 and zeroes bank (e + 1) & 1 for
//    the next launch on the stream;
//  - err: a word in pinned host memory, set when a CID workgroup gave up
//    waiting for a DEK, or found no work item (the launch's results are
//    then invalid and the host fails or repeats the post);
//  - wait_ticks: that wait's bound in s_memrealtime ticks (100 MHz);
//  - skip_msg: test hook -- the DEK of this message is written but its
//    ready flag is not (~0u: none).
constexpr uint32_t kListStride = 32;  // words between counters (128 B); kLists: launch_plan.h
struct DcConst {
  uint32_t *ready;
  uint32_t *lists;
  uint32_t *err;
  uint64_t wait_ticks;
  uint32_t skip_msg;
};
// Per launch (kernel argument): the epoch, and the messages and log2
// workgroups per message of both passes (a.n, a.split_log2, given again so
// the item search does not touch the pass arguments: reading those before
// the branch made the bodies spill SGPRs).
struct DcState {
  uint32_t epoch;
  uint32_t n;
  uint32_t sl;
  uint32_t fine_div;  // the last ceil(m / fine_div) messages of each list
                      // run their CID pass as fine items (0: none)
  const DcConst *c;
};

// The DEK pass stores message j's DEK with agent-scope atomic stores, waits
// for them, then sets ready[j] = epoch; the CID workgroups of message j wait
// for that.
__device__ __forceinline__ void publish_dek(uint8_t *dst, const uint32_t (&w)[8],
                                            const DcState &d, uint64_t j) {
  publish_cv(reinterpret_cast<uint32_t *>(dst), w);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const DcConst *c = d.c;
  if (j != c->skip_msg)
    __hip_atomic_store(c->ready + j, d.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A CID item's wait for its message's DEK (k_pass_dc): from the DEK work
// items of the same launch.  Work items are taken from work lists
// (k_pass_dc), so every DEK item was taken by a workgroup that was already
// running before this one took its CID item: the wait depends only on
// running workgroups, whatever the dispatch order or other launches sharing
// the chip.  It is bounded anyway; a timeout marks the launch failed in
// d.err (the host then discards its results) and the workgroup finishes
// with whatever key it read, so counters and flags stay consistent for later
// launches.  Every thread of the workgroup calls it; dek is uniform.
__device__ __forceinline__ void dc_dek_wait(const DcState *dc, uint64_t j, uint32_t bid,
                                            const uint8_t *ref, uint32_t *lds,
                                            uint32_t (&dek)[8]) {
  (void)bid;
  if (threadIdx.x == 0) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    const DcConst *c = dc->c;  // (the DEK items this one waits for precede it in its list)
    while (__hip_atomic_load(c->ready + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) !=
           dc->epoch) {
      __builtin_amdgcn_s_sleep(4);
      if (__builtin_amdgcn_s_memrealtime() - t0 > c->wait_ticks) {
        __hip_atomic_store(c->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
    }
    // the DEK loads below must not be hoisted above the flag load that
    // saw the epoch (a compiler barrier; the loads are agent-scope, so no
    // cache invalidate is needed)
    __atomic_signal_fence(__ATOMIC_ACQUIRE);
#if GLFSX_WGTIME
    if (bid + 4096u < 8192u) g_wgtime[bid + 4096u][8] = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
    for (int i = 0; i < 8; ++i)
      lds[i] = load_cv_word(reinterpret_cast<const uint32_t *>(ref + 32) + i);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) dek[i] = __builtin_amdgcn_readfirstlane(lds[i]);
  __syncthreads();
}

// The body of one workgroup (number bid) of a pass.  FUSE: 0 = a pass of its
// own; 1 = the DEK part of k_pass_dc (publishes each DEK with its ready
// flag); 2 = the CID part (waits for its message's DEK).
template <int G, bool CHACHA, bool ALIGNED, int A, int FUSE>
__device__ __forceinline__ void pass_body(const KArgs &a, uint32_t bid, uint4 *lds_u4,
                                          const DcState *dc) {
  uint32_t *lds = reinterpret_cast<uint32_t *>(lds_u4);
  WGT(bid, 0);
  // message j, sub-range sidx (split mode) = chunks [sidx*256G, +256G)
  const uint64_t j = bid >> a.split_log2;
  const uint32_t sidx = bid & ((1u << a.split_log2) - 1u);
  const uint64_t len_full = (j + 1 == a.n) ? a.last_len : a.msg_len;
  constexpr uint64_t kSpan = uint64_t(256 * G) << 10;  // bytes per workgroup
  const uint64_t c0b = uint64_t(sidx) * kSpan;
  if (sidx != 0 && c0b >= len_full) return;  // empty sub-range (uniform)
  const uint64_t len = min(len_full - c0b, kSpan);
  const bool split = len_full > kSpan;  // the message spans > 1 workgroup
  const uint32_t cbase = sidx * uint32_t(256 * G);
  const uint8_t *msg = a.src + j * a.stride + c0b;
  uint8_t *cmsg = (CHACHA && a.ctext) ? a.ctext + j * a.stride + c0b : nullptr;
  uint8_t *ref = a.refs + (j / a.ref_bf) * a.ref_stride + (j % a.ref_bf) * 64;
  const uint32_t t = threadIdx.x;

  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = a.key[i];
  uint32_t dek[8];
  if constexpr (FUSE == 2) {
    dc_dek_wait(dc, j, bid, ref, lds, dek);
  } else if constexpr (CHACHA) {
    // DEK written by the preceding pass into bytes [32,64) of this ref slot.
    const uint8_t *dp = ref + 32;
    if ((reinterpret_cast<uintptr_t>(dp) & 3) == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        dek[i] = __builtin_amdgcn_readfirstlane(
            reinterpret_cast<const uint32_t *>(dp)[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        dek[i] = __builtin_amdgcn_readfirstlane(
            uint32_t(dp[4 * i]) | (uint32_t(dp[4 * i + 1]) << 8) |
            (uint32_t(dp[4 * i + 2]) << 16) | (uint32_t(dp[4 * i + 3]) << 24));
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) dek[i] = 0;
  }

  const uint32_t C = len ? uint32_t((len + 1023) >> 10) : 1u;
  const bool whole = !split && C <= uint32_t(G);
  const uint32_t first = t * G;
  const uint32_t n_my = first < C ? min(uint32_t(G), C - first) : 0u;
  uint32_t cv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool fast = ALIGNED && n_my == uint32_t(G) &&
                    len >= (uint64_t(first) + G) << 10;
  // staged stores write other lanes' lines: only when the whole wave is fast
  const bool wave_fast = __ballot(fast) == ~0ull;
  if (fast) {
    if (wave_fast && (cmsg || !CHACHA))  // wave-uniform
      lane_subtree_full<G, CHACHA, true, A>(
          cv, msg, cmsg, first, whole, key, a.base, dek,
          lds_offset(lds_u4 + 512 + (t >> 6) * 512), uint32_t(len), cbase);
    else
      lane_subtree_full<G, CHACHA, false, A>(cv, msg, cmsg, first, whole, key,
                                             a.base, dek, 0u, 0u, cbase);
  } else if (n_my) {
    lane_subtree<G, CHACHA, ALIGNED, A>(cv, msg, cmsg, len, first, n_my, whole,
                                     key, a.base, dek, cbase);
  }
  if (whole) {  // uniform: depends on len only; lane 0 holds the root output
    if (t == 0) {
      if constexpr (FUSE == 1) publish_dek(ref + a.out_off, cv, *dc, j);
      else store_digest(ref + a.out_off, cv);
    }
    return;
  }
  const uint32_t active = (C + G - 1) / G;
  if (t < active) {
#pragma unroll
    for (int i = 0; i < 8; ++i) lds[t * 8 + i] = cv[i];
  }
  __syncthreads();
  WGT(bid, 1);
  tree_merge(lds, active, t, key, a.base, !split, cv);
  WGT(bid, 2);
  if (!split) {
    if (t == 0) {
      if constexpr (FUSE == 1) publish_dek(ref + a.out_off, cv, *dc, j);
      else store_digest(ref + a.out_off, cv);
    }
    return;
  }
  // split (uniform): this workgroup's subtree CV to scratch; the message's
  // last workgroup merges the W = ceil(len / span) CVs (left-complete tree,
  // ROOT on the last parent) and resets the counter for the next launch
  const uint64_t wbase = j << a.split_log2;
  if (t == 0) publish_cv(a.scratch + (wbase + sidx) * 8, cv);
  const uint32_t W = uint32_t((len_full + kSpan - 1) / kSpan);
  // the arrival flag lives in the (now idle) staging image: one more LDS
  // word would take the kernel past 40 KiB, i.e. from four workgroups per
  // CU to three (160 KiB / 40 KiB)
  uint32_t *flag = reinterpret_cast<uint32_t *>(lds_u4 + 512);
  if (!arrive_last(a.cnt + j, W, t, flag)) {
    WGT(bid, 3);
    return;
  }
  if (t < W) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      cv[i] = load_cv_word(a.scratch + (wbase + t) * 8 + i);
      lds[t * 8 + i] = cv[i];
    }
  }
  __syncthreads();
  tree_merge(lds, W, t, key, a.base, true, cv);
  if (t == 0) {
    if constexpr (FUSE == 1) publish_dek(ref + a.out_off, cv, *dc, j);
    else store_digest(ref + a.out_off, cv);
    a.cnt[j] = 0;
  }
  WGT(bid, 3);
}

// Clock probe of the bulk passes (glfsx_clock_probe): once a process has
// called it, every k_pass workgroup adds its lifetime in shader-clock cycles
// (s_memtime) and in 100 MHz ticks (s_memrealtime) to these two device
// words (KArgs::clk), so a caller reads the clock the chip held over the
// launches since its reset: cycles / ticks x 100 MHz.  Two scalar timer
// reads per wave and, when on, two atomic adds per workgroup (thread 0).
// The words are per device, not per launch: k_pass launches of other
// callers on the same device in that window are counted too.
__device__ unsigned long long g_clk[2];

template <int G, bool CHACHA, bool ALIGNED, int A = 2>
__global__ __launch_bounds__(256) void k_pass(KArgs a) {
  __shared__ uint4 lds_u4[512 + kStage];
  const uint64_t c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  pass_body<G, CHACHA, ALIGNED, A, 0>(a, blockIdx.x, lds_u4, nullptr);
  if (threadIdx.x == 0 && a.clk) {
    const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    __hip_atomic_fetch_add(&a.clk[0], (unsigned long long)(c1 - c0), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&a.clk[1], (unsigned long long)(r1 - r0), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Both passes of a split-mode post in one launch: the DEK items run the DEK
// pass (a), the CID items the ChaCha20+CID pass (b), each CID item starting
// as soon as its message's DEK is published, so the CID pass fills the DEK
// pass's tail instead of waiting for the whole launch to drain.
//
// Work is taken from kLists lists, not by blockIdx: list x holds the items
// of messages j = x, x + 8, ... -- all their DEK items, then all their CID
// items -- and hands them out in that order through one device-wide
// counter.  A workgroup takes from the list of its own XCD first and moves
// on to the others when that one is used up.  A CID item then only ever
// waits for DEK items of its own list, which were handed out before it to
// workgroups that were already running: the wait needs no assumption about
// the order in which the hardware dispatches workgroups, how it places them
// on XCDs, or other launches (streams, processes) occupying the CUs.  Every
// workgroup finds an item (as many items as workgroups, each handed out
// once).  One counter per XCD keeps the start of the launch from queueing
// all 1024 first workgroups on one word (a single counter cost config 2
// 1.7 %), and keeps a message's DEK and CID items on one XCD.
template <int G>
__global__ __launch_bounds__(256) void k_pass_dc(KArgs a, KArgs b, KArgs c, DcState d) {
  __shared__ uint4 lds_u4[512 + kStage];
  uint32_t *lds = reinterpret_cast<uint32_t *>(lds_u4);
  // thread 0 finds the item and leaves (workgroup number within its pass,
  // kind: 0 DEK, 1 CID, 2 none) in LDS; only those two words stay live
  if (threadIdx.x == 0) {
#if GLFSX_WGTIME
    const uint64_t t_entry = __builtin_amdgcn_s_memrealtime();
#endif
    const uint32_t sl = d.sl;
    const uint32_t n = d.n;
    uint32_t *bank = d.c->lists + (d.epoch & 1u) * kLists * kListStride;
    if (blockIdx.x == 0) {  // the next launch's counters (this stream's last
      uint32_t *nb = d.c->lists + ((d.epoch + 1u) & 1u) * kLists * kListStride;
      for (uint32_t x = 0; x < kLists; ++x)  // user of them has completed)
        __hip_atomic_store(nb + x * kListStride, 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & (kLists - 1u);
    uint32_t bid = 0, kind = 2;
    for (uint32_t k = 0; k < kLists; ++k) {
      const uint32_t x = (xcc + k) & (kLists - 1u);
      const uint32_t msgs = dc_list_msgs(n, x);
      if (msgs == 0) continue;
      const uint32_t f = G > 1 ? dc_list_fine(msgs, d.fine_div) : 0u;
      const uint32_t t = __hip_atomic_fetch_add(bank + x * kListStride, 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t nd = msgs << sl, nc = (msgs - f) << sl;
      if (t < nd + nc) {  // DEK, or coarse CID: the list's message u >> sl
        const uint32_t u = t < nd ? t : t - nd;
        bid = ((x + kLists * (u >> sl)) << sl) | (u & ((1u << sl) - 1u));
        kind = t < nd ? 0u : 1u;
        break;
      }
      if (t < dc_list_items(msgs, f, sl)) {  // fine CID: 2^(sl+1) per message
        const uint32_t u = t - nd - nc;
        bid = ((x + kLists * (msgs - f + (u >> (sl + 1u)))) << (sl + 1u)) |
              (u & ((2u << sl) - 1u));
        kind = 3u;
        break;
      }
    }
    lds[0] = bid;
    lds[1] = kind;
#if GLFSX_WGTIME
    if (kind != 2 && bid + (kind ? 4096u : 0u) < 8192u) {  // kernel entry, item fetched
      g_wgtime[bid + (kind ? 4096u : 0u)][6] = t_entry;
      g_wgtime[bid + (kind ? 4096u : 0u)][7] = __builtin_amdgcn_s_memrealtime();
    }
#endif
  }
  __syncthreads();
  const uint32_t bid = __builtin_amdgcn_readfirstlane(lds[0]);
  const uint32_t kind = __builtin_amdgcn_readfirstlane(lds[1]);
  __syncthreads();
  if (kind == 2) {  // no item left anywhere: counters were not at zero
    if (threadIdx.x == 0)
      __hip_atomic_store(d.c->err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  if (kind == 0) {
    pass_body<G, false, true, 2, 1>(a, bid, lds_u4, &d);
  } else if (kind == 1) {
    pass_body<G, true, true, 2, 2>(b, bid, lds_u4, &d);
  } else {
    if constexpr (G > 1) pass_body<G / 2, true, true, 2, 2>(c, bid, lds_u4, &d);
  }
}
