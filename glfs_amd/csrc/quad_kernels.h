// quad_kernels.h -- BLAKE3 with four lanes per chaining state (latency mode):
// the quad-layout compression, tree_reduce_q, and the kernel k_quad.
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

// ---- Latency mode, BLAKE3-only passes: four lanes per chaining state ----
// A BLAKE3 chunk is 16 dependent compressions; in a launch that leaves one
// wave per SIMD their latency is the pass's latency.  Here lane q of a quad
// holds column q of the 4x4 state (a = v[q], b = v[4+q], c = v[8+q],
// d = v[12+q]) and runs one G per step; the diagonal step rotates rows b, c,
// d across the quad by DPP quad_perm and back.  The 16 message words sit in
// the quad's 64-B LDS slot; lane q reads the four it needs per round (words
// s_r[2q], s_r[2q+1], s_r[8+2q], s_r[9+2q]) at offsets fixed per lane.  A
// chaining value ends up as cv[q] = a ^ c, cv[4+q] = b ^ d in lane q.
// 1024-lane workgroups: 256 quads = 256 chunks (256 KiB) per workgroup; the
// workgroup's subtree is merged pairwise through the slots (the same
// left-complete tree as tree_reduce_q), and the last workgroup of a split
// message merges the workgroups' CVs.
//
// One round (column step, diagonal step) in quad layout as asm blocks
// (round 6).  tools/chainlat.hip measured the chain's
// instructions at one wave per SIMD: a dependent v_add/v_xor/v_alignbit
// chain issues every ~5-8 cycles and the wave as a whole about one VALU
// instruction per ~4.8 cycles whatever the dependences, so the round costs
// what it issues.  Every row rotation is folded into its first consumer
// (v_add_u32_dpp / v_xor_b32_dpp, the permute on src0): b, c, d stay in the
// diagonal frame (lanes q+1, q+2, q+3) from a diagonal step until the next
// column step reads them back; a never moves.  The diagonal step's first add
// is split as t = a + m2 (issued in the column step) then v_add_u32_dpp
// a = rot1(b) + t.  26 ARX instructions, one filler add and two s_nop 0 per
// round (a DPP read of a VGPR written one or two instructions before needs
// two wait states).  The earlier forms are in git history: the compiler's
// (rotations as DPP moves it folded itself, ~5.6 wait states per round) and
// a 33-instruction block with three v_mov_b32_dpp per step change
// (tools/qchain.hip: 1312 -> 1233 -> 1118 cycles per compression at one wave
// per SIMD; PostBlob 4 KiB p50 40.4 -> 37.7 us, config 2's index-node
// kernels 62.8 -> 57.9 us for the last step, profiles/r6/ab_qfold/).
// In: t = a + m0, m1..m3; the state in the column frame (QCOL0: lane q
// holds column q) or the diagonal frame (QCOL).  Out: the diagonal frame.
//   quad_perm [1,2,3,0]: lane q <- q+1; [2,3,0,1]: q+2; [3,0,1,2]: q+3.
#define QCOL0_ASM                                                               \
  "v_add_u32 %0, %1, %4\n"                                                      \
  "v_xor_b32 %3, %3, %0\n"                                                      \
  "v_alignbit_b32 %3, %3, %3, 16\n"                                             \
  "v_add_u32 %2, %2, %3\n"                                                      \
  "v_xor_b32 %1, %1, %2\n"                                                      \
  "v_alignbit_b32 %1, %1, %1, 12\n"
#define QCOL_ASM                                                                \
  "s_nop 0\n"                                                                   \
  "v_add_u32_dpp %0, %1, %4 quad_perm:[3,0,1,2] row_mask:0xf bank_mask:0xf\n"   \
  "v_xor_b32_dpp %3, %3, %0 quad_perm:[1,2,3,0] row_mask:0xf bank_mask:0xf\n"   \
  "v_alignbit_b32 %3, %3, %3, 16\n"                                             \
  "v_add_u32_dpp %2, %2, %3 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"   \
  "v_xor_b32_dpp %1, %1, %2 quad_perm:[3,0,1,2] row_mask:0xf bank_mask:0xf\n"   \
  "v_alignbit_b32 %1, %1, %1, 12\n"
#define QREST_ASM                                                               \
  "v_add3_u32 %0, %0, %1, %5\n"                                                 \
  "v_xor_b32 %3, %3, %0\n"                                                      \
  "v_alignbit_b32 %3, %3, %3, 8\n"                                              \
  "v_add_u32 %2, %2, %3\n"                                                      \
  "v_xor_b32 %1, %1, %2\n"                                                      \
  "v_alignbit_b32 %1, %1, %1, 7\n"                                              \
  "v_add_u32 %4, %0, %6\n"                                                      \
  "s_nop 0\n"                                                                   \
  "v_add_u32_dpp %0, %1, %4 quad_perm:[1,2,3,0] row_mask:0xf bank_mask:0xf\n"   \
  "v_xor_b32_dpp %3, %3, %0 quad_perm:[3,0,1,2] row_mask:0xf bank_mask:0xf\n"   \
  "v_alignbit_b32 %3, %3, %3, 16\n"                                             \
  "v_add_u32_dpp %2, %2, %3 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"   \
  "v_xor_b32_dpp %1, %1, %2 quad_perm:[1,2,3,0] row_mask:0xf bank_mask:0xf\n"   \
  "v_alignbit_b32 %1, %1, %1, 12\n"                                             \
  "v_add3_u32 %0, %0, %1, %7\n"                                                 \
  "v_xor_b32 %3, %3, %0\n"                                                      \
  "v_alignbit_b32 %3, %3, %3, 8\n"                                              \
  "v_add_u32 %2, %2, %3\n"                                                      \
  "v_xor_b32 %1, %1, %2\n"                                                      \
  "v_alignbit_b32 %1, %1, %1, 7\n"

// One compression in quad layout.  addr[4r+k]: LDS byte address of the k-th
// message word this lane uses in round r.  On return (a, b) = (cv[q], cv[4+q]).
// Every lane of a quad must be active (the rotations read the other three).
// quad_compress_m: m holds round 0's four words, already read; with PF, the
// four words at nxt (the next compression's round 0) are read during round 6
// and left in m, so a chain of compressions over a static LDS image waits
// for LDS only once (k_one).
typedef const __attribute__((address_space(3))) uint32_t *lds_word;
template <bool PF>
__device__ __forceinline__ void quad_compress_m(uint32_t &a, uint32_t &b, uint32_t c,
                                                uint32_t d, const uint32_t (&addr)[28],
                                                uint32_t (&m)[4], const uint32_t *nxt) {
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    uint32_t n[4] = {0, 0, 0, 0};
    if (r < 6) {
#pragma unroll
      for (int k = 0; k < 4; ++k) n[k] = *reinterpret_cast<lds_word>(addr[4 * r + 4 + k]);
    } else if (PF) {
#pragma unroll
      for (int k = 0; k < 4; ++k) n[k] = *reinterpret_cast<lds_word>(nxt[k]);
    }
    uint32_t t = a + m[0];
    if (r == 0)
      asm volatile(QCOL0_ASM QREST_ASM : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(t)
                   : "v"(m[1]), "v"(m[2]), "v"(m[3]));
    else
      asm volatile(QCOL_ASM QREST_ASM : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(t)
                   : "v"(m[1]), "v"(m[2]), "v"(m[3]));
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = n[k];
  }
  // back from the diagonal frame: a ^= c_q, b = b_q ^ d_q
  uint32_t u;
  asm volatile("v_xor_b32_dpp %0, %2, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n"
               "s_nop 1\n"
               "v_mov_b32_dpp %4, %1 quad_perm:[3,0,1,2] row_mask:0xf bank_mask:0xf\n"
               "v_xor_b32_dpp %1, %3, %4 quad_perm:[1,2,3,0] row_mask:0xf bank_mask:0xf\n"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "=&v"(u));
}

__device__ __forceinline__ void quad_compress(uint32_t &a, uint32_t &b,
                                              uint32_t c, uint32_t d,
                                              const uint32_t (&addr)[28]) {
  // round r+1's four words are read while round r runs
  uint32_t m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = *reinterpret_cast<lds_word>(addr[k]);
  quad_compress_m<false>(a, b, c, d, addr, m, nullptr);
}

__device__ __forceinline__ uint32_t qsel(uint32_t q, uint32_t x0, uint32_t x1,
                                         uint32_t x2, uint32_t x3) {
  return q == 0 ? x0 : q == 1 ? x1 : q == 2 ? x2 : x3;
}

// The 28 LDS addresses of a 64-B slot at byte `slot` for lane q; with x
// (a multiple of 4), word w of the slot lives at word w ^ x (the block
// slots of k_quad, below).
__device__ __forceinline__ void quad_addrs(uint32_t (&addr)[28], uint32_t slot,
                                           uint32_t q, uint32_t x = 0) {
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    constexpr int kk[4] = {0, 1, 8, 9};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = qsel(q, kSched.s[r][kk[k]], kSched.s[r][kk[k] + 2],
                              kSched.s[r][kk[k] + 4], kSched.s[r][kk[k] + 6]);
      addr[4 * r + k] = slot + 4u * (w ^ x);
    }
  }
}

// The pairwise merge with four lanes per parent: the k CVs at lds[0 .. 8k) merge
// pairwise, parent i reading its message (CV 2i || CV 2i+1) in place as the
// 64-B slot at lds + 16i words, 64 parents per step (256 lanes).  A one-lane
// parent is a chain of ~700 dependent instructions; in quad layout it is
// ~200 plus LDS reads, so the 8 levels of a 256-lane subtree (pass_body's
// per-workgroup merge, 13-18 us in round 2's per-workgroup timeline) take
// 9 short steps.  ROOT on the last parent when `root`; on return thread 0 holds the result in p.
__device__ __forceinline__ void tree_reduce_q(uint32_t *lds, uint32_t k, uint32_t t,
                              const uint32_t (&key)[8], uint32_t base, bool root,
                              uint32_t (&p)[8]) {
  const uint32_t q = t & 3u, quad = t >> 2;
  const uint32_t kq_lo = qsel(q, key[0], key[1], key[2], key[3]);
  const uint32_t kq_hi = qsel(q, key[4], key[5], key[6], key[7]);
  const uint32_t ivq = qsel(q, kIV[0], kIV[1], kIV[2], kIV[3]);
  uint32_t rel[28];
  quad_addrs(rel, lds_offset(lds), q);
  while (k > 1) {  // uniform
    const uint32_t half = k >> 1, odd = k & 1u;
    const uint32_t fl = base | kParent | ((root && k == 2) ? kRoot : 0u);
    const uint32_t dq = qsel(q, 0u, 0u, 64u, fl);
    uint32_t rl[2] = {0, 0}, rh[2] = {0, 0};
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {  // half <= 128 parents: <= 2 per quad
      const uint32_t i = quad + 64u * r;
      if (i < half) {  // quad-uniform
        uint32_t addr[28];
#pragma unroll
        for (int x = 0; x < 28; ++x) addr[x] = rel[x] + 64u * i;
        uint32_t cl = kq_lo, ch = kq_hi;
        quad_compress(cl, ch, ivq, dq, addr);
        rl[r] = cl;
        rh[r] = ch;
      }
    }
    // the odd CV moves from index k-1 to index half (its words are not
    // among the slots being rewritten: (k-1)*8 >= half*8)
    const uint32_t ov = (odd && t < 8) ? lds[(k - 1) * 8 + t] : 0u;
    __syncthreads();  // every slot of this level has been read
#pragma unroll
    for (uint32_t r = 0; r < 2; ++r) {
      const uint32_t i = quad + 64u * r;
      if (i < half) {
        lds[i * 8 + q] = rl[r];
        lds[i * 8 + 4 + q] = rh[r];
      }
    }
    if (odd && t < 8) lds[half * 8 + t] = ov;
    __syncthreads();
    k = half + odd;
  }
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = lds[i];
  }
}

// QPW quads (chunks) per workgroup: 256 (1024 lanes, 4 waves per SIMD) or
// 64 (256 lanes, one wave per SIMD: the chain runs at its latency instead
// of sharing its SIMD with three more waves; a 2 MiB node spreads over 32
// CUs instead of 8).
template <int QPW>
__global__ __launch_bounds__(QPW * 4) void k_quad(KArgs a) {
  // Block slots of the chunk phase: one 64-B slot per quad; QPW = 64 has a
  // second set QPW x 64 B further on (block b+1 is stored while block b
  // compresses, and its first words are read in block b's last round).
  // The subtree merges use the first set's 64-B slots as parent slots.
  constexpr bool kTwo = QPW == 64;
  __shared__ uint4 slots[QPW * (kTwo ? 8 : 4)];
  __shared__ uint32_t passbuf[8];       // the odd subtree passing up a level
  const uint32_t tid = threadIdx.x, q = tid & 3u, quad = tid >> 2;
  const uint64_t j = blockIdx.x >> a.split_log2;
  const uint32_t sidx = blockIdx.x & ((1u << a.split_log2) - 1u);
  const uint64_t len = (j + 1 == a.n) ? a.last_len : a.msg_len;
  constexpr uint64_t kSpan = uint64_t(QPW) << 10;
  const uint64_t c0b = uint64_t(sidx) * kSpan;
  if (sidx != 0 && c0b >= len) return;  // empty sub-range (uniform)
  const bool whole = len <= kSpan;       // the message fits this workgroup
  const uint64_t mylen = min(len - c0b, kSpan);
  const uint32_t cnt = mylen ? uint32_t((mylen + 1023) >> 10) : 1u;
  const uint8_t *msg = a.src + j * a.stride + c0b;
  const uint32_t slot = lds_offset(slots + quad * 4);
  const uint32_t kq_lo = qsel(q, a.key[0], a.key[1], a.key[2], a.key[3]);
  const uint32_t kq_hi = qsel(q, a.key[4], a.key[5], a.key[6], a.key[7]);
  const uint32_t ivq = qsel(q, kIV[0], kIV[1], kIV[2], kIV[3]);
  uint32_t addr[28];
  quad_addrs(addr, slot, q);
  uint32_t cl = kq_lo, ch = kq_hi;  // this quad's chaining value
  if (quad < cnt) {
    const uint64_t coff = uint64_t(quad) << 10;
    const uint32_t clen = uint32_t(min<uint64_t>(mylen - coff, 1024));
    const uint32_t nb = clen ? (clen + 63) >> 6 : 1u;
    const uint32_t ctr = sidx * uint32_t(QPW) + quad;  // chunk counter (messages < 4 GiB)
    const uint8_t *cp = msg + coff + 16u * q;
    uint4 blk[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      blk[b] = make_uint4(0, 0, 0, 0);
      const int32_t avail = int32_t(clen) - 64 * b - 16 * int32_t(q);
      if (avail >= 16) {
        blk[b] = *reinterpret_cast<const uint4 *>(cp + 64 * b);
      } else if (avail > 0) {
        uint32_t w[4] = {0, 0, 0, 0};
        for (int i = 0; i < avail; ++i) w[i >> 2] |= uint32_t(cp[64 * b + i]) << (8 * (i & 3));
        blk[b] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    // The quad's four lanes are one wave's, and a wave's LDS instructions
    // are performed in issue order: a compression's reads after its
    // block's store see it, and a later store into the slot comes after
    // them, so neither needs a wait (round 5 waited for both: two LDS round
    // trips per block on the chain); the empty asm keeps the compiler's
    // order.
    // Block slots are word-swizzled: word w of quad i's slot sits at word
    // w ^ x_i, x_i = 4 ((i >> 1) & 3), so the eight quads of a 32-lane LDS
    // group (ds_read_b32 banks = word mod 32) reading the same word hit
    // eight banks instead of two (plain 64-B slots: 4-way conflicts on every
    // message read); a lane's 16-B block store stays one aligned granule.
    // (QPW = 256 keeps plain slots: a second 28-address set would spill the
    // 1024-lane workgroup's 128 registers)
    const uint32_t x = kTwo ? 4u * ((quad >> 1) & 3u) : 0u;
    const uint32_t gq = 16u * (q ^ (x >> 2));  // this lane's granule in a slot
    constexpr uint32_t kB = kTwo ? QPW * 64u : 0u;  // the second slot set
    uint32_t caddr[28];
    if constexpr (kTwo) {
      quad_addrs(caddr, slot, q, x);
#pragma unroll
      for (int k = 0; k < 28; ++k) asm volatile("" : "+v"(caddr[k]));  // kept, not rebuilt per read
    }
    uint32_t m[4];
    if constexpr (kTwo) {
      *reinterpret_cast<lds_u32x4 *>(slot + gq) =
          u32x4{blk[0].x, blk[0].y, blk[0].z, blk[0].w};
      asm volatile("" ::: "memory");
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = *reinterpret_cast<lds_word>(caddr[k]);
    }
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      if (uint32_t(b) < nb) {
        const bool more = uint32_t(b) + 1 < nb;
        if constexpr (kTwo) {
          if (b + 1 < 16 && more)
            *reinterpret_cast<lds_u32x4 *>(slot + kB * ((b + 1) & 1) + gq) =
                u32x4{blk[(b + 1) & 15].x, blk[(b + 1) & 15].y, blk[(b + 1) & 15].z,
                      blk[(b + 1) & 15].w};
        } else {
          *reinterpret_cast<lds_u32x4 *>(slot + gq) =
              u32x4{blk[b].x, blk[b].y, blk[b].z, blk[b].w};
        }
        asm volatile("" ::: "memory");
        const uint32_t blen = min(clen - min(clen, 64u * b), 64u);
        uint32_t fl = a.base;
        if (b == 0) fl |= kChunkStart;
        if (uint32_t(b) + 1 == nb) {
          fl |= kChunkEnd;
          if (whole && cnt == 1) fl |= kRoot;
        }
        const uint32_t dq = qsel(q, ctr, 0u, blen, fl);
        if constexpr (kTwo) {
          uint32_t ab[28], nxt[4];
#pragma unroll
          for (int k = 0; k < 28; ++k) ab[k] = caddr[k] + kB * (b & 1);
          const uint32_t noff = more ? kB * ((b + 1) & 1) : kB * (b & 1);
#pragma unroll
          for (int k = 0; k < 4; ++k) nxt[k] = caddr[k] + noff;
          quad_compress_m<true>(cl, ch, ivq, dq, ab, m, nxt);
        } else {
          quad_compress(cl, ch, ivq, dq, addr);
        }
        asm volatile("" ::: "memory");
      }
    }
  }
  // the workgroup's subtree: pairwise through the slots
  uint32_t count = cnt;
  while (count > 1) {  // uniform
    const uint32_t half = count >> 1, odd = count & 1u;
    __syncthreads();  // slots of the previous level have been read
    if (quad < count) {
      if (odd && quad == count - 1) {
        passbuf[q] = cl;
        passbuf[4 + q] = ch;
      } else {
        uint32_t *ps = reinterpret_cast<uint32_t *>(slots + (quad >> 1) * 4);
        ps[(quad & 1u) * 8 + q] = cl;
        ps[(quad & 1u) * 8 + 4 + q] = ch;
      }
    }
    __syncthreads();
    if (quad < half) {
      const uint32_t fl = a.base | kParent | ((whole && count == 2) ? kRoot : 0u);
      cl = kq_lo;
      ch = kq_hi;
      const uint32_t dq = qsel(q, 0u, 0u, 64u, fl);
      quad_compress(cl, ch, ivq, dq, addr);
    } else if (odd && quad == half) {
      cl = passbuf[q];
      ch = passbuf[4 + q];
    }
    count = half + odd;
  }
  uint32_t *const out = reinterpret_cast<uint32_t *>(
      a.refs + (j / a.ref_bf) * a.ref_stride + (j % a.ref_bf) * 64 + a.out_off);
  if (whole) {
    if (quad == 0) {  // lanes 0-3: words q and 4+q of the result
      out[q] = cl;
      out[4 + q] = ch;
    }
    return;
  }
  // split: subtree CV to scratch; the message's last workgroup merges the W
  // CVs through the slots exactly like its own subtree (ROOT at the top)
  const uint64_t wbase = j << a.split_log2;
  if (tid < 64) {  // wave 0: quad 0's CV into lane 0, which stores it and
                   // then releases it (arrive_last) in program order
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w[k] = __builtin_amdgcn_readlane(cl, k);
      w[4 + k] = __builtin_amdgcn_readlane(ch, k);
    }
    if (tid == 0) publish_cv(a.scratch + (wbase + sidx) * 8, w);
  }
  const uint32_t W = uint32_t((len + kSpan - 1) / kSpan);
  __shared__ uint32_t s_flag;
  if (!arrive_last(a.cnt + j, W, tid, &s_flag)) return;
  if (quad < W) {
    cl = load_cv_word(a.scratch + (wbase + quad) * 8 + q);
    ch = load_cv_word(a.scratch + (wbase + quad) * 8 + 4 + q);
  }
  count = W;
  while (count > 1) {  // uniform
    const uint32_t half = count >> 1, odd = count & 1u;
    __syncthreads();
    if (quad < count) {
      if (odd && quad == count - 1) {
        passbuf[q] = cl;
        passbuf[4 + q] = ch;
      } else {
        uint32_t *ps = reinterpret_cast<uint32_t *>(slots + (quad >> 1) * 4);
        ps[(quad & 1u) * 8 + q] = cl;
        ps[(quad & 1u) * 8 + 4 + q] = ch;
      }
    }
    __syncthreads();
    if (quad < half) {
      const uint32_t fl = a.base | kParent | (count == 2 ? kRoot : 0u);
      cl = kq_lo;
      ch = kq_hi;
      const uint32_t dq = qsel(q, 0u, 0u, 64u, fl);
      quad_compress(cl, ch, ivq, dq, addr);
    } else if (odd && quad == half) {
      cl = passbuf[q];
      ch = passbuf[4 + q];
    }
    count = half + odd;
  }
  if (quad == 0) {
    out[q] = cl;
    out[4 + q] = ch;
    if (q == 0) a.cnt[j] = 0;
  }
}
