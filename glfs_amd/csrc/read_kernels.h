// read_kernels.h -- the read side and utilities: k_decrypt, k_decrypt_lines,
// k_chacha_xor, and k_fill (synthetic data).
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

// Read side (bigblob/ref.go:113-126 getF -> cryptoXOR, blob.go:31-69): decrypt
// n blocks of bs bytes (bs % 64 == 0) laid out contiguously, block j with
// the DEK in bytes [32,64) of refs[j].  One thread per 64-B keystream block.
__global__ __launch_bounds__(256) void k_decrypt(KArgs a) {
  const uint64_t per = a.msg_len >> 6;  // keystream blocks per bigblob block
  const uint64_t total_kb = (a.n - 1) * per + ((a.last_len + 63) >> 6);
  // a.stride: first keystream block (the part before it went through
  // k_decrypt_lines)
  for (uint64_t kb = a.stride + blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; kb < total_kb;
       kb += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t j = kb / per;
    const uint32_t ctr = uint32_t(kb - j * per);
    const uint64_t off = kb << 6;
    const uint64_t end = j * a.msg_len + ((j + 1 == a.n) ? a.last_len : a.msg_len);
    const uint32_t avail = uint32_t(min<uint64_t>(64, end - off));
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(a.refs + j * 64 + 32);
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = dp[i];
    uint32_t m[16], x[16];
    const bool al = ((reinterpret_cast<uintptr_t>(a.src) |
                      reinterpret_cast<uintptr_t>(a.ctext)) & 15) == 0;
    if (al) load_block<true>(m, a.src + off, avail);
    else load_block<false>(m, a.src + off, avail);
    chacha_block(x, k, ctr);
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] ^= x[i];
    if (al) store_block<true>(a.ctext + off, m, avail);
    else store_block<false>(a.ctext + off, m, avail);
  }
}

// Read side, bulk: one wave per 4 KiB unit of ctext (lane l = keystream
// block l of the unit), bs % 4096 == 0 so the unit's DEK is uniform (scalar
// loads into SGPRs; the key-only quarter-rounds of round 1 are hoisted by the
// compiler).  Each wave has two 4 KiB images: unit u+stride arrives by
// buffer_load ... lds (4 instructions x 8 full 128-B lines) while unit u is
// decrypted.  Image layout: piece p (16 B) of lane L's block sits at
// 64L + 16 (p ^ ((L >> 2) & 3)), so the lane's ds_read_b128s are conflict-free
// and the loader / storer lane l of instruction k touches image byte
// 1024k + 16l <-> unit byte 1024k + vo(l).  Covers units [0, n_units);
// k_decrypt does the rest.
template <int A>
__global__ __launch_bounds__(256) void k_decrypt_lines(KArgs a, uint64_t n_units,
                                                       uint32_t upb_shift,
                                                       uint32_t run_shift) {
  __shared__ uint4 img[4 * 512];
  const uint32_t l = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t wbase = lds_offset(img + wv * 512);
  const uint32_t sb = __builtin_amdgcn_readfirstlane(wbase);
  const uint32_t vo = ((l >> 2) << 6) + (((l & 3u) ^ ((l >> 4) & 3u)) << 4);
  const uint32_t wa = wbase + (l << 6) + (((l >> 2) & 3u) << 4);
  const uint32_t rl = wbase + (l << 4);  // linear slot for the stores
  const uint64_t upb = a.msg_len >> 12;  // units per bigblob block
  // the wave walks runs of R = 2^run_shift consecutive units inside one
  // bigblob block (R divides the units per block): the DEK and its key-only
  // quarter-rounds are loop-invariant over a run
  const uint64_t n_runs = (n_units + (1ull << run_shift) - 1) >> run_shift;
  const uint64_t wstride = uint64_t(gridDim.x) * 4;
  auto issue = [&](uint64_t uu, uint32_t buf) {
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.src) + (uu << 12), 0, 4096u, 0x00020000);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          src, (__attribute__((address_space(3))) void *)(uintptr_t)(sb + 4096u * buf + 1024u * k),
          16, vo, 1024u * k, 0, 0);
  };
  uint64_t run = uint64_t(blockIdx.x) * 4 + wv;
  if (run < n_runs) issue(run << run_shift, 0);
  uint32_t buf = 0;
  for (; run < n_runs; run += wstride) {
    const uint64_t u0 = run << run_shift;
    const uint64_t u1 = min(u0 + (1ull << run_shift), n_units);
    // bigblob block (uniform): its DEK.  upb_shift = log2(units per block)
    // when that is a power of two (no 64-bit scalar division per run)
    const uint64_t j = upb_shift < 64 ? u0 >> upb_shift : u0 / upb;
    const __attribute__((address_space(4))) uint32_t *kp =
        (const __attribute__((address_space(4))) uint32_t *)(uintptr_t)(
            a.refs + j * 64 + 32);
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = kp[i];
    const uint64_t nrun = run + wstride;
   for (uint64_t u = u0; u < u1; ++u, buf ^= 1u) {
    const uint64_t un = u + 1 < u1 ? u + 1 : (nrun << run_shift);
    // the other image was last read by the previous unit's store ds_reads
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const bool more = u + 1 < u1 || nrun < n_runs;
    if (more) issue(un, buf ^ 1u);
    // this unit's lines: all but the 4 youngest vector-memory ops (the next
    // unit's loads) are done -- the previous unit's stores included
    if (more)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t w = opaque(wa) + 4096u * buf;
    u32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      v[q] = *reinterpret_cast<const lds_u32x4 *>(w ^ (uint32_t(q) << 4));
    uint32_t x[16];
    chacha_block<A>(x, key, uint32_t((u - j * upb) << 6) + l);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x4 c = v[q];
      c.x ^= x[4 * q];
      c.y ^= x[4 * q + 1];
      c.z ^= x[4 * q + 2];
      c.w ^= x[4 * q + 3];
      *reinterpret_cast<lds_u32x4 *>(w ^ (uint32_t(q) << 4)) = c;
    }
    const __amdgpu_buffer_rsrc_t dst =
        __builtin_amdgcn_make_buffer_rsrc(a.ctext + (u << 12), 0, 4096u, 0x00020000);
    const uint32_t r0 = opaque(rl) + 4096u * buf;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u32x4 c = *reinterpret_cast<const lds_u32x4 *>(r0 + 1024u * k);
      __builtin_amdgcn_raw_buffer_store_b128(c, dst, vo, 1024u * k, 0);
    }
   }
  }
}

__global__ __launch_bounds__(256) void k_chacha_xor(KArgs a) {
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = a.key[i];
  const uint64_t nblk = (a.msg_len + 63) >> 6;
  for (uint64_t b = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; b < nblk;
       b += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t off = b << 6;
    const uint64_t rem = a.msg_len - off;
    const uint32_t avail = rem < 64 ? uint32_t(rem) : 64u;
    uint32_t m[16], x[16];
    const bool al = ((reinterpret_cast<uintptr_t>(a.src + off) |
                      reinterpret_cast<uintptr_t>(a.ctext + off)) & 15) == 0;
    if (al) load_block<true>(m, a.src + off, avail);
    else load_block<false>(m, a.src + off, avail);
    chacha_block(x, k, uint32_t(b));
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] ^= x[i];
    if (al) store_block<true>(a.ctext + off, m, avail);
    else store_block<false>(a.ctext + off, m, avail);
  }
}

// Synthetic data (bench/test inputs): byte o = byte (o & 7) of
// splitmix64(seed ^ (o >> 3)); same generator as oracle_fill_splitmix.
__global__ __launch_bounds__(256) void k_fill(uint8_t *dst, uint64_t offset,
                                              uint64_t n, uint64_t seed) {
  const uint64_t words = (n + 7) >> 3;
  for (uint64_t w = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; w < words;
       w += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t v = splitmix64(seed ^ ((offset >> 3) + w));
    if ((w + 1) * 8 <= n && ((reinterpret_cast<uintptr_t>(dst) & 7) == 0)) {
      reinterpret_cast<uint64_t *>(dst)[w] = v;
    } else {
      for (uint64_t i = w * 8; i < n && i < w * 8 + 8; ++i)
        dst[i] = uint8_t(v >> (8 * (i & 7)));
    }
  }
}
