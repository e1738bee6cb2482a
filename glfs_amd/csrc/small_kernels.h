// small_kernels.h -- small blobs, one lane per blob: SArgs, the hex output of
// roots, small_blob / small_fine, and the kernels k_small and k_small_q.
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

// Small blobs (glfs.PostBlob of many blobs that each fit one bigblob block,
// e.g. BASELINE config 4's 1M x 4 KiB): one lane per blob.  A blob of
// 0 < len <= block_size has root = post(rawSalt, blob) (blob.go:190-193); the
// empty blob has root = post(indexSalt, "") (blob.go:187-189), so the key is
// selected per lane.  Every lane finishes its own BLAKE3 tree (G >= chunks).
struct SArgs {
  const uint8_t *src;
  uint8_t *ctext;
  const uint64_t *offs;
  const uint64_t *lens;
  uint64_t n;
  uint8_t *refs;      // 64 B per blob, dense
  uint32_t key[8];    // DEK pass: rawSalt words; CID pass: CID key words
  uint32_t key0[8];   // DEK pass: indexSalt words (empty blobs); CID pass: = key
  uint32_t base;
  uint32_t out_off;
  uint64_t n_coarse;  // k_small_q: items [0, n_coarse) are 64 blobs (one per
                      // lane); the blobs after them go as fine items
  uint64_t small_max;  // longer blobs are skipped (SmallJob::small_max)
  uint8_t *hex_out;    // CID pass, nullable: the root as tree-line hex digits
  const uint64_t *hex_pos;
};

// The 64 hex digits of the 32 bytes in w (tree.go:309's "cid"/"dek" field
// of a TreeEntry line, encoding as tree_kernels.hip's hex32) at dst, any
// alignment: aligned 4-byte stores of the digits shifted into place
// (alignbyte), the two partial words at the ends byte by byte -- no byte
// outside [dst, dst + 64) is written.
__device__ __forceinline__ void put_hex32(uint8_t *dst, const uint32_t w[8]) {
  const uint32_t s = uint32_t(reinterpret_cast<uintptr_t>(dst) & 3u);
  const uint32_t sh = 8u * (4u - s);  // s = 0: the whole next word
  uint32_t *base = reinterpret_cast<uint32_t *>(dst - s);
  uint32_t prev = 0;  // streamed one digit word at a time: few live values
#pragma unroll
  for (int k = 0; k <= 16; ++k) {
    const uint32_t cur = k < 16 ? hex4(w[k >> 1] >> (16 * (k & 1))) : 0u;
    const uint32_t v = uint32_t(((uint64_t(cur) << 32) | prev) >> sh);
    if ((k >= 1 && k <= 15) || (k == 0 && s == 0)) {
      base[k] = v;
    } else {
      const uint32_t lo = k == 0 ? s : 0u, hi = k == 0 ? 4u : s;
      uint8_t *b = reinterpret_cast<uint8_t *>(base + k);
      for (uint32_t x = lo; x < hi; ++x) b[x] = uint8_t(v >> (8u * x));
    }
    prev = cur;
  }
}

// Blob i for the calling lane (nothing when i >= n); lds_u4: the
// workgroup's 4 x 8 KiB staging images.  No barriers.
template <int G, bool CHACHA, int A>
__device__ __forceinline__ void small_blob(const SArgs &a, uint64_t i, uint4 *lds_u4) {
  if (i >= a.n) return;
  const uint64_t off = a.offs[i], len = a.lens[i];
  if (len > a.small_max) return;  // posted by the host's large-blob route
  const uint8_t *msg = a.src + off;
  uint8_t *cmsg = (CHACHA && a.ctext) ? a.ctext + off : nullptr;
  uint8_t *ref = a.refs + i * 64;
  uint32_t key[8], dek[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) key[w] = len ? a.key[w] : a.key0[w];
  if constexpr (CHACHA) {
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(ref + 32);
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = dp[w];
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = 0;
  }
  const uint32_t C = len ? uint32_t((len + 1023) >> 10) : 1u;
  const bool aligned = ((reinterpret_cast<uintptr_t>(msg) |
                         reinterpret_cast<uintptr_t>(cmsg)) & 15) == 0;
  uint32_t cv[8];
  // a full wave of back-to-back blobs of exactly G KiB (config 4: 4 KiB
  // blobs packed densely) has k_pass's lane layout: stage through LDS for
  // full-line loads (and ctext stores)
  const uint32_t l = threadIdx.x & 63u;
  // (readfirstlane returns int: widen through uint32_t, or a low word of
  // 2^31 or more sign-extends into the high word -- every wave of blobs in
  // the upper 2 GiB of each 4 GiB then failed the density test below and
  // took the per-lane path)
  const uint64_t o0 =
      (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(off >> 32)))) << 32) |
      uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(off)));
  const bool dense = aligned && len == uint64_t(G) << 10 &&
                     off == o0 + (uint64_t(l) * G << 10) && (!CHACHA || cmsg);
  if (__ballot(dense) == ~0ull) {  // wave-uniform
    lane_subtree_full<G, CHACHA, true, A>(
        cv, a.src + o0, cmsg ? a.ctext + o0 : nullptr, l * G, true, key, a.base,
        dek, lds_offset(lds_u4 + (threadIdx.x >> 6) * 512), 64u * G << 10,
        0u - l * G);
  } else if (aligned && len == uint64_t(G) << 10) {
    lane_subtree_full<G, CHACHA, false, A>(cv, msg, cmsg, 0u, true, key, a.base, dek);
  } else if (aligned) {
    lane_subtree<G, CHACHA, true, A>(cv, msg, cmsg, len, 0u, C, true, key, a.base, dek);
  } else {
    lane_subtree<G, CHACHA, false, A>(cv, msg, cmsg, len, 0u, C, true, key, a.base, dek);
  }
  store_digest(ref + a.out_off, cv);
  if (CHACHA && a.hex_out) {  // the tree line's cid and dek digits
    const uint64_t pos = a.hex_pos[i];
    if (pos != ~0ull) {  // ~0: the lines did not fit their buffer
      put_hex32(a.hex_out + pos, cv);
      put_hex32(a.hex_out + pos + kDekAfterCid, dek);
    }
  }
}

// A fine item of k_small_q: 64/G blobs, G lanes per blob (lane l hashes
// chunk l % G of blob b0 + l / G), so the item takes about 1/G of a
// one-lane-per-blob item's time.  Handed out last, they shorten the run-down
// at the end of the launch.  Dense blobs of exactly G KiB take k_pass's
// staged G = 1 lane layout over the wave's contiguous 64 KiB; the G chunk
// CVs of a blob then merge through lane shuffles (log2 G parent levels, ROOT
// on the last: the same tree as a lane's own stack).  Anything else: one
// lane per blob on the first 64/G lanes.
template <int G, bool CHACHA, int A>
__device__ __forceinline__ void small_fine(const SArgs &a, uint64_t b0, uint4 *lds_u4) {
  constexpr uint32_t BPI = 64u / G;
  const uint32_t l = threadIdx.x & 63u, c = l % G;
  const uint64_t i = b0 + l / G;
  const bool valid = i < a.n;
  const uint64_t off = valid ? a.offs[i] : 0, len = valid ? a.lens[i] : 0;
  const uint8_t *msg = a.src + off;
  uint8_t *cmsg = (CHACHA && a.ctext) ? a.ctext + off : nullptr;
  const uint64_t o0 =
      (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(off >> 32)))) << 32) |
      uint32_t(__builtin_amdgcn_readfirstlane(uint32_t(off)));
  const bool aligned = ((reinterpret_cast<uintptr_t>(msg) |
                         reinterpret_cast<uintptr_t>(cmsg)) & 15) == 0;
  const bool dense = valid && aligned && len == uint64_t(G) << 10 && len <= a.small_max &&
                     off == o0 + (uint64_t(l) << 10) - (uint64_t(c) << 10) &&
                     (!CHACHA || cmsg);
  if (__ballot(dense) != ~0ull) {
    small_blob<G, CHACHA, A>(a, l < BPI ? b0 + l : ~0ull, lds_u4);
    return;
  }
  uint8_t *ref = a.refs + i * 64;
  uint32_t key[8], dek[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) key[w] = a.key[w];
  if constexpr (CHACHA) {
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(ref + 32);
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = dp[w];
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = 0;
  }
  uint32_t cv[8];
  lane_subtree_full<1, CHACHA, true, A>(
      cv, a.src + o0, CHACHA ? a.ctext + o0 : nullptr, l, false, key, a.base, dek,
      lds_offset(lds_u4 + (threadIdx.x >> 6) * 512), 64u << 10, c - l);
#pragma unroll
  for (uint32_t st = 1; st < uint32_t(G); st <<= 1) {
    uint32_t m[16];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      m[w] = cv[w];
      m[8 + w] = uint32_t(__shfl_down(int(cv[w]), st, 64));
      cv[w] = key[w];
    }
    b3_compress<A>(cv, m, 0u, 0u, 64u, a.base | kParent | (2 * st == G ? kRoot : 0u));
  }
  if (c == 0) {
    store_digest(ref + a.out_off, cv);
    if (CHACHA && a.hex_out) {
      const uint64_t pos = a.hex_pos[i];
      if (pos != ~0ull) {
        put_hex32(a.hex_out + pos, cv);
        put_hex32(a.hex_out + pos + kDekAfterCid, dek);
      }
    }
  }
}

template <int G, bool CHACHA, int A = 2>
__global__ __launch_bounds__(256) void k_small(SArgs a) {
  // 4 waves x 8 KiB staging image (same layout as k_pass's)
  __shared__ uint4 lds_u4[4 * 512];
  small_blob<G, CHACHA, A>(a, blockIdx.x * uint64_t(blockDim.x) + threadIdx.x, lds_u4);
}

// The same with as many workgroups as the chip holds at once, each WAVE
// taking items of 64 consecutive blobs: its first by its number, the next
// ones from a device-wide counter (bank epoch & 1 of two, the other zeroed
// by workgroup 0 for the next launch on the stream).  A wave that finishes
// early takes more, so the launch ends within about one item of its last
// wave instead of with whole workgroups' worth of CUs idle (config 4's
// 4096-workgroup launches lost ~12 % to that tail: scripts/sb_sizes.py).
// kSmallQWaves waves per SIMD at least (4: at most 128 VGPRs, like
// k_small; the loop let the CID form grow to 133 VGPRs, i.e. three waves,
// and capping it spills 5 VGPRs: both measured)
constexpr int kSmallQWaves = 4;
template <int G, bool CHACHA, int A = 2>
__global__ __launch_bounds__(256, kSmallQWaves) void k_small_q(SArgs a, uint32_t *ctr,
                                                               uint32_t epoch) {
  __shared__ uint4 lds_u4[4 * 512];
  if (blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_store(ctr + ((epoch + 1u) & 1u) * 32u, 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  uint32_t *mine = ctr + (epoch & 1u) * 32u;
  constexpr uint32_t BPI = G > 1 ? 64u / G : 64u;
  const uint64_t fine0 = a.n_coarse << 6;
  const uint64_t items = a.n_coarse + (a.n > fine0 ? (a.n - fine0 + BPI - 1) / BPI : 0);
  const uint32_t waves = gridDim.x * 4u;
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t item = blockIdx.x * 4u + (threadIdx.x >> 6);
  while (item < items) {  // wave-uniform
    if (G == 1 || item < a.n_coarse)
      small_blob<G, CHACHA, A>(a, (item << 6) | lane, lds_u4);
    else if constexpr (G > 1)
      small_fine<G, CHACHA, A>(a, fine0 + (item - a.n_coarse) * BPI, lds_u4);
    uint32_t t = 0;
    if (lane == 0)
      t = __hip_atomic_fetch_add(mine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    item = waves + uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(t)));
  }
}
