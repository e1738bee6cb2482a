// one_open_kernels.h -- the one-shot verified read: one block of at most
// kMaxOneLen bytes checked and decrypted by one workgroup of one launch
// (k_one_open, k_one_open_v), the read side's counterpart of k_one.
// A fragment of the post_kernels.hip translation unit, included there after
// one_kernels.h inside its namespace; not a stand-alone header.

// On the write side the DEK must exist before the keystream, so k_one's two
// BLAKE3 trees run in series.  Here the DEK arrives with the ref:
//   stage : the ctext from the caller's pinned staging into image A
//           (one_stage: every load in flight at once, zero padded, swizzled);
//   xor   : lane t makes keystream block t (+ k * lanes) with the ref's DEK
//           and writes A ^ keystream into image B (tail masked, so B is zero
//           past len as A is); B is stored out while the hashes run;
//   hash  : quads [0, QUADS) hash A under the CID key, quads [QUADS, 2 QUADS)
//           hash B under the salt, in lock-step: both messages have the same
//           length, so the same chunk count and merge tree, and every
//           __syncthreads() of one_tree is reached by both halves with the
//           same trip count.  Each tree has its own parent slots and
//           pass-through buffer;
//   check : the four lanes holding each root compare it with the ref's words.
// SALTED = false is the CID-only form: QUADS quads, no image B (the
// plaintext, when wanted, goes from the registers to the caller's staging).

// A ^ ChaCha20(dek) over the padded image (whole 64-B blocks; one block
// when empty), the keystream masked past len.  TO_LDS: into image B with A's
// swizzle; otherwise bytes [0, len) to dst (16-B aligned, not null).
template <int LANES, bool TO_LDS>
__device__ __forceinline__ void one_open_xor(const uint4 *a_u4, uint4 *b_u4, uint8_t *dst,
                                             uint32_t len, const uint32_t (&dek)[8]) {
  const uint32_t nblk = len ? (len + 63) >> 6 : 1u;
  for (uint32_t kb = threadIdx.x; kb < nblk; kb += LANES) {
    uint32_t x[16];
    chacha_block<0>(x, dek, kb);
    const uint32_t avail = min(len - min(len, kb * 64u), 64u);
    if (avail < 64) mask_tail(x, avail);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint4 v = a_u4[img_g(kb * 4 + i)];
      v.x ^= x[4 * i];
      v.y ^= x[4 * i + 1];
      v.z ^= x[4 * i + 2];
      v.w ^= x[4 * i + 3];
      if constexpr (TO_LDS) {
        b_u4[img_g(kb * 4 + i)] = v;
      } else {
        const uint32_t p = kb * 64u + 16u * i;
        if (p + 16u <= len) {
          *reinterpret_cast<uint4 *>(dst + p) = v;
        } else {
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
          for (uint32_t k = 0; p + k < len; ++k) dst[p + k] = uint8_t(w[k >> 2] >> (8 * (k & 3)));
        }
      }
    }
  }
}

// The body of a one-shot verified read.  V: g is the descriptor itself (a
// kernel argument); otherwise the launch's array in pinned host memory,
// staged by one_desc.
template <int QUADS, bool SALTED, bool V>
__device__ __forceinline__ void one_open_run(const OneOpenDesc *g) {
  constexpr int kTrees = SALTED ? 2 : 1;
  constexpr int kLanes = QUADS * 4 * kTrees;
  __shared__ uint4 img_u4[kTrees][QUADS * 64];     // A: the ctext; B: the plaintext
  __shared__ uint4 ts_u4[kTrees][QUADS / 2 * 4];   // each tree's parent inputs
  __shared__ uint32_t passbuf[kTrees][8];
  __shared__ uint32_t s_status;
  const OneOpenDesc *dp;
  if constexpr (V) {
    dp = g;
  } else {
    __shared__ OneOpenDesc s_desc;
    dp = one_desc(&s_desc, g + blockIdx.x);
  }
  const uint32_t len = dp->len;
  const uint32_t tid = threadIdx.x, q = tid & 3u, quad = tid >> 2;
  if (tid == 0) s_status = 0;
  // 16 (CID only) or 8 loads per lane cover the image: kLanes x IT x 16 B
  one_stage<kLanes, 16 / kTrees>(img_u4[0], dp->src, len, len, nullptr);
  uint32_t rel[28];
  quad_addrs(rel, 0u, q);
  __syncthreads();
  uint32_t dek[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) dek[i] = dp->ref[8 + i];
  uint8_t *const ptext = dp->ptext;
  uint32_t cl, ch;
  if constexpr (SALTED) {
    one_open_xor<kLanes, true>(img_u4[0], img_u4[1], nullptr, len, dek);
    __syncthreads();
    if (ptext) one_store<kLanes>(img_u4[1], ptext, len);  // drains during the hashes
    // this lane's tree: 0 the CID over A, 1 the DEK over B
    const bool t1 = quad >= uint32_t(QUADS);
    const uint32_t rq = t1 ? quad - uint32_t(QUADS) : quad;
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = t1 ? dp->salt[i] : dp->cid_key[i];
    const uint32_t base = (t1 || dp->cid_keyed) ? kKeyed : 0u;
    one_hash(cl, ch, lds_offset(img_u4[t1 ? 1 : 0]), lds_offset(ts_u4[t1 ? 1 : 0]),
             passbuf[t1 ? 1 : 0], len, key, base, q, rq, rel);
    if (rq == 0) {  // lanes 0-3 of each half: root words q and 4+q
      const uint32_t o = t1 ? 8u : 0u;
      if (cl != dp->ref[o + q] || ch != dp->ref[o + 4 + q])
        atomicOr(&s_status, t1 ? 2u : 1u);
    }
  } else {
    if (ptext) one_open_xor<kLanes, false>(img_u4[0], nullptr, ptext, len, dek);
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = dp->cid_key[i];
    one_hash(cl, ch, lds_offset(img_u4[0]), lds_offset(ts_u4[0]), passbuf[0], len, key,
             dp->cid_keyed ? kKeyed : 0u, q, quad, rel);
    if (quad == 0 && (cl != dp->ref[q] || ch != dp->ref[4 + q])) atomicOr(&s_status, 1u);
  }
  __syncthreads();
  if (tid == 0) *dp->status = s_status;
  one_signal(dp);
}

template <int QUADS, bool SALTED>
__global__ __launch_bounds__(QUADS * (SALTED ? 8 : 4)) void k_one_open(const OneOpenDesc *descs) {
  one_open_run<QUADS, SALTED, false>(descs);
}

// A launch of one request: the descriptor travels as the kernel argument (as
// k_one_v's).
template <int QUADS, bool SALTED>
__global__ __launch_bounds__(QUADS * (SALTED ? 8 : 4)) void k_one_open_v(const OneOpenDesc d) {
  one_open_run<QUADS, SALTED, true>(&d);
}
