// ragged_kernels.h -- a post over messages of unequal length in throughput
// form: RArgs, the plan (k_rag_count / k_rag_prefix), the chunk pass
// (rag_chunk, k_rag_chunk) and the two merge levels (k_rag_merge_a,
// k_rag_merge_b).
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

// The messages i with lo < lens[i] <= hi of a batch (the others are skipped,
// their ref slots left alone) are flattened into one sequence of BLAKE3
// chunks, C_i = max(1, ceil(len_i / 1024)) each, and the work is handed out
// by flattened chunk number: work is proportional to the bytes, whatever the
// mix of lengths.  Nothing inside a launch waits for another workgroup; every
// hand-off is a kernel boundary on the stream:
//   plan   k_rag_count, k_rag_prefix: exclusive prefixes over the messages of
//          their chunks, their merge groups (ceil(C_i / 256), none for a
//          one-chunk message) and the messages of more than 256 chunks; the
//          three totals go to a pinned word the host reads;
//   per pass (DEK, then ChaCha20 + CID):
//     k_rag_chunk    one lane per chunk; a one-chunk message is finished
//                    here (ROOT), every other chunk CV goes to cvs;
//     k_rag_merge_a  one workgroup per group of 256 consecutive chunk CVs of
//                    a message (a perfect subtree, except the last); ROOT
//                    here for a message of at most 256 chunks, else the
//                    group's CV goes to gcv;
//     k_rag_merge_b  one workgroup per message of more than 256 chunks: its
//                    <= 64 group CVs, ROOT.
// The prefixes are two-level: `pre` holds, per message, the exclusive prefix
// inside its plan workgroup of 256 messages, the three quantities packed in
// one word (chunks in bits [0, 32), groups in [32, 48), large messages in
// [48, 64): 256 messages of <= 16384 chunks fit); wpre[q] the exclusive
// prefix of quantity q over the plan workgroups, wpre[q][m] its total.
constexpr uint32_t kRagWG = 256;
struct RArgs {
  const uint8_t *src;
  uint8_t *ctext;
  const uint64_t *offs, *lens;
  uint64_t n, lo, hi;
  uint8_t *refs;
  uint32_t key[8];
  uint32_t base;     // kKeyed or 0
  uint32_t out_off;  // 32: the DEK pass, 0: the CID pass
  uint64_t *pre;     // n words
  uint64_t *wpre;    // 3 x (m + 1) words
  uint64_t m;        // plan workgroups: ceil(n / 256)
  uint64_t total;    // items of this launch: chunks, groups or large messages
  uint32_t *cvs;     // 8 words per flattened chunk
  uint32_t *gcv;     // 8 words per merge group
};

__device__ __forceinline__ uint64_t rag_field(uint64_t packed, int q) {
  return q == 0 ? packed & 0xffffffffull : q == 1 ? (packed >> 32) & 0xffffull : packed >> 48;
}
__device__ __forceinline__ bool rag_selected(uint64_t len, uint64_t lo, uint64_t hi) {
  return (lo == ~0ull || len > lo) && len <= hi;  // lo = ~0: from the empty message on
}
__device__ __forceinline__ uint32_t rag_chunks(uint64_t len) {
  return len ? uint32_t((len + 1023) >> 10) : 1u;
}

// Item x (< its total) of quantity q belongs to message i; base = the number
// of q's items before message i.
template <int Q>
__device__ __forceinline__ void rag_find(const RArgs &a, uint64_t x, uint64_t &i,
                                         uint64_t &base) {
  const uint64_t *wp = a.wpre + Q * (a.m + 1);
  uint64_t lo = 0, hi = a.m;  // the last workgroup w with wp[w] <= x
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (wp[mid] <= x) lo = mid; else hi = mid;
  }
  const uint64_t wb = wp[lo], xr = x - wb, i0 = lo * kRagWG;
  const uint64_t *p = a.pre + i0;
  uint32_t l = 0, h = uint32_t(min<uint64_t>(kRagWG, a.n - i0));
  while (h - l > 1) {  // the last message of it with pre <= xr
    const uint32_t mid = (l + h) >> 1;
    if (rag_field(p[mid], Q) <= xr) l = mid; else h = mid;
  }
  i = i0 + l;
  base = wb + rag_field(p[l], Q);
}
// The number of q's items before message i.
template <int Q>
__device__ __forceinline__ uint64_t rag_base(const RArgs &a, uint64_t i) {
  return a.wpre[Q * (a.m + 1) + i / kRagWG] + rag_field(a.pre[i], Q);
}

// Plan, first level: the packed counts of 256 messages, their exclusive
// prefix inside the workgroup, and the workgroup's three totals.  MARK (the
// ragged open, ragged_open_kernels.h): a message that is not selected gets
// the word `mark` at unsel[i] -- it fails closed without being read.
template <bool MARK>
__global__ __launch_bounds__(kRagWG) void k_rag_count(RArgs a, uint32_t *unsel, uint32_t mark) {
  __shared__ uint64_t s[kRagWG];
  const uint32_t t = threadIdx.x;
  const uint64_t i = uint64_t(blockIdx.x) * kRagWG + t;
  uint64_t x = 0;
  if (i < a.n) {
    const uint64_t len = a.lens[i];
    if (rag_selected(len, a.lo, a.hi)) {
      const uint64_t c = rag_chunks(len);
      x = c | ((c > 1 ? (c + 255) >> 8 : 0ull) << 32) | (uint64_t(c > 256) << 48);
    } else if constexpr (MARK) {
      unsel[i] = mark;
    }
  }
  uint64_t v = x;
  s[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kRagWG; d <<= 1) {  // Hillis-Steele inclusive scan
    const uint64_t add = t >= d ? s[t - d] : 0;
    __syncthreads();
    v += add;
    s[t] = v;
    __syncthreads();
  }
  if (i < a.n) a.pre[i] = v - x;
  if (t == kRagWG - 1) {
#pragma unroll
    for (int q = 0; q < 3; ++q) a.wpre[q * (a.m + 1) + blockIdx.x] = rag_field(v, q);
  }
}

// Plan, second level: workgroup q turns wpre[q][0 .. m) into its exclusive
// prefix, T at a time, and stores the total at wpre[q][m] and in the host's
// pinned word q.
template <uint32_t T>
__global__ __launch_bounds__(T) void k_rag_prefix(uint64_t *wpre, uint64_t m,
                                                  uint64_t *host_out) {
  __shared__ uint64_t s[T];
  uint64_t *w = wpre + blockIdx.x * (m + 1);
  uint64_t carry = 0;
  for (uint64_t c0 = 0; c0 < m; c0 += T) {
    const uint64_t i = c0 + threadIdx.x;
    const uint64_t x = i < m ? w[i] : 0;
    uint64_t v = x;
    s[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < T; d <<= 1) {
      const uint64_t add = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
      __syncthreads();
      v += add;
      s[threadIdx.x] = v;
      __syncthreads();
    }
    if (i < m) w[i] = carry + v - x;
    carry += s[T - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    w[m] = carry;
    __hip_atomic_store(host_out + blockIdx.x, carry, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Flattened chunk x for the calling lane (nothing when x >= a.total).  The
// lane hashes its chunk alone, every access bounded by the chunk's own bytes
// inside [off, off + len).  (A staged form for waves of 64 consecutive full
// chunks of one message -- k_pass's G = 1 lane layout through LDS -- was
// built and measured: no gain on the 64 KiB batch; it
// is not kept.)
template <bool CHACHA, int A>
__device__ __forceinline__ void rag_chunk(const RArgs &a, uint64_t x) {
  if (x >= a.total) return;
  uint64_t i, cb;
  rag_find<0>(a, x, i, cb);
  const uint32_t k = uint32_t(x - cb);  // the chunk's number in its message
  const uint64_t off = a.offs[i], len = a.lens[i];
  const uint32_t C = rag_chunks(len);
  const uint8_t *msg = a.src + off;
  uint8_t *cmsg = (CHACHA && a.ctext) ? a.ctext + off : nullptr;
  uint8_t *ref = a.refs + i * 64;
  uint32_t key[8], dek[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) key[w] = a.key[w];
  if constexpr (CHACHA) {  // the DEK pass left it in the ref slot
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(ref + 32);
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = dp[w];
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) dek[w] = 0;
  }
  const bool aligned = ((reinterpret_cast<uintptr_t>(msg) |
                         reinterpret_cast<uintptr_t>(cmsg)) & 15) == 0;
  uint32_t cv[8];
  if (aligned)
    lane_subtree<1, CHACHA, true, A>(cv, msg, cmsg, len, k, 1u, C == 1, key, a.base, dek);
  else
    lane_subtree<1, CHACHA, false, A>(cv, msg, cmsg, len, k, 1u, C == 1, key, a.base, dek);
  if (C == 1) {
    store_digest(ref + a.out_off, cv);
  } else {
    uint4 *q = reinterpret_cast<uint4 *>(a.cvs + x * 8);
    q[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    q[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
  }
}

template <bool CHACHA, int A>
__global__ __launch_bounds__(256) void k_rag_chunk(RArgs a) {
  const uint64_t tiles = (a.total + 255) >> 8;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)  // uniform
    rag_chunk<CHACHA, A>(a, (tile << 8) | threadIdx.x);
}

// Merge level A: workgroup g merges group g's <= 256 chunk CVs.
__global__ __launch_bounds__(256) void k_rag_merge_a(RArgs a) {
  __shared__ uint32_t lds[256 * 8];
  const uint32_t t = threadIdx.x;
  for (uint64_t g = blockIdx.x; g < a.total; g += gridDim.x) {  // uniform
    uint64_t i, gb;
    rag_find<1>(a, g, i, gb);
    const uint32_t C = rag_chunks(a.lens[i]);
    const uint32_t c0 = uint32_t(g - gb) * 256u;
    const uint32_t cnt = min(256u, C - c0);
    const uint64_t cbase = rag_base<0>(a, i) + c0;
    if (t < cnt) {
      const uint4 *q = reinterpret_cast<const uint4 *>(a.cvs + (cbase + t) * 8);
      const uint4 v0 = q[0], v1 = q[1];
      lds[t * 8 + 0] = v0.x; lds[t * 8 + 1] = v0.y; lds[t * 8 + 2] = v0.z; lds[t * 8 + 3] = v0.w;
      lds[t * 8 + 4] = v1.x; lds[t * 8 + 5] = v1.y; lds[t * 8 + 6] = v1.z; lds[t * 8 + 7] = v1.w;
    }
    __syncthreads();
    uint32_t key[8], p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 8; ++w) key[w] = a.key[w];
    tree_reduce_q(lds, cnt, t, key, a.base, C <= 256u, p);
    if (t == 0) {
      if (C <= 256u) {
        store_digest(a.refs + i * 64 + a.out_off, p);
      } else {
#pragma unroll
        for (int w = 0; w < 8; ++w) a.gcv[g * 8 + w] = p[w];
      }
    }
    __syncthreads();  // lds is rewritten by the next group
  }
}

// Merge level B: workgroup b merges the <= 64 group CVs of the b-th message
// of more than 256 chunks.
__global__ __launch_bounds__(256) void k_rag_merge_b(RArgs a) {
  __shared__ uint32_t lds[256 * 8];
  const uint32_t t = threadIdx.x;
  for (uint64_t b = blockIdx.x; b < a.total; b += gridDim.x) {  // uniform
    uint64_t i, bb;
    rag_find<2>(a, b, i, bb);
    const uint32_t C = rag_chunks(a.lens[i]);
    const uint32_t ng = (C + 255u) >> 8;  // <= 64 (kMaxRaggedLen)
    const uint64_t gbase = rag_base<1>(a, i);
    if (t < ng) {
#pragma unroll
      for (int w = 0; w < 8; ++w) lds[t * 8 + w] = a.gcv[(gbase + t) * 8 + w];
    }
    __syncthreads();
    uint32_t key[8], p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 8; ++w) key[w] = a.key[w];
    tree_reduce_q(lds, ng, t, key, a.base, true, p);
    if (t == 0) store_digest(a.refs + i * 64 + a.out_off, p);
    __syncthreads();
  }
}
