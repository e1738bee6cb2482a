// b3_arx.h -- BLAKE3 and ChaCha20 primitives of the post kernels: the message
// schedule, the ARX forms (compiler-scheduled C, one asm statement per
// instruction in quarter-round order, asm step-interleaved), b3_round /
// b3_compress, chacha_block, and load_block / store_block / mask_tail.
// A fragment of the post_kernels.hip translation unit, included there in
// order inside its namespace; not a stand-alone header.

struct Sched {
  int s[7][16];
};
constexpr Sched make_sched() {
  constexpr int perm[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  Sched t{};
  for (int i = 0; i < 16; ++i) t.s[0][i] = i;
  for (int r = 1; r < 7; ++r)
    for (int i = 0; i < 16; ++i) t.s[r][i] = t.s[r - 1][perm[i]];
  return t;
}
constexpr Sched kSched = make_sched();

__device__ __forceinline__ uint32_t rotr(uint32_t x, uint32_t n) {
  return __builtin_amdgcn_alignbit(x, x, n);
}

// ARX steps as single-instruction asm statements: same instructions as the
// C form, but the compiler schedules them as opaque units, which on gfx950
// issues measurably faster (DESIGN.md "Rooflines", tools/arx.hip).  Used
// from the second round on, so round 1 keeps the C form's constant folding
// (IV literals, uniform key words).
template <int N>
__device__ __forceinline__ uint32_t rotr_a(uint32_t x) {
  uint32_t d;
  asm("v_alignbit_b32 %0, %1, %1, %2" : "=v"(d) : "v"(x), "i"(N));
  return d;
}
__device__ __forceinline__ uint32_t xor_a(uint32_t a, uint32_t b) {
  uint32_t d;
  asm("v_xor_b32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ uint32_t add_a(uint32_t a, uint32_t b) {
  uint32_t d;
  asm("v_add_u32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ uint32_t add3_a(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t d;
  asm("v_add3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

#define B3G_A(a, b, c, d, x, y)       \
  a = add3_a(a, b, (x));              \
  d = rotr_a<16>(xor_a(d, a));        \
  c = add_a(c, d);                    \
  b = rotr_a<12>(xor_a(b, c));        \
  a = add3_a(a, b, (y));              \
  d = rotr_a<8>(xor_a(d, a));         \
  c = add_a(c, d);                    \
  b = rotr_a<7>(xor_a(b, c));

#define CQR_A(a, b, c, d)             \
  a = add_a(a, b);                    \
  d = rotr_a<16>(xor_a(d, a));        \
  c = add_a(c, d);                    \
  b = rotr_a<20>(xor_a(b, c));        \
  a = add_a(a, b);                    \
  d = rotr_a<24>(xor_a(d, a));        \
  c = add_a(c, d);                    \
  b = rotr_a<25>(xor_a(b, c));

#define B3G_C(a, b, c, d, x, y) \
  a = a + b + (x);            \
  d = rotr(d ^ a, 16);        \
  c = c + d;                  \
  b = rotr(b ^ c, 12);        \
  a = a + b + (y);            \
  d = rotr(d ^ a, 8);         \
  c = c + d;                  \
  b = rotr(b ^ c, 7);

#define B3G(a, b, c, d, x, y)           \
  if constexpr (R == 0 || !A) {         \
    B3G_C(a, b, c, d, x, y)             \
  } else {                              \
    B3G_A(a, b, c, d, x, y)             \
  }

// Step-interleaved form: the ARX rounds of the many-wave kernels written
// step by step over all independent chains of a half-round (4 G or 4 QR; 8
// when a BLAKE3 round is fused with a ChaCha20 double round), with a
// scheduling barrier after each step, so the compiler cannot serialise the
// chains: two dependent instructions are always at least 3 (7 fused)
// independent ones apart.  Each step is one asm statement per instruction
// (measured +2.5% config 2, +1-2% small blobs and read side; the same steps
// in compiler-visible C were 5.7% slower; that alternate is in git history).
// The kernels take the form as their int template parameter A (0 = compiler-
// scheduled C, 1 = asm in quarter-round order, 2 = asm step-interleaved);
// the headline's CID pass runs form 1 (launch_plan.h pass_rec).
#define SB() __builtin_amdgcn_sched_barrier(0)
constexpr int kCol[4][4] = {{0, 4, 8, 12}, {1, 5, 9, 13}, {2, 6, 10, 14}, {3, 7, 11, 15}};
constexpr int kDia[4][4] = {{0, 5, 10, 15}, {1, 6, 11, 12}, {2, 7, 8, 13}, {3, 4, 9, 14}};

// One half-round, 12 steps: B3 (if G) = 4 BLAKE3 G's on v with message words
// m[s[mo + 2k]], m[s[mo + 2k + 1]]; Q (if Q) = 4 ChaCha20 quarter-rounds on x.
template <bool DIAG, int R, bool G, bool Q>
__device__ __forceinline__ void half_il(uint32_t (&v)[16], const uint32_t (&m)[16],
                                        uint32_t (&x)[16]) {
  constexpr const int (*I)[4] = DIAG ? kDia : kCol;
  constexpr const int *s = kSched.s[R];
  constexpr int mo = DIAG ? 8 : 0;
#define IL_STEP(gstmt, qstmt)                        \
  _Pragma("unroll") for (int k = 0; k < 4; ++k) {    \
    if constexpr (G) { gstmt; }                      \
    if constexpr (Q) { qstmt; }                      \
  }                                                  \
  SB();
#define VA v[I[k][0]]
#define VB v[I[k][1]]
#define VC v[I[k][2]]
#define VD v[I[k][3]]
#define XA x[I[k][0]]
#define XB x[I[k][1]]
#define XC x[I[k][2]]
#define XD x[I[k][3]]
  IL_STEP(VA = add3_a(VA, VB, m[s[mo + 2 * k]]), XA = add_a(XA, XB))
  IL_STEP(VD = xor_a(VD, VA), XD = xor_a(XD, XA))
  IL_STEP(VD = rotr_a<16>(VD), XD = rotr_a<16>(XD))
  IL_STEP(VC = add_a(VC, VD), XC = add_a(XC, XD))
  IL_STEP(VB = xor_a(VB, VC), XB = xor_a(XB, XC))
  IL_STEP(VB = rotr_a<12>(VB), XB = rotr_a<20>(XB))
  IL_STEP(VA = add3_a(VA, VB, m[s[mo + 2 * k + 1]]), XA = add_a(XA, XB))
  IL_STEP(VD = xor_a(VD, VA), XD = xor_a(XD, XA))
  IL_STEP(VD = rotr_a<8>(VD), XD = rotr_a<24>(XD))
  IL_STEP(VC = add_a(VC, VD), XC = add_a(XC, XD))
  IL_STEP(VB = xor_a(VB, VC), XB = xor_a(XB, XC))
  IL_STEP(VB = rotr_a<7>(VB), XB = rotr_a<25>(XB))
#undef VA
#undef VB
#undef VC
#undef VD
#undef XA
#undef XB
#undef XC
#undef XD
#undef IL_STEP
}

template <int R, int A = 2>
__device__ __forceinline__ void b3_round(uint32_t (&v)[16],
                                         const uint32_t (&m)[16]) {
  if constexpr (A == 2 && R > 0) {
    uint32_t x[16];
    half_il<false, R, true, false>(v, m, x);
    half_il<true, R, true, false>(v, m, x);
    return;
  }
  constexpr const int *s = kSched.s[R];
  B3G(v[0], v[4], v[8], v[12], m[s[0]], m[s[1]]);
  B3G(v[1], v[5], v[9], v[13], m[s[2]], m[s[3]]);
  B3G(v[2], v[6], v[10], v[14], m[s[4]], m[s[5]]);
  B3G(v[3], v[7], v[11], v[15], m[s[6]], m[s[7]]);
  B3G(v[0], v[5], v[10], v[15], m[s[8]], m[s[9]]);
  B3G(v[1], v[6], v[11], v[12], m[s[10]], m[s[11]]);
  B3G(v[2], v[7], v[8], v[13], m[s[12]], m[s[13]]);
  B3G(v[3], v[4], v[9], v[14], m[s[14]], m[s[15]]);
}

// cv <- first 8 words of compress(cv, m, counter, block_len, flags): the
// chaining value, or for a ROOT compression the first 32 output bytes
// (XOF block 0), which is all the write path ever reads.
template <int A = 2>
__device__ __forceinline__ void b3_compress(uint32_t (&cv)[8],
                                            const uint32_t (&m)[16],
                                            uint32_t ctr_lo, uint32_t ctr_hi,
                                            uint32_t blen, uint32_t flags) {
  uint32_t v[16] = {cv[0],  cv[1],  cv[2],  cv[3],  cv[4],  cv[5],
                    cv[6],  cv[7],  kIV[0], kIV[1], kIV[2], kIV[3],
                    ctr_lo, ctr_hi, blen,   flags};
  b3_round<0, A>(v, m);
  b3_round<1, A>(v, m);
  b3_round<2, A>(v, m);
  b3_round<3, A>(v, m);
  b3_round<4, A>(v, m);
  b3_round<5, A>(v, m);
  b3_round<6, A>(v, m);
#pragma unroll
  for (int i = 0; i < 8; ++i) cv[i] = v[i] ^ v[i + 8];
}

#define CQR(a, b, c, d) \
  a += b;               \
  d = rotr(d ^ a, 16);  \
  c += d;               \
  b = rotr(b ^ c, 20);  \
  a += b;               \
  d = rotr(d ^ a, 24);  \
  c += d;               \
  b = rotr(b ^ c, 25);

// RFC 8439 block function, nonce 0^12 (ref.go:138), 32-bit block counter.
template <int A = 2>
__device__ __forceinline__ void chacha_block(uint32_t (&x)[16],
                                             const uint32_t (&k)[8],
                                             uint32_t ctr) {
  constexpr uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u,
                     c3 = 0x6b206574u;
  x[0] = c0;
  x[1] = c1;
  x[2] = c2;
  x[3] = c3;
#pragma unroll
  for (int i = 0; i < 8; ++i) x[4 + i] = k[i];
  x[12] = ctr;
  x[13] = 0;
  x[14] = 0;
  x[15] = 0;
  // round 1 in C: its key-only quarter-rounds are uniform and hoisted
  CQR(x[0], x[4], x[8], x[12]);
  CQR(x[1], x[5], x[9], x[13]);
  CQR(x[2], x[6], x[10], x[14]);
  CQR(x[3], x[7], x[11], x[15]);
  CQR(x[0], x[5], x[10], x[15]);
  CQR(x[1], x[6], x[11], x[12]);
  CQR(x[2], x[7], x[8], x[13]);
  CQR(x[3], x[4], x[9], x[14]);
#pragma unroll
  for (int i = 1; i < 10; ++i) {
   if constexpr (A == 2) {
    uint32_t v[16], m[16];
    half_il<false, 0, false, true>(v, m, x);
    half_il<true, 0, false, true>(v, m, x);
    continue;
   }
   if constexpr (A) {
    CQR_A(x[0], x[4], x[8], x[12]);
    CQR_A(x[1], x[5], x[9], x[13]);
    CQR_A(x[2], x[6], x[10], x[14]);
    CQR_A(x[3], x[7], x[11], x[15]);
    CQR_A(x[0], x[5], x[10], x[15]);
    CQR_A(x[1], x[6], x[11], x[12]);
    CQR_A(x[2], x[7], x[8], x[13]);
    CQR_A(x[3], x[4], x[9], x[14]);
   } else {
    CQR(x[0], x[4], x[8], x[12]);
    CQR(x[1], x[5], x[9], x[13]);
    CQR(x[2], x[6], x[10], x[14]);
    CQR(x[3], x[7], x[11], x[15]);
    CQR(x[0], x[5], x[10], x[15]);
    CQR(x[1], x[6], x[11], x[12]);
    CQR(x[2], x[7], x[8], x[13]);
    CQR(x[3], x[4], x[9], x[14]);
   }
  }
  x[0] += c0;
  x[1] += c1;
  x[2] += c2;
  x[3] += c3;
#pragma unroll
  for (int i = 0; i < 8; ++i) x[4 + i] += k[i];
  x[12] += ctr;
}

// 64-byte message block at p with `avail` valid bytes (zero padded).
template <bool ALIGNED>
__device__ __forceinline__ void load_block(uint32_t (&m)[16], const uint8_t *p,
                                           uint32_t avail) {
  if (ALIGNED && avail >= 64) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    uint4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    m[0] = w0.x; m[1] = w0.y; m[2] = w0.z; m[3] = w0.w;
    m[4] = w1.x; m[5] = w1.y; m[6] = w1.z; m[7] = w1.w;
    m[8] = w2.x; m[9] = w2.y; m[10] = w2.z; m[11] = w2.w;
    m[12] = w3.x; m[13] = w3.y; m[14] = w3.z; m[15] = w3.w;
  } else {
    const uint32_t lim = avail < 64 ? avail : 64;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t idx = 4 * i + b;
        if (idx < lim) w |= uint32_t(p[idx]) << (8 * b);
      }
      m[i] = w;
    }
  }
}

template <bool ALIGNED>
__device__ __forceinline__ void store_block(uint8_t *p, const uint32_t (&c)[16],
                                            uint32_t avail) {
  if (ALIGNED && avail >= 64) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(c[0], c[1], c[2], c[3]);
    q[1] = make_uint4(c[4], c[5], c[6], c[7]);
    q[2] = make_uint4(c[8], c[9], c[10], c[11]);
    q[3] = make_uint4(c[12], c[13], c[14], c[15]);
  } else {
    const uint32_t lim = avail < 64 ? avail : 64;
    for (uint32_t idx = 0; idx < lim; ++idx)
      p[idx] = uint8_t(c[idx >> 2] >> (8 * (idx & 3)));
  }
}

// Zero the bytes of m at and beyond `avail` (only called when avail < 64).
__device__ __forceinline__ void mask_tail(uint32_t (&m)[16], uint32_t avail) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t lo = 4 * i;
    uint32_t keep;
    if (lo + 4 <= avail) keep = 0xffffffffu;
    else if (lo >= avail) keep = 0u;
    else keep = (1u << (8 * (avail - lo))) - 1u;
    m[i] &= keep;
  }
}
