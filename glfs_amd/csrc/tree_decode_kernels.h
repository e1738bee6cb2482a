// tree_decode_kernels.h -- a fragment of tree_kernels.hip (included inside
// namespace glfsx, after k_tree_prefix): the inverse of k_tree_len /
// k_tree_prefix / k_tree_write.  The lines of a tree blob in HBM back to the
// encoder's columns, in seven launches whatever n or len:
//
//   k_td_count   each workgroup counts the 0x0A bytes of one kTdSpan-byte span
//   k_tree_prefix  the spans' counts -> exclusive prefix; the total is n
//   k_td_index   the same spans again: the index of every line's '\n'
//   k_td_parse   one lane per line through tree_line.h's grammar: status and
//                decoded name / type lengths, scanned within the workgroup
//   k_tree_prefix x 2  the workgroups' name and type totals
//   k_td_write   one lane per line again: every column, the unescaped
//                strings at their offsets, the NAME and ORDER bits, n_bad
//
// Count and index are two passes over the same bytes, not one pass with a
// look-back chain: HIP promises no dispatch order (k_pass_dc).
// Nothing is written before the write kernel, which first compares the
// totals with the capacities, so a too-small capacity leaves every output
// untouched.  The parse and write kernels stage their workgroup's contiguous
// bytes into an LDS image with 16-byte loads when they fit (kImg), as
// k_tree_write builds its lines there; otherwise the lanes read global bytes.
// Every read of the input is inside [data, data + len): the image's partial
// 16-byte granules are loaded byte by byte, and the grammar never reads at or
// past a line's '\n'.
namespace {

constexpr uint32_t kTdLane = kTdSpan / kTreeWG;  // 64 bytes per lane
static_assert(kTdLane == 64, "one 64-bit newline mask per lane");

struct DArgs {
  const uint8_t *data;
  uint64_t len;
  uint64_t n_cap;
  uint64_t *span_cnt;  // per span: newlines, then (k_tree_prefix) the exclusive prefix
  uint64_t *res;       // n, names_len, types_len, n_bad, tail (TreeDecodeJob)
  uint64_t *ends;      // n_cap: index of line i's '\n'
  uint64_t *lname, *ltype;  // n_cap: inclusive ends of the decoded strings in the workgroup
  uint64_t *wname, *wtype;  // per parse workgroup: totals, then exclusive prefixes
  uint8_t *names;
  uint64_t names_cap;
  uint64_t *name_offs;
  uint32_t *modes;
  uint8_t *types;
  uint64_t types_cap;
  uint64_t *type_offs;
  uint8_t *roots;
  uint64_t *sizes, *block_sizes;
  uint32_t *status;
};

// bit k of the result: byte k of w is 0x0A (exact, no carries between bytes)
__device__ __forceinline__ uint32_t nl_bits(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
  return ((z >> 7) & 1) | ((z >> 14) & 2) | ((z >> 21) & 4) | ((z >> 28) & 8);
}

// The lane's 64 bytes of its span as a mask of newlines.  Spans are cut at
// multiples of kTdSpan from the 16-byte boundary at or below data, so every
// granule is aligned whatever the input's alignment; the granules that
// straddle the input's ends are read byte by byte.  *pos0: the input index
// of the lane's first byte (negative before the input: as int64).
__device__ __forceinline__ uint64_t lane_newlines(const DArgs &a, int64_t *pos0) {
  const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(a.data) & 15);
  const int64_t p0 = int64_t(uint64_t(blockIdx.x) * kTdSpan + threadIdx.x * kTdLane) - mis;
  *pos0 = p0;
  uint64_t m = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t lo = p0 + 16 * g;
    if (lo >= 0 && uint64_t(lo) + 16 <= a.len) {
      const uint4 v = *reinterpret_cast<const uint4 *>(a.data + lo);
      const uint64_t b = nl_bits(v.x) | (nl_bits(v.y) << 4) | (nl_bits(v.z) << 8) |
                         (nl_bits(v.w) << 12);
      m |= b << (16 * g);
    } else {
      for (int k = 0; k < 16; ++k) {
        const int64_t x = lo + k;
        if (x >= 0 && uint64_t(x) < a.len && a.data[x] == '\n') m |= 1ull << (16 * g + k);
      }
    }
  }
  return m;
}

__global__ __launch_bounds__(kTreeWG) void k_td_count(DArgs a) {
  int64_t p0;
  __shared__ uint32_t s[kTreeWG];
  s[threadIdx.x] = uint32_t(__popcll(lane_newlines(a, &p0)));
  __syncthreads();
  for (uint32_t d = kTreeWG / 2; d; d >>= 1) {
    if (threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.span_cnt[blockIdx.x] = s[0];
    if (blockIdx.x == 0) {  // the words the later kernels add to
      const uint64_t tail = a.data[a.len - 1] != '\n';
      a.res[3] = tail;
      a.res[4] = tail;
    }
  }
}

__global__ __launch_bounds__(kTreeWG) void k_td_index(DArgs a) {
  __shared__ uint32_t s[kTreeWG];
  int64_t p0;
  uint64_t m = lane_newlines(a, &p0);
  uint32_t v = uint32_t(__popcll(m));
  const uint32_t own = v;
  s[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t d = 1; d < kTreeWG; d <<= 1) {  // inclusive scan, as k_tree_len
    const uint32_t add = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
    __syncthreads();
    v += add;
    s[threadIdx.x] = v;
    __syncthreads();
  }
  uint64_t r = a.span_cnt[blockIdx.x] + (v - own);  // this lane's first line
  while (m) {
    const int k = __ffsll(static_cast<unsigned long long>(m)) - 1;
    m &= m - 1;
    if (r < a.n_cap) a.ends[r] = uint64_t(p0 + k);
    ++r;
  }
}

typedef const __attribute__((address_space(3))) uint8_t *lds_cp;

__device__ __forceinline__ void hex_words(lds_cp p, uint64_t at, uint32_t w[16]) {
  // 16 bytes at any byte offset (LDS accesses may be unaligned on gfx950)
  typedef const __attribute__((address_space(3))) u32x4_t lds_v4 __attribute__((aligned(1)));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u32x4_t v = *reinterpret_cast<lds_v4 *>(p + uint32_t(at) + 16 * q);
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
}
__device__ __forceinline__ void hex_words(const uint8_t *p, uint64_t at, uint32_t w[16]) {
  tl_load_words(p, at, w, 16);
}

// One line through the grammar, its two hex fields converted several digits
// per instruction sequence (tl_unhex64, the mirror of hex4): true when
// canonical, with *L and the 64-byte root as 16 words.
template <class P>
__device__ bool td_line(P p, uint64_t start, uint64_t end, TlLine *L, uint32_t root[16]) {
  if (!tl_parse(p, start, end, L, false)) return false;
  uint32_t w[16];
  hex_words(p, L->cid_at, w);
  bool ok = tl_unhex64(w, root);
  hex_words(p, L->cid_at + kTlDekAfterCid, w);
  ok &= tl_unhex64(w, root + 8);
  return ok;
}

// What a parse / write workgroup works on: its lines [first, first + cnt) and
// their bytes [b0, b1) (the last '\n' included), staged into img at offset
// sh when they fit.
struct WgLines {
  uint64_t n, first, b0, b1;
  uint32_t cnt, sh;
  bool lds;
};

__device__ __forceinline__ WgLines wg_stage(const DArgs &a, uint4 *img4) {
  WgLines w{};
  const uint64_t n = a.res[0];
  w.n = n <= a.n_cap ? n : 0;  // more lines than the index holds: nothing to do
  w.first = uint64_t(blockIdx.x) * kTreeWG;
  if (w.first >= w.n) return w;
  w.cnt = uint32_t(min<uint64_t>(kTreeWG, w.n - w.first));
  w.b0 = w.first ? a.ends[w.first - 1] + 1 : 0;
  w.b1 = a.ends[w.first + w.cnt - 1] + 1;
  w.sh = uint32_t((reinterpret_cast<uintptr_t>(a.data) + w.b0) & 15);
  w.lds = w.b1 - w.b0 + w.sh <= kImg;
  if (!w.lds) return w;
  // image byte x <-> input byte b0 - sh + x; granules [16g, 16g + 16)
  uint8_t *img = reinterpret_cast<uint8_t *>(img4);
  const uint32_t tot = uint32_t(w.b1 - w.b0) + w.sh;
  const uint32_t ng = (tot + 15) / 16;
  for (uint32_t g = threadIdx.x; g < ng; g += kTreeWG) {
    const uint32_t lo = 16 * g, hi = lo + 16;
    if (lo >= w.sh && hi <= tot) {
      img4[g] = *reinterpret_cast<const uint4 *>(a.data + w.b0 + lo - w.sh);
    } else {
      for (uint32_t x = max(lo, w.sh); x < min(hi, tot); ++x) img[x] = a.data[w.b0 + x - w.sh];
    }
  }
  return w;
}

__global__ __launch_bounds__(kTreeWG) void k_td_parse(DArgs a) {
  __shared__ uint4 img4[kImg / 16];
  const WgLines w = wg_stage(a, img4);
  __syncthreads();
  const uint32_t t = threadIdx.x;
  const uint64_t i = w.first + t;
  uint64_t nl = 0, tl = 0;
  if (t < w.cnt) {
    const uint64_t start = t ? a.ends[i - 1] + 1 : w.b0, end = a.ends[i];
    TlLine L{};
    uint32_t root[16];
    bool ok;
    if (w.lds) {
      const uint64_t o = w.sh - w.b0;  // input index -> image index
      ok = td_line((lds_cp)img4, start + o, end + o, &L, root);
    } else {
      ok = td_line(a.data, start, end, &L, root);
    }
    if (ok) {
      nl = L.name_len;
      tl = L.type_len;
    }
  }
  __syncthreads();  // the image is done with: its memory holds the two scans
  uint64_t *s1 = reinterpret_cast<uint64_t *>(img4), *s2 = s1 + kTreeWG;
  s1[t] = nl;
  s2[t] = tl;
  __syncthreads();
  for (uint32_t d = 1; d < kTreeWG; d <<= 1) {
    const uint64_t a1 = t >= d ? s1[t - d] : 0, a2 = t >= d ? s2[t - d] : 0;
    __syncthreads();
    nl += a1;
    tl += a2;
    s1[t] = nl;
    s2[t] = tl;
    __syncthreads();
  }
  if (t < w.cnt) {
    a.lname[i] = nl;
    a.ltype[i] = tl;
  }
  if (t == kTreeWG - 1) {
    a.wname[blockIdx.x] = nl;
    a.wtype[blockIdx.x] = tl;
  }
}

template <class P>
__device__ __forceinline__ void td_strings(const DArgs &a, P p, const TlLine &L, bool have_prev,
                                           uint64_t prev_name_at, uint8_t *name_out,
                                           uint8_t *type_out, uint32_t *st) {
  *st |= tl_name_bits(p, L.name_at, a.data, prev_name_at, have_prev, name_out);
  if (type_out) {
    TlUnescape<P> u(p, L.type_at);
    for (int c; (c = u.next()) >= 0;) *type_out++ = uint8_t(c);
  }
}

__global__ __launch_bounds__(kTreeWG) void k_td_write(DArgs a) {
  __shared__ uint4 img4[kImg / 16];
  __shared__ uint8_t s_bad[kTreeWG];
  const WgLines w = wg_stage(a, img4);
  __syncthreads();
  const uint32_t t = threadIdx.x;
  const uint64_t i = w.first + t;
  const uint64_t ntot = a.res[1], ttot = a.res[2];
  // uniform: with a capacity too small nothing is written (the host reports it)
  const bool wr = a.res[0] <= a.n_cap && (!a.names || ntot <= a.names_cap) &&
                  (!a.types || ttot <= a.types_cap);
  if (wr && a.res[0] == 0 && blockIdx.x == 0 && t == 0) {
    if (a.name_offs) a.name_offs[0] = 0;
    if (a.type_offs) a.type_offs[0] = 0;
  }
  TlLine L{};
  uint32_t root[16];
  uint32_t st = 0;
  if (t < w.cnt) {
    const uint64_t start = t ? a.ends[i - 1] + 1 : w.b0, end = a.ends[i];
    bool ok;
    if (w.lds) {
      const uint64_t o = w.sh - w.b0;  // input index -> image index
      ok = td_line((lds_cp)img4, start + o, end + o, &L, root);
    } else {
      ok = td_line(a.data, start, end, &L, root);
    }
    if (!ok) {
      st = 1;  // GLFSX_TREE_NONCANON: empty strings, zero columns
      L = TlLine{};
      for (int k = 0; k < 16; ++k) root[k] = 0;
    }
  }
  s_bad[t] = uint8_t(st);
  __syncthreads();
  if (t < w.cnt) {
    const uint64_t noff = a.wname[blockIdx.x] + (t ? a.lname[i - 1] : 0);
    const uint64_t toff = a.wtype[blockIdx.x] + (t ? a.ltype[i - 1] : 0);
    if (!st) {
      // the line before: lane t - 1's, or the previous workgroup's last
      // line, read again from the source
      bool have_prev = false;
      uint64_t prev_at = 0;
      if (i) {
        const uint64_t pe = a.ends[i - 1], ps = i > 1 ? a.ends[i - 2] + 1 : 0;
        if (t) {
          have_prev = !s_bad[t - 1];
        } else {
          TlLine PL{};
          uint32_t pr[16];
          have_prev = td_line(a.data, ps, pe, &PL, pr);
        }
        prev_at = ps + 9;  // past `{"name":"`
      }
      uint8_t *no = (wr && a.names) ? a.names + noff : nullptr;
      uint8_t *to = (wr && a.types) ? a.types + toff : nullptr;
      if (w.lds)
        td_strings(a, (lds_cp)img4, L, have_prev, prev_at, no, to, &st);
      else
        td_strings(a, a.data, L, have_prev, prev_at, no, to, &st);
    }
    if (wr) {
      if (a.name_offs) {
        a.name_offs[i] = noff;
        if (i + 1 == w.n) a.name_offs[w.n] = ntot;
      }
      if (a.type_offs) {
        a.type_offs[i] = toff;
        if (i + 1 == w.n) a.type_offs[w.n] = ttot;
      }
      if (a.modes) a.modes[i] = L.mode;
      if (a.sizes) a.sizes[i] = L.size;
      if (a.block_sizes) a.block_sizes[i] = L.block_size;
      if (a.status) a.status[i] = st;
      if (a.roots) {
        uint8_t *r = a.roots + 64 * i;
        if ((reinterpret_cast<uintptr_t>(a.roots) & 15) == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            reinterpret_cast<uint4 *>(r)[q] =
                uint4{root[4 * q], root[4 * q + 1], root[4 * q + 2], root[4 * q + 3]};
        } else {
#pragma unroll
          for (int k = 0; k < 16; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) r[4 * k + q] = uint8_t(root[k] >> (8 * q));
        }
      }
    }
  }
  const int bad = __syncthreads_count(st != 0);
  if (t == 0 && bad)
    atomicAdd(reinterpret_cast<unsigned long long *>(a.res + 3), static_cast<unsigned long long>(bad));
}

DArgs decode_args(const TreeDecodeJob &j) {
  DArgs a{};
  a.data = j.data;
  a.len = j.len;
  a.n_cap = j.n_cap;
  const uint64_t spans = tree_decode_spans(j.data, j.len), wgs = tree_decode_wgs(j.n_cap);
  uint64_t *s = j.scratch;
  a.res = s; s += 8;
  a.span_cnt = s; s += spans;
  a.wname = s; s += wgs;
  a.wtype = s; s += wgs;
  a.ends = s; s += j.n_cap;
  a.lname = s; s += j.n_cap;
  a.ltype = s;
  a.names = j.names;
  a.names_cap = j.names_cap;
  a.name_offs = j.name_offs;
  a.modes = j.modes;
  a.types = j.types;
  a.types_cap = j.types_cap;
  a.type_offs = j.type_offs;
  a.roots = j.roots;
  a.sizes = j.sizes;
  a.block_sizes = j.block_sizes;
  a.status = j.status;
  return a;
}

}  // namespace

hipError_t launch_tree_decode(const TreeDecodeJob &j, hipStream_t s) {
  if (j.len == 0 || j.n_cap == 0) return hipErrorInvalidValue;
  const DArgs a = decode_args(j);
  const uint32_t spans = uint32_t(tree_decode_spans(j.data, j.len));
  const uint32_t wgs = uint32_t(tree_decode_wgs(j.n_cap));
  uint64_t *const none = nullptr;
#define TD_LAUNCH(...)                               \
  do {                                               \
    hipLaunchKernelGGL(__VA_ARGS__);                 \
    const hipError_t e = hipGetLastError();          \
    if (e != hipSuccess) return e;                   \
  } while (0)
  TD_LAUNCH(k_td_count, dim3(spans), dim3(kTreeWG), 0, s, a);
  TD_LAUNCH(k_tree_prefix<1024>, dim3(1), dim3(1024), 0, s, a.span_cnt, uint64_t(spans),
            a.res + 0, 0u, none);
  TD_LAUNCH(k_td_index, dim3(spans), dim3(kTreeWG), 0, s, a);
  TD_LAUNCH(k_td_parse, dim3(wgs), dim3(kTreeWG), 0, s, a);
  TD_LAUNCH(k_tree_prefix<1024>, dim3(1), dim3(1024), 0, s, a.wname, uint64_t(wgs), a.res + 1,
            0u, none);
  TD_LAUNCH(k_tree_prefix<1024>, dim3(1), dim3(1024), 0, s, a.wtype, uint64_t(wgs), a.res + 2,
            0u, none);
  TD_LAUNCH(k_td_write, dim3(wgs), dim3(kTreeWG), 0, s, a);
#undef TD_LAUNCH
  return hipSuccess;
}
