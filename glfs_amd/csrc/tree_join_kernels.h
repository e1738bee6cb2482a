// tree_join_kernels.h -- a fragment of tree_kernels.hip (included inside
// namespace glfsx, after k_tree_prefix): the two primitives of the
// tree-to-tree operations (compare.go, reduce.go, filter.go) over the
// decoder's columns.
//
//   k_tree_join   one launch: one lane per entry of A and of B.  Each runs
//                 tree_join.h's lower bound over the other side's names and
//                 writes its own match (and A's lanes the pair's class): no
//                 atomics, no scatter, nothing shared between lanes.  A lane's
//                 search is ~log2(n) dependent steps of two offset loads and a
//                 name compare; the first steps of every lane probe the same
//                 few entries, which stay in the caches.
//   k_ts_len / k_tree_prefix x 2 / k_ts_write   the select: output entry t is
//                 entry sel[t] of A or entry -1 - sel[t] of B.  The lengths of
//                 the selected strings are scanned within the workgroup, the
//                 workgroups' totals by k_tree_prefix (as the encoder's and
//                 the decoder's), and the write kernel copies every column.
//                 A sel value that names no entry is flagged by k_ts_len in
//                 scratch; k_ts_write checks that flag and the capacities
//                 before it writes anything.
//
// Names are read as tree_join.h says: eight bytes at a time from any byte
// offset while eight are left, single bytes after that, never at or past a
// name's end.  The copies of the select do the same.
namespace {

struct JArgs {
  TreeCols a, b;
  int64_t *a_match, *b_match;
  uint8_t *a_class;
};

__global__ __launch_bounds__(kTreeWG) void k_tree_join(JArgs j) {
  const uint64_t g = uint64_t(blockIdx.x) * kTreeWG + threadIdx.x;
  const bool in_a = g < j.a.n;
  const uint64_t i = in_a ? g : g - j.a.n;
  if (!in_a && i >= j.b.n) return;
  const TreeCols x = in_a ? j.a : j.b, y = in_a ? j.b : j.a;  // mine, the other side
  int64_t *match = in_a ? j.a_match : j.b_match;
  uint8_t *cls = in_a ? j.a_class : nullptr;
  if (!match && !cls) return;
  const uint64_t at = x.name_offs[i];
  const int64_t m = tj_find(y.names, y.name_offs, y.n, x.names + at, x.name_offs[i + 1] - at);
  if (match) match[i] = m;
  if (!cls) return;
  uint8_t c = kJoinOnly;
  if (m >= 0) {
    const uint64_t ta = x.type_offs[i], tb = y.type_offs[m];
    c = tj_class(x.types + ta, x.type_offs[i + 1] - ta, x.roots + 64 * i, x.sizes[i],
                 x.block_sizes[i], y.types + tb, y.type_offs[m + 1] - tb, y.roots + 64 * uint64_t(m),
                 y.sizes[m], y.block_sizes[m]);
  }
  cls[i] = c;
}

struct SArgs {
  TreeCols a, b;
  const int64_t *sel;
  uint64_t k;
  uint64_t *res;            // bytes of names, bytes of types, bad sel flag
  uint64_t *wname, *wtype;  // per workgroup: totals, then exclusive prefixes
  uint64_t *lname, *ltype;  // k: inclusive ends within the workgroup
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

// Output entry t's source: the side and the index there; false when sel[t]
// names no entry (nothing of either side may be read then).
__device__ __forceinline__ bool ts_pick(const SArgs &a, uint64_t t, TreeCols *c, uint64_t *idx) {
  const int64_t v = a.sel[t];
  *c = v >= 0 ? a.a : a.b;
  *idx = v >= 0 ? uint64_t(v) : uint64_t(-1 - v);
  return *idx < c->n;
}

__device__ __forceinline__ void ts_copy(uint8_t *dst, const uint8_t *src, uint64_t n) {
  uint64_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    __builtin_memcpy(&w, src + i, 8);
    __builtin_memcpy(dst + i, &w, 8);
  }
  for (; i < n; ++i) dst[i] = src[i];
}

__global__ __launch_bounds__(kTreeWG) void k_ts_len(SArgs a) {
  __shared__ uint64_t s1[kTreeWG], s2[kTreeWG];
  const uint32_t t = threadIdx.x;
  const uint64_t i = uint64_t(blockIdx.x) * kTreeWG + t;
  uint64_t nl = 0, tl = 0;
  if (i < a.k) {
    TreeCols c;
    uint64_t idx;
    if (ts_pick(a, i, &c, &idx)) {
      nl = c.name_offs[idx + 1] - c.name_offs[idx];
      tl = c.type_offs[idx + 1] - c.type_offs[idx];
    } else {
      a.res[2] = 1;  // every such lane stores the same word
    }
  }
  s1[t] = nl;
  s2[t] = tl;
  __syncthreads();
  for (uint32_t d = 1; d < kTreeWG; d <<= 1) {  // inclusive scans, as k_td_parse
    const uint64_t a1 = t >= d ? s1[t - d] : 0, a2 = t >= d ? s2[t - d] : 0;
    __syncthreads();
    nl += a1;
    tl += a2;
    s1[t] = nl;
    s2[t] = tl;
    __syncthreads();
  }
  if (i < a.k) {
    a.lname[i] = nl;
    a.ltype[i] = tl;
  }
  if (t == kTreeWG - 1) {
    a.wname[blockIdx.x] = nl;
    a.wtype[blockIdx.x] = tl;
  }
}

__global__ __launch_bounds__(kTreeWG) void k_ts_write(SArgs a) {
  const uint64_t ntot = a.res[0], ttot = a.res[1];
  // uniform: a bad sel value or a capacity too small, and nothing is written
  // (the host reports it)
  if (a.res[2] || (a.names && ntot > a.names_cap) || (a.types && ttot > a.types_cap)) return;
  const uint32_t t = threadIdx.x;
  const uint64_t i = uint64_t(blockIdx.x) * kTreeWG + t;
  if (i >= a.k) return;
  TreeCols c;
  uint64_t idx;
  if (!ts_pick(a, i, &c, &idx)) return;  // (flagged: not reached)
  const uint64_t noff = a.wname[blockIdx.x] + (t ? a.lname[i - 1] : 0);
  const uint64_t toff = a.wtype[blockIdx.x] + (t ? a.ltype[i - 1] : 0);
  const uint64_t ns = c.name_offs[idx], ts = c.type_offs[idx];
  if (a.names) ts_copy(a.names + noff, c.names + ns, c.name_offs[idx + 1] - ns);
  if (a.types) ts_copy(a.types + toff, c.types + ts, c.type_offs[idx + 1] - ts);
  if (a.name_offs) {
    a.name_offs[i] = noff;
    if (i + 1 == a.k) a.name_offs[a.k] = ntot;
  }
  if (a.type_offs) {
    a.type_offs[i] = toff;
    if (i + 1 == a.k) a.type_offs[a.k] = ttot;
  }
  if (a.modes) a.modes[i] = c.modes[idx];
  if (a.sizes) a.sizes[i] = c.sizes[idx];
  if (a.block_sizes) a.block_sizes[i] = c.block_sizes[idx];
  if (a.status) a.status[i] = c.status ? c.status[idx] : 0u;
  if (a.roots) ts_copy(a.roots + 64 * i, c.roots + 64 * idx, 64);
}

}  // namespace

hipError_t launch_tree_join(const TreeJoinJob &j, hipStream_t s) {
  const uint64_t lanes = j.a.n + j.b.n;
  if (lanes == 0) return hipSuccess;
  const uint64_t wgs = (lanes + kTreeWG - 1) / kTreeWG;
  if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const JArgs a{j.a, j.b, j.a_match, j.b_match, j.a_class};
  hipLaunchKernelGGL(k_tree_join, dim3(uint32_t(wgs)), dim3(kTreeWG), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tree_select(const TreeSelectJob &j, hipStream_t s) {
  if (j.k == 0) return hipErrorInvalidValue;
  const uint64_t wgs = (j.k + kTreeWG - 1) / kTreeWG;
  if (wgs > 0x7FFFFFFFull) return hipErrorInvalidValue;
  SArgs a{};
  a.a = j.a;
  a.b = j.b;
  a.sel = j.sel;
  a.k = j.k;
  uint64_t *p = j.scratch;
  a.res = p; p += 8;
  a.wname = p; p += wgs;
  a.wtype = p; p += wgs;
  a.lname = p; p += j.k;
  a.ltype = p;
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
  uint64_t *const none = nullptr;
#define TS_LAUNCH(...)                               \
  do {                                               \
    hipLaunchKernelGGL(__VA_ARGS__);                 \
    const hipError_t e = hipGetLastError();          \
    if (e != hipSuccess) return e;                   \
  } while (0)
  TS_LAUNCH(k_ts_len, dim3(uint32_t(wgs)), dim3(kTreeWG), 0, s, a);
  TS_LAUNCH(k_tree_prefix<1024>, dim3(1), dim3(1024), 0, s, a.wname, wgs, a.res + 0, 0u, none);
  TS_LAUNCH(k_tree_prefix<1024>, dim3(1), dim3(1024), 0, s, a.wtype, wgs, a.res + 1, 0u, none);
  if (j.write) TS_LAUNCH(k_ts_write, dim3(uint32_t(wgs)), dim3(kTreeWG), 0, s, a);
#undef TS_LAUNCH
  return hipSuccess;
}
