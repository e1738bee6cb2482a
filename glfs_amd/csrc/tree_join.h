// tree_join.h -- matching the entries of two trees by name, defined once.
//
// The reference's tree-to-tree operations (compare.go:52-124, and reduce.go
// and filter.go after it) all look every entry of one sorted tree up in
// another with Lookup (tree.go:22-30: a binary search by strings.Compare).
// Here that is three pure functions over the decoder's columns:
//
//   tj_compare      strings.Compare of two names: unsigned bytes, and a proper
//                   prefix sorts first
//   tj_lower_bound  the first entry of a name column (names, offs, n) whose
//                   name is not below the key
//   tj_class        what a matched pair is to Compare: two trees, the same
//                   object, or different ones
//
// No HIP includes: the host join (tree.cpp glfsx_tree_join) and the kernel
// (tree_join_kernels.h) both call these, so they cannot disagree.  P is any
// byte pointer (`const uint8_t *` in any address space).
//
// Loads.  Names start at arbitrary byte offsets.  tj_compare takes them eight
// bytes at a time while both names have eight bytes left -- a copy of eight
// bytes from an unaligned address, which gfx950 serves with one load -- and
// orders the two words as big-endian numbers, which is the order of their
// bytes; what is left (fewer than eight bytes of the shorter name) is read
// byte by byte.  So every read of a name is at an index below its length:
// nothing outside [names, names + offs[n]) is touched, whatever the
// alignment.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TJ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TJ_HD inline
#endif

namespace glfsx {

// a_class of glfsx_tree_join (GLFSX_JOIN_* in include/glfsx.h)
constexpr uint8_t kJoinOnly = 0, kJoinTrees = 1, kJoinSame = 2, kJoinDiff = 3;

// the eight bytes at p as a number whose order is the bytes' order
template <class P>
TJ_HD uint64_t tj_load_be64(P p) {
  uint64_t w;
  __builtin_memcpy(&w, &p[0], 8);
#if __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
  w = __builtin_bswap64(w);
#endif
  return w;
}

// strings.Compare(a[0..an), b[0..bn)): -1, 0 or 1
template <class P>
TJ_HD int tj_compare(P a, uint64_t an, P b, uint64_t bn) {
  const uint64_t m = an < bn ? an : bn;
  uint64_t i = 0;
  for (; i + 8 <= m; i += 8) {
    const uint64_t x = tj_load_be64(a + i), y = tj_load_be64(b + i);
    if (x != y) return x < y ? -1 : 1;
  }
  for (; i < m; ++i) {
    const uint32_t x = uint8_t(a[i]), y = uint8_t(b[i]);
    if (x != y) return x < y ? -1 : 1;
  }
  return an < bn ? -1 : (an > bn ? 1 : 0);
}

// The first i in [0, n] with name i >= key (n: every name is below it).
// Terminates after at most 64 steps and returns an index in [0, n] whatever
// the order of the names.
template <class P>
TJ_HD uint64_t tj_lower_bound(P names, const uint64_t *offs, uint64_t n, P key, uint64_t key_len) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    const uint64_t at = offs[mid];
    if (tj_compare(names + at, offs[mid + 1] - at, key, key_len) < 0)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The index in (names, offs, n) of the entry named key, or -1.
template <class P>
TJ_HD int64_t tj_find(P names, const uint64_t *offs, uint64_t n, P key, uint64_t key_len) {
  const uint64_t i = tj_lower_bound(names, offs, n, key, key_len);
  if (i >= n) return -1;
  const uint64_t at = offs[i];
  return tj_compare(names + at, offs[i + 1] - at, key, key_len) == 0 ? int64_t(i) : -1;
}

template <class P>
TJ_HD bool tj_is_tree(P t, uint64_t n) {
  return n == 4 && t[0] == 't' && t[1] == 'r' && t[2] == 'e' && t[3] == 'e';
}

// The 64 bytes at a and at b (CID || DEK) are equal.
template <class P>
TJ_HD bool tj_ref_equal(P a, P b) {
  uint64_t d = 0;
  for (int k = 0; k < 64; k += 8) d |= tj_load_be64(a + k) ^ tj_load_be64(b + k);
  return d == 0;
}

// The class of a matched pair: both types exactly "tree" -> kJoinTrees;
// equal types and equal CID, DEK, size and block size (glfs.go:44-46 Ref
// .Equals, blob.go:27-29 Root.Equals) -> kJoinSame; anything else, differing
// types included -> kJoinDiff.
template <class P>
TJ_HD uint8_t tj_class(P a_type, uint64_t a_type_len, P a_root, uint64_t a_size, uint64_t a_bs,
                       P b_type, uint64_t b_type_len, P b_root, uint64_t b_size, uint64_t b_bs) {
  if (tj_is_tree(a_type, a_type_len) && tj_is_tree(b_type, b_type_len)) return kJoinTrees;
  if (tj_compare(a_type, a_type_len, b_type, b_type_len) != 0) return kJoinDiff;
  if (a_size != b_size || a_bs != b_bs) return kJoinDiff;
  return tj_ref_equal(a_root, b_root) ? kJoinSame : kJoinDiff;
}

}  // namespace glfsx
