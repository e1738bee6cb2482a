// tree_join_test.cpp -- tree_join.h's functions and glfsx_tree_join, as a
// stand-alone program for the host sanitizers (tests/test_tree_join.py builds
// it with -fsanitize=address,undefined and runs it; nothing is loaded into
// Python).
//
//   1. tj_compare against a byte loop written here, over names that are
//      prefixes of one another, that differ in a byte >= 0x80, and that are
//      equal up to byte 3, 4, 7, 8, 15, 16 and 299 of 300; each name in a heap
//      buffer of exactly its length, at every alignment the allocator gives
//      plus an offset of 0..7, so a read past a name is an AddressSanitizer
//      report.
//   2. tj_lower_bound / tj_find against a linear scan.
//   3. glfsx_tree_join against a brute-force O(na nb) join written here, every
//      column in a heap buffer of exactly its length: small and threaded
//      sizes, no match / all matching, every class, null outputs, and one
//      unsorted side (the outputs' range only).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>

#include "tree.cpp"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);             \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

namespace {

typedef std::string S;

// strings.Compare, byte by byte
int ref_compare(const S &a, const S &b) {
  const size_t m = std::min(a.size(), b.size());
  for (size_t i = 0; i < m; ++i) {
    const unsigned x = (unsigned char)a[i], y = (unsigned char)b[i];
    if (x != y) return x < y ? -1 : 1;
  }
  return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

// a heap copy of exactly n bytes (n == 0: a block of no bytes)
template <class T>
T *exact(const T *src, size_t n) {
  T *p = static_cast<T *>(malloc(n * sizeof(T)));
  if (n) memcpy(p, src, n * sizeof(T));
  return p;
}

// s ending at the last byte of its block, `shift` bytes into it
struct Placed {
  uint8_t *block;
  const uint8_t *p;
  Placed(const S &s, size_t shift) {
    block = static_cast<uint8_t *>(malloc(shift + s.size()));
    if (s.size()) memcpy(block + shift, s.data(), s.size());
    p = block + shift;
  }
  ~Placed() { free(block); }
};

std::vector<S> special_names() {
  std::vector<S> v = {"", "a", "ab", S("ab\0", 3), "b", "a\x7f", "a\x80", "a\xff", "\x80", "\x7f"};
  const S base(300, 'x');
  for (size_t at : {3u, 4u, 7u, 8u, 15u, 16u, 299u}) {
    S lo = base, hi = base;
    lo[at] = 'a';
    hi[at] = '\xe9';
    v.push_back(lo);
    v.push_back(hi);
  }
  v.push_back(base);
  v.push_back(base.substr(0, 299));
  for (size_t n = 1; n <= 17; ++n) v.push_back(S(n, 'q'));
  return v;
}

struct Cols {  // one side, every column in a block of exactly its length
  glfsx_tree_cols c{};
  std::vector<S> names, types;
  std::vector<uint8_t> roots;
  std::vector<uint64_t> sizes, bss;
  void place() {
    const uint64_t n = names.size();
    S nb, tb;
    std::vector<uint64_t> no(1, 0), to(1, 0);
    for (uint64_t i = 0; i < n; ++i) {
      nb += names[i];
      tb += types[i];
      no.push_back(nb.size());
      to.push_back(tb.size());
    }
    c.n = n;
    c.names = exact(reinterpret_cast<const uint8_t *>(nb.data()), nb.size());
    c.name_offs = exact(no.data(), no.size());
    c.types = exact(reinterpret_cast<const uint8_t *>(tb.data()), tb.size());
    c.type_offs = exact(to.data(), to.size());
    c.roots = exact(roots.data(), roots.size());
    c.sizes = exact(sizes.data(), sizes.size());
    c.block_sizes = exact(bss.data(), bss.size());
  }
  ~Cols() {
    free(const_cast<uint8_t *>(c.names));
    free(const_cast<uint64_t *>(c.name_offs));
    free(const_cast<uint8_t *>(c.types));
    free(const_cast<uint64_t *>(c.type_offs));
    free(const_cast<uint8_t *>(c.roots));
    free(const_cast<uint64_t *>(c.sizes));
    free(const_cast<uint64_t *>(c.block_sizes));
  }
  void add(const S &name, const S &type, uint8_t fill, uint64_t size, uint64_t bs) {
    names.push_back(name);
    types.push_back(type);
    roots.insert(roots.end(), 64, fill);
    sizes.push_back(size);
    bss.push_back(bs);
  }
};

uint8_t ref_class(const Cols &a, uint64_t i, const Cols &b, uint64_t j) {
  if (a.types[i] == "tree" && b.types[j] == "tree") return GLFSX_JOIN_TREES;
  const bool same = a.types[i] == b.types[j] && a.sizes[i] == b.sizes[j] && a.bss[i] == b.bss[j] &&
                    memcmp(&a.roots[64 * i], &b.roots[64 * j], 64) == 0;
  return same ? GLFSX_JOIN_SAME : GLFSX_JOIN_DIFF;
}

// the join against the O(na nb) loop; guard words around every output
void check_join(Cols &a, Cols &b, bool sorted = true) {
  a.place();
  b.place();
  const uint64_t na = a.c.n, nb = b.c.n;
  std::vector<int64_t> am(na + 2, 0x5A5A5A5A5A5A5A5All), bm(nb + 2, 0x5A5A5A5A5A5A5A5All);
  std::vector<uint8_t> ac(na + 2, 0x5A);
  CHECK(glfsx_tree_join(&a.c, &b.c, am.data() + 1, bm.data() + 1, ac.data() + 1) == 0);
  CHECK(am[0] == 0x5A5A5A5A5A5A5A5All && am[na + 1] == am[0]);
  CHECK(bm[0] == 0x5A5A5A5A5A5A5A5All && bm[nb + 1] == bm[0]);
  CHECK(ac[0] == 0x5A && ac[na + 1] == 0x5A);
  if (!sorted) {  // unspecified results, but in range
    for (uint64_t i = 0; i < na; ++i) CHECK(am[i + 1] >= -1 && am[i + 1] < int64_t(nb));
    for (uint64_t j = 0; j < nb; ++j) CHECK(bm[j + 1] >= -1 && bm[j + 1] < int64_t(na));
    for (uint64_t i = 0; i < na; ++i) CHECK(ac[i + 1] <= GLFSX_JOIN_DIFF);
    return;
  }
  std::vector<int64_t> wa(na, -1), wb(nb, -1);
  for (uint64_t i = 0; i < na; ++i)
    for (uint64_t j = 0; j < nb; ++j)
      if (a.names[i] == b.names[j]) {
        wa[i] = int64_t(j);
        wb[j] = int64_t(i);
      }
  for (uint64_t i = 0; i < na; ++i) {
    CHECK(am[i + 1] == wa[i]);
    CHECK(ac[i + 1] == (wa[i] < 0 ? GLFSX_JOIN_ONLY : ref_class(a, i, b, uint64_t(wa[i]))));
  }
  for (uint64_t j = 0; j < nb; ++j) CHECK(bm[j + 1] == wb[j]);
  // every output nullable: each alone gives the same words
  std::vector<int64_t> am2(na), bm2(nb);
  std::vector<uint8_t> ac2(na);
  CHECK(glfsx_tree_join(&a.c, &b.c, am2.data(), nullptr, nullptr) == 0);
  CHECK(glfsx_tree_join(&a.c, &b.c, nullptr, bm2.data(), nullptr) == 0);
  CHECK(glfsx_tree_join(&a.c, &b.c, nullptr, nullptr, ac2.data()) == 0);
  CHECK(glfsx_tree_join(&a.c, &b.c, nullptr, nullptr, nullptr) == 0);
  CHECK(std::equal(am2.begin(), am2.end(), am.begin() + 1));
  CHECK(std::equal(bm2.begin(), bm2.end(), bm.begin() + 1));
  CHECK(std::equal(ac2.begin(), ac2.end(), ac.begin() + 1));
}

void random_side(std::mt19937_64 &rng, const std::vector<S> &pool, uint64_t n, Cols *c) {
  std::set<S, bool (*)(const S &, const S &)> pick(
      [](const S &x, const S &y) { return ref_compare(x, y) < 0; });
  while (pick.size() < n) pick.insert(pool[rng() % pool.size()]);
  const char *types[] = {"blob", "tree", "tre", ""};
  for (const S &nm : pick)
    c->add(nm, types[rng() % 4], uint8_t(rng() % 3), rng() % 3, 1 + rng() % 2);
}

}  // namespace

int main() {
  using namespace glfsx;
  // 1. tj_compare
  const std::vector<S> sp = special_names();
  for (const S &x : sp)
    for (const S &y : sp)
      for (size_t sx = 0; sx < 8; sx += 3)
        for (size_t sy = 0; sy < 8; sy += 5) {
          Placed px(x, sx), py(y, sy);
          CHECK(tj_compare(px.p, x.size(), py.p, y.size()) == ref_compare(x, y));
        }
  CHECK(tj_compare<const uint8_t *>(nullptr, 0, nullptr, 0) == 0);

  // 2. tj_lower_bound / tj_find over the sorted special names
  {
    std::vector<S> sorted = sp;
    std::sort(sorted.begin(), sorted.end(), [](const S &x, const S &y) { return ref_compare(x, y) < 0; });
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(sorted.size())}) {
      S nb;
      std::vector<uint64_t> no(1, 0);
      for (uint64_t i = 0; i < n; ++i) {
        nb += sorted[i];
        no.push_back(nb.size());
      }
      uint8_t *names = exact(reinterpret_cast<const uint8_t *>(nb.data()), nb.size());
      uint64_t *offs = exact(no.data(), no.size());
      for (const S &key : sp) {
        Placed pk(key, 1);
        uint64_t want = 0;
        while (want < n && ref_compare(sorted[want], key) < 0) ++want;
        CHECK(tj_lower_bound<const uint8_t *>(names, offs, n, pk.p, key.size()) == want);
        const int64_t f = tj_find<const uint8_t *>(names, offs, n, pk.p, key.size());
        CHECK(f == ((want < n && sorted[want] == key) ? int64_t(want) : -1));
      }
      free(names);
      free(offs);
    }
  }

  // 3. glfsx_tree_join
  std::mt19937_64 rng(7);
  std::vector<S> pool = sp;
  for (int i = 0; i < 30000; ++i) {
    char t[16];
    snprintf(t, sizeof t, "%07d", i);
    pool.push_back(t);
  }
  for (uint64_t na : {0, 1, 5, 300})
    for (uint64_t nb : {0, 1, 7, 300}) {
      Cols a, b;
      random_side(rng, na <= 7 ? sp : pool, na, &a);  // the small sides: special names only
      random_side(rng, nb <= 7 ? sp : pool, nb, &b);
      check_join(a, b);
    }
  {  // enough entries for several host threads
    Cols a, b;
    random_side(rng, pool, 9000, &a);
    random_side(rng, pool, 8500, &b);
    check_join(a, b);
  }
  {  // no match at all; all matching, with every class
    Cols a, b, c, d;
    for (int i = 0; i < 50; ++i) {
      a.add("a" + std::to_string(100 + i), "blob", 1, 1, 1);
      b.add("b" + std::to_string(100 + i), "blob", 1, 1, 1);
    }
    check_join(a, b);
    const char *ta[] = {"tree", "blob", "blob", "tre", "blob", "blob", "blob", "blob", "tree"};
    const char *tb[] = {"tree", "tree", "blob", "tree", "blob", "blob", "blob", "blob", "blob"};
    for (int i = 0; i < 9; ++i) {
      c.add("n" + std::to_string(i), ta[i], 3, 10, 20);
      d.add("n" + std::to_string(i), tb[i], 3, 10, 20);
    }
    d.roots[64 * 4 + 31] ^= 1;  // one byte of the CID
    d.roots[64 * 5 + 63] ^= 0x80;  // one byte of the DEK
    d.sizes[6] += 1;
    d.bss[7] += 1;
    check_join(c, d);
  }
  {  // an unsorted side: in range, in bounds, and it returns
    Cols a, b;
    random_side(rng, pool, 3000, &a);
    random_side(rng, pool, 3000, &b);
    std::shuffle(a.names.begin(), a.names.end(), rng);
    check_join(a, b, false);
    Cols c, d;
    random_side(rng, pool, 3000, &c);
    random_side(rng, pool, 3000, &d);
    std::reverse(d.names.begin(), d.names.end());
    check_join(c, d, false);
  }
  {  // arguments
    Cols a;
    a.add("x", "blob", 0, 0, 0);
    a.place();
    glfsx_tree_cols none{};
    int64_t m;
    uint8_t k;
    CHECK(glfsx_tree_join(nullptr, &a.c, nullptr, nullptr, nullptr) == GLFSX_E_ARG);
    CHECK(glfsx_tree_join(&a.c, &none, &m, nullptr, &k) == 0 && m == -1 && k == GLFSX_JOIN_ONLY);
    glfsx_tree_cols bad = a.c;
    bad.name_offs = nullptr;
    CHECK(glfsx_tree_join(&bad, &a.c, &m, nullptr, nullptr) == GLFSX_E_ARG);
    bad = a.c;
    bad.roots = nullptr;
    CHECK(glfsx_tree_join(&bad, &a.c, &m, nullptr, nullptr) == 0 && m == 0);
    CHECK(glfsx_tree_join(&bad, &a.c, &m, nullptr, &k) == GLFSX_E_ARG);
  }
  printf("tree_join_test: ok\n");
  return 0;
}
