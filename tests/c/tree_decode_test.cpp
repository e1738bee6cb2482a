// tree_decode_test.cpp -- glfsx_tree_decode against glfsx_tree_encode, as a
// stand-alone program for the host sanitizers (tests/test_tree_decode.py
// builds it with -fsanitize=address,undefined and runs it; nothing is loaded
// into Python).
//
//   1. decode(encode(columns)) == columns with every status 0, over every
//      escaping class of test_native_encoder_matches_python's pool.  One
//      class cannot come back as it went in: the encoder writes each byte of
//      invalid UTF-8 as the escape of U+FFFD, so such a name decodes to
//      EF BF BD per bad byte -- what Go's decoder gives too.  The expected
//      columns are the inputs with that substitution (go_valid, written here
//      independently of tree.cpp).
//   2. encode(decode(lines)) == lines for the lines whose strings were valid
//      UTF-8; for the others (whose U+FFFD re-encodes raw, not as the
//      escape) it equals the encoding of the expected columns, which decodes
//      to the same columns again.
//   3. The negative corpus of argv[1] (records of u32 length, u8 strict,
//      bytes), each decoded from a heap buffer of exactly its length so
//      that a read past the end is an AddressSanitizer report.  A strict
//      case must be flagged: a line of it NONCANON, or a tail.  A case that is
//      not strict (a substitution that may spell another canonical line)
//      must be flagged or prove itself canonical: encode(decode(x)) == x.
#include <cstdio>
#include <cstdlib>
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

// s with every byte that utf8.DecodeRune rejects replaced by EF BF BD
S go_valid(const S &s) {
  S o;
  for (size_t i = 0; i < s.size();) {
    const unsigned char b = s[i];
    auto c = [&](size_t k) { return i + k < s.size() ? (unsigned char)s[i + k] : 0; };
    auto t = [&](size_t k) { return (c(k) & 0xC0) == 0x80; };
    size_t n = 0;
    if (b < 0x80) n = 1;
    else if (b >= 0xC2 && b <= 0xDF && t(1)) n = 2;
    else if (b >= 0xE0 && b <= 0xEF && t(1) && t(2) && !(b == 0xE0 && c(1) < 0xA0) &&
             !(b == 0xED && c(1) > 0x9F)) n = 3;
    else if (b >= 0xF0 && b <= 0xF4 && t(1) && t(2) && t(3) && !(b == 0xF0 && c(1) < 0x90) &&
             !(b == 0xF4 && c(1) > 0x8F)) n = 4;
    if (n) o.append(s, i, n); else o += "\xEF\xBF\xBD";
    i += n ? n : 1;
  }
  return o;
}

struct Cols {
  std::vector<S> names, types;
  std::vector<uint32_t> modes;
  std::vector<uint8_t> roots;
  std::vector<uint64_t> sizes, bss;
};

S encode(const Cols &c) {
  const uint64_t n = c.names.size();
  S nb, tb;
  std::vector<uint64_t> no(1, 0), to(1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    nb += c.names[i];
    tb += c.types[i];
    no.push_back(nb.size());
    to.push_back(tb.size());
  }
  uint64_t len = 0;
  auto u8 = [](const S &s) { return reinterpret_cast<const uint8_t *>(s.data()); };
  CHECK(glfsx_tree_encode(n, u8(nb), no.data(), c.modes.data(), u8(tb), to.data(), c.roots.data(),
                          c.sizes.data(), c.bss.data(), nullptr, 0, &len, nullptr) == 0);
  S out(len, '\0');
  CHECK(glfsx_tree_encode(n, u8(nb), no.data(), c.modes.data(), u8(tb), to.data(), c.roots.data(),
                          c.sizes.data(), c.bss.data(), reinterpret_cast<uint8_t *>(&out[0]), len,
                          &len, nullptr) == 0);
  return out;
}

struct Dec {
  Cols c;
  std::vector<uint32_t> status;
  uint64_t counts[5];
};

// from a heap copy of exactly x's length; guard bytes around every output
Dec decode(const S &x) {
  Dec d;
  uint8_t *in = static_cast<uint8_t *>(malloc(x.size() ? x.size() : 1));
  memcpy(in, x.data(), x.size());
  const uint8_t *arg = x.size() ? in : nullptr;
  CHECK(glfsx_tree_decode(arg, x.size(), nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr,
                          nullptr, nullptr, nullptr, nullptr, 0, d.counts) == 0);
  const uint64_t n = d.counts[0], nl = d.counts[1], tl = d.counts[2];
  std::vector<uint8_t> names(nl + 2, 0xA5), types(tl + 2, 0xA5);
  std::vector<uint64_t> no(n + 3, 0xA5), to(n + 3, 0xA5);
  d.c.modes.assign(n, 0);
  d.c.roots.assign(64 * n, 0);
  d.c.sizes.assign(n, 0);
  d.c.bss.assign(n, 0);
  d.status.assign(n, 0);
  uint64_t c2[5];
  if (n) {  // a capacity one short: an error, the counts, nothing written
    CHECK(glfsx_tree_decode(arg, x.size(), names.data() + 1, nl, no.data() + 1, nullptr,
                            types.data() + 1, tl, to.data() + 1, nullptr, nullptr, nullptr,
                            nullptr, n - 1, c2) == GLFSX_E_ARG);
    CHECK(c2[0] == n && c2[1] == nl && c2[2] == tl && no[1] == 0xA5 && to[1] == 0xA5);
    if (nl) {
      CHECK(glfsx_tree_decode(arg, x.size(), names.data() + 1, nl - 1, no.data() + 1, nullptr,
                              nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, n,
                              c2) == GLFSX_E_ARG);
      CHECK(no[1] == 0xA5 && names[1] == 0xA5);
    }
  }
  CHECK(glfsx_tree_decode(arg, x.size(), names.data() + 1, nl, no.data() + 1, d.c.modes.data(),
                          types.data() + 1, tl, to.data() + 1, d.c.roots.data(),
                          d.c.sizes.data(), d.c.bss.data(), d.status.data(), n, c2) == 0);
  for (int k = 0; k < 5; ++k) CHECK(c2[k] == d.counts[k]);
  CHECK(names[0] == 0xA5 && names[nl + 1] == 0xA5 && types[0] == 0xA5 && types[tl + 1] == 0xA5);
  CHECK(no[0] == 0xA5 && no[n + 2] == 0xA5 && to[0] == 0xA5 && to[n + 2] == 0xA5);
  CHECK(no[1] == 0 && to[1] == 0 && no[n + 1] == nl && to[n + 1] == tl);
  for (uint64_t i = 0; i < n; ++i) {
    CHECK(no[i + 1] <= no[i + 2] && to[i + 1] <= to[i + 2]);
    d.c.names.emplace_back(reinterpret_cast<char *>(names.data()) + 1 + no[i + 1],
                           no[i + 2] - no[i + 1]);
    d.c.types.emplace_back(reinterpret_cast<char *>(types.data()) + 1 + to[i + 1],
                           to[i + 2] - to[i + 1]);
  }
  free(in);
  return d;
}

bool same(const Cols &a, const Cols &b) {
  return a.names == b.names && a.types == b.types && a.modes == b.modes && a.roots == b.roots &&
         a.sizes == b.sizes && a.bss == b.bss;
}

uint64_t rng_state = 7;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

void round_trips() {
  // the pool of test_native_encoder_matches_python as Go strings' bytes,
  // plus U+2028 / U+2029 / U+FFFD written raw in the name
  const S pool[] = {"plain", "<a&b>", S("\n\r\t\b\f\x00\x1f\x7f", 8), " x ",
                    "\xC3\xA9\xE6\x97\xA5\xE6\x9C\xAC\xF0\x9F\x98\x80", "bad\x80\xff", "q\"b\\s",
                    "", "0000005", "\xED\xA0\x80", "\xE2\x80\xA8\xE2\x80\xA9\xEF\xBF\xBD"};
  const S tys[] = {"blob", "tree", "t<&>", " "};
  const uint64_t np = sizeof pool / sizeof *pool;
  struct E { S key, name, type; };
  std::vector<E> es;
  for (int i = 0; i < 20000; ++i) {  // enough for parallel_ranges to thread
    E e;
    e.name = pool[rnd() % np] + std::to_string(i) + pool[rnd() % np];
    e.key = go_valid(e.name);
    e.type = tys[rnd() % 4];
    es.push_back(e);
  }
  // a tree's names ascend: by the bytes they decode to
  std::sort(es.begin(), es.end(), [](const E &a, const E &b) { return a.key < b.key; });
  es.erase(std::unique(es.begin(), es.end(), [](const E &a, const E &b) { return a.key == b.key; }),
           es.end());
  CHECK(es.size() > 19000);
  Cols in, want;
  const uint64_t big[] = {0, 9, 10, 4294967295ull, 4294967296ull, ~0ull, ~0ull - 1,
                          9999999999999999999ull, 10000000000000000000ull};
  for (size_t i = 0; i < es.size(); ++i) {
    in.names.push_back(es[i].name);
    want.names.push_back(es[i].key);
    in.types.push_back(es[i].type);
    in.modes.push_back(i % 5 == 0 ? 0xFFFFFFFFu : i % 5 == 1 ? 0u : uint32_t(rnd()));
    for (int k = 0; k < 64; ++k) in.roots.push_back(uint8_t(rnd()));
    in.sizes.push_back(i % 3 ? rnd() >> (rnd() % 64) : big[i % 9]);
    in.bss.push_back(i % 2 ? 128 : 2 << 20);
  }
  want.types = in.types; want.modes = in.modes; want.roots = in.roots;
  want.sizes = in.sizes; want.bss = in.bss;
  const S lines = encode(in);
  const Dec d = decode(lines);
  CHECK(d.counts[0] == es.size() && d.counts[3] == 0 && d.counts[4] == 0);
  for (uint32_t s : d.status) CHECK(s == 0);
  CHECK(same(d.c, want));
  const S again = encode(d.c);
  CHECK(again == encode(want));
  size_t a = 0, b = 0, exact = 0;
  for (size_t i = 0; i < es.size(); ++i) {  // line by line
    const size_t ea = lines.find('\n', a) + 1, eb = again.find('\n', b) + 1;
    if (es[i].name == es[i].key) {
      CHECK(lines.compare(a, ea - a, again, b, eb - b) == 0);
      ++exact;
    }
    a = ea;
    b = eb;
  }
  CHECK(exact > es.size() / 2 && exact < es.size());
  CHECK(same(decode(again).c, want));
  // the empty input, and one line
  const Dec e0 = decode(S());
  CHECK(e0.counts[0] == 0 && e0.counts[3] == 0 && e0.counts[4] == 0);
  Cols one;
  one.names = {"a"}; one.types = {"blob"}; one.modes = {420}; one.roots.assign(64, 0x11);
  one.sizes = {9}; one.bss = {2 << 20};
  const Dec e1 = decode(encode(one));
  CHECK(e1.counts[0] == 1 && e1.counts[3] == 0 && same(e1.c, one));
}

void negatives(const char *path) {
  FILE *f = fopen(path, "rb");
  CHECK(f);
  uint64_t cases = 0, strict_cases = 0, proven = 0;
  for (;;) {
    uint32_t len;
    uint8_t strict;
    if (fread(&len, 4, 1, f) != 1) break;
    CHECK(fread(&strict, 1, 1, f) == 1);
    S x(len, '\0');
    CHECK(len == 0 || fread(&x[0], 1, len, f) == len);
    const Dec d = decode(x);
    bool flagged = d.counts[4] != 0;  // a tail
    for (uint32_t s : d.status) flagged |= (s & GLFSX_TREE_NONCANON) != 0;
    CHECK(d.counts[3] >= (flagged ? 1u : 0u));
    if (!flagged) {
      if (strict) printf("not flagged: case %llu: %s\n", (unsigned long long)cases, x.c_str());
      CHECK(!strict);
      CHECK(encode(d.c) == x);  // it is a line the encoder writes
      ++proven;
    }
    ++cases;
    strict_cases += strict;
  }
  fclose(f);
  CHECK(cases > 1000 && strict_cases > 500);
  printf("negative corpus: %llu cases, %llu strict, %llu canonical by re-encoding\n",
         (unsigned long long)cases, (unsigned long long)strict_cases, (unsigned long long)proven);
}

}  // namespace

int main(int argc, char **argv) {
  CHECK(argc == 2);
  round_trips();
  negatives(argv[1]);
  printf("tree_decode_test: ok\n");
  return 0;
}
