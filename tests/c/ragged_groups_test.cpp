// ragged_groups_test.cpp -- the grouping of glfsx_open_blobs
// (glfs_amd/csrc/ragged_groups.h) as a stand-alone program: built with the
// host compiler under AddressSanitizer and UBSan by tests/test_ragged_groups.py.
#include "ragged_groups.h"

#include <cstdio>
#include <cstdlib>

using namespace glfsx;

static int g_checks = 0;
#define CHECK(x)                                                      \
  do {                                                                \
    ++g_checks;                                                       \
    if (!(x)) {                                                       \
      std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

constexpr uint64_t MIB = 1ull << 20, CAP = 64 * MIB;

// The properties every grouping has: every message in exactly one group, in
// order; no group empty; no group above cap (a lone message longer than cap
// aside); staging offsets 16-B aligned, in order and disjoint, the group's
// bytes the end of its last message.
static void check_properties(const std::vector<uint64_t> &lens, uint64_t cap,
                             const std::vector<RaggedGroup> &groups,
                             const std::vector<uint64_t> &soff) {
  CHECK(soff.size() == lens.size());
  uint64_t next = 0;
  for (const RaggedGroup &g : groups) {
    CHECK(g.i0 == next);
    CHECK(g.i1 > g.i0);
    CHECK(g.i1 <= lens.size());
    uint64_t end = 0;
    for (uint64_t i = g.i0; i < g.i1; ++i) {
      CHECK(soff[i] % 16 == 0);
      CHECK(soff[i] >= end);       // disjoint, in order
      CHECK(soff[i] < end + 16);   // packed: no more than the alignment's gap
      end = soff[i] + lens[i];
    }
    CHECK(g.bytes == end);
    CHECK(g.bytes <= cap || (g.i1 - g.i0 == 1 && lens[g.i0] > cap));
    next = g.i1;
  }
  CHECK(next == lens.size());
  // greedy: the first message of a group did not fit the one before it
  for (size_t k = 1; k < groups.size(); ++k) {
    const uint64_t b = groups[k - 1].bytes, at = (b + 15) & ~15ull;
    CHECK(b > cap || at < b || at > cap || lens[groups[k].i0] > cap - at);
  }
}

static std::vector<RaggedGroup> run(const std::vector<uint64_t> &lens, uint64_t cap = CAP) {
  std::vector<RaggedGroup> groups;
  std::vector<uint64_t> soff(3, 99);  // stale contents are replaced
  ragged_groups(lens.data(), lens.size(), cap, &groups, &soff);
  check_properties(lens, cap, groups, soff);
  return groups;
}

int main() {
  {  // empty input (a null pointer is never read)
    std::vector<RaggedGroup> groups(2);
    std::vector<uint64_t> soff(5, 1);
    ragged_groups(nullptr, 0, CAP, &groups, &soff);
    CHECK(groups.empty() && soff.empty());
  }
  {  // all-zero lengths: one group of no bytes
    const auto g = run(std::vector<uint64_t>(1000, 0));
    CHECK(g.size() == 1 && g[0].i0 == 0 && g[0].i1 == 1000 && g[0].bytes == 0);
  }
  {  // one 16 MiB message
    const auto g = run({16 * MIB});
    CHECK(g.size() == 1 && g[0].bytes == 16 * MIB);
  }
  {  // sums landing exactly on 64 MiB: one group; one byte over: two
    auto g = run({16 * MIB, 16 * MIB, 16 * MIB, 16 * MIB});
    CHECK(g.size() == 1 && g[0].bytes == CAP);
    g = run({16 * MIB, 16 * MIB, 16 * MIB, 16 * MIB - 1, 1});
    CHECK(g.size() == 2 && g[0].i1 == 4);  // the last one would start at 64 MiB
    g = run({16 * MIB, 16 * MIB, 16 * MIB, 16 * MIB, 1});
    CHECK(g.size() == 2 && g[0].i1 == 4 && g[1].bytes == 1);
    g = run({16 * MIB, 16 * MIB, 16 * MIB, 16 * MIB + 1});
    CHECK(g.size() == 2 && g[0].i1 == 3 && g[1].bytes == 16 * MIB + 1);
    // the alignment's gap counts: 1 + 15 (gap) + 64 MiB - 16 fits, one more does not
    g = run({1, CAP - 16});
    CHECK(g.size() == 1 && g[0].bytes == CAP);
    g = run({1, CAP - 15});
    CHECK(g.size() == 2);
    // zero-length messages ride along at the very end of a full group
    g = run({CAP, 0, 0, 5});
    CHECK(g.size() == 2 && g[0].i1 == 3);
  }
  {  // 1 M messages of 4 KiB: 64 groups of 16384
    const auto g = run(std::vector<uint64_t>(1u << 20, 4096));
    CHECK(g.size() == 64);
    for (const RaggedGroup &x : g) CHECK(x.i1 - x.i0 == 16384 && x.bytes == CAP);
  }
  {  // a message longer than the cap is a group of its own
    const auto g = run({5, 200, 7}, 100);
    CHECK(g.size() == 3 && g[1].i0 == 1 && g[1].i1 == 2 && g[1].bytes == 200);
  }
  {  // mixed odd lengths under a small cap, and the 64-bit edge
    std::vector<uint64_t> lens;
    uint64_t x = 12345;
    for (int i = 0; i < 5000; ++i) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      lens.push_back((x >> 33) % 5000);
    }
    run(lens, 65536);
    run(lens, 4999);
    const auto g = run({~0ull, 3, ~0ull - 20}, ~0ull);
    CHECK(g.size() == 2 && g[1].i0 == 1 && g[1].bytes == ~0ull - 4);  // 16 + (2^64 - 21)
  }
  std::printf("ragged_groups_test: ok (%d checks)\n", g_checks);
  return 0;
}
