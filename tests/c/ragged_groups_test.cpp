// ragged_groups_test.cpp -- the grouping of glfsx_open_blobs and the run
// copier (glfs_amd/csrc/ragged_groups.h) as a stand-alone program: built with the
// host compiler under AddressSanitizer and UBSan by tests/test_ragged_groups.py.
#include "ragged_groups.h"

#include <algorithm>
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

// ---- the run copier (ragged_runs) ----
static uint64_t g_rng = 99;
static uint64_t rnd(uint64_t below) {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (g_rng >> 24) % below;
}

struct Run {
  uint64_t src, stage, len;
};
struct Msgs {
  std::vector<uint64_t> src, stage, len;
  void add(uint64_t s, uint64_t d, uint64_t l) {
    src.push_back(s);
    stage.push_back(d);
    len.push_back(l);
  }
};

// Copying by the emitted runs gives byte for byte what one copy per message
// gives, both ways, into heap buffers of exactly the needed size; no two
// consecutive runs are contiguous on both sides.  Returns the runs.
static std::vector<Run> check_runs(const Msgs &m) {
  const uint64_t n = m.len.size();
  std::vector<Run> runs;
  ragged_runs(m.src.data(), m.stage.data(), m.len.data(), n,
              [&](uint64_t s, uint64_t d, uint64_t l) { runs.push_back({s, d, l}); });
  uint64_t src_size = 0, stage_size = 0, bytes = 0, run_bytes = 0;
  for (uint64_t j = 0; j < n; ++j) {
    if (m.len[j] == 0 || m.len[j] == kRaggedAbsent) continue;
    src_size = std::max(src_size, m.src[j] + m.len[j]);
    stage_size = std::max(stage_size, m.stage[j] + m.len[j]);
    bytes += m.len[j];
  }
  std::vector<uint8_t> mem(src_size), by_run(stage_size, 0), by_msg(stage_size, 0);
  std::vector<uint8_t> back_run(src_size, 0), back_msg(src_size, 0);
  for (uint8_t &b : mem) b = uint8_t(rnd(256));
  for (const Run &r : runs) {
    CHECK(r.len > 0);
    run_bytes += r.len;
    CHECK(r.src + r.len <= src_size && r.stage + r.len <= stage_size);
    std::copy(mem.begin() + r.src, mem.begin() + r.src + r.len, by_run.begin() + r.stage);
  }
  CHECK(run_bytes == bytes);
  for (uint64_t j = 0; j < n; ++j)
    if (m.len[j] && m.len[j] != kRaggedAbsent)
      std::copy(mem.begin() + m.src[j], mem.begin() + m.src[j] + m.len[j],
                by_msg.begin() + m.stage[j]);
  CHECK(by_run == by_msg);
  for (const Run &r : runs)  // the scatter, over the same runs
    std::copy(by_run.begin() + r.stage, by_run.begin() + r.stage + r.len,
              back_run.begin() + r.src);
  for (uint64_t j = 0; j < n; ++j)
    if (m.len[j] && m.len[j] != kRaggedAbsent)
      std::copy(by_msg.begin() + m.stage[j], by_msg.begin() + m.stage[j] + m.len[j],
                back_msg.begin() + m.src[j]);
  CHECK(back_run == back_msg);
  for (size_t k = 1; k < runs.size(); ++k)  // maximal
    CHECK(!(runs[k].src == runs[k - 1].src + runs[k - 1].len &&
            runs[k].stage == runs[k - 1].stage + runs[k - 1].len));
  return runs;
}

// n messages of seeded lengths: `gap` leaves holes at the source, `align`
// rounds each staging offset up, `permute` lays the sources out in another
// order, `zeros` / `absent` make about one message in four empty / absent.
static Msgs make_msgs(uint64_t n, bool gap, uint64_t align, bool permute, bool zeros,
                      bool absent) {
  std::vector<uint64_t> len(n), src(n), order(n);
  for (uint64_t j = 0; j < n; ++j) {
    len[j] = zeros && rnd(4) == 0 ? 0 : 1 + rnd(align > 1 && rnd(2) ? 4 * align : 300);
    if (align > 1 && rnd(3) == 0) len[j] = (len[j] + align - 1) / align * align;
    order[j] = j;
  }
  if (permute)
    for (uint64_t j = n; j > 1; --j) std::swap(order[j - 1], order[rnd(j)]);
  uint64_t s = 0;
  for (uint64_t k = 0; k < n; ++k) {  // sources: disjoint, in `order`
    if (gap && rnd(3) == 0) s += 1 + rnd(50);
    src[order[k]] = s;
    s += len[order[k]];
  }
  Msgs m;
  uint64_t d = 0;
  for (uint64_t j = 0; j < n; ++j) {
    if (absent && rnd(4) == 0) {  // as post_small_groups marks them
      m.add(src[j], 0, kRaggedAbsent);
      continue;
    }
    d = (d + align - 1) / align * align;
    m.add(src[j], d, len[j]);
    d += len[j];
  }
  return m;
}

static void test_runs() {
  {  // n = 0: no run, null pointers never read
    int calls = 0;
    ragged_runs(nullptr, nullptr, nullptr, 0, [&](uint64_t, uint64_t, uint64_t) { ++calls; });
    CHECK(calls == 0);
  }
  {  // n = 1: the message, or nothing
    Msgs m;
    m.add(5, 16, 7);
    auto r = check_runs(m);
    CHECK(r.size() == 1 && r[0].src == 5 && r[0].stage == 16 && r[0].len == 7);
    m.len[0] = 0;
    CHECK(check_runs(m).empty());
    m.len[0] = kRaggedAbsent;
    CHECK(check_runs(m).empty());
  }
  for (uint64_t n : {2, 3, 17, 400}) {
    // fully contiguous: one run, zero lengths included
    CHECK(check_runs(make_msgs(n, false, 1, false, false, false)).size() == 1);
    CHECK(check_runs(make_msgs(n, false, 1, false, true, false)).size() <= 1);
    check_runs(make_msgs(n, true, 1, false, false, false));   // gapped at the source only
    check_runs(make_msgs(n, false, 16, false, false, false));  // at the staging only
    check_runs(make_msgs(n, false, 64, false, false, false));
    check_runs(make_msgs(n, false, 1, true, false, false));    // permuted sources
    check_runs(make_msgs(n, true, 16, true, true, true));      // everything at once
    // absent messages in the middle and at both ends
    Msgs m = make_msgs(n, false, 1, false, false, true);
    m.len.front() = m.len.back() = kRaggedAbsent;
    if (n > 2) m.len[n / 2] = kRaggedAbsent;
    const auto r = check_runs(m);
    // an absent message leaves a hole at the source, so it ends a run
    uint64_t want = 0;
    for (uint64_t j = 0; j < n; ++j)
      want += m.len[j] != kRaggedAbsent && (j == 0 || m.len[j - 1] == kRaggedAbsent);
    CHECK(r.size() == want);
  }
  {  // sizes aligned at the staging stay one run; one odd size splits it
    Msgs m;
    for (uint64_t j = 0; j < 8; ++j) m.add(64 * j, 64 * j, 64);
    CHECK(check_runs(m).size() == 1);
    m.len[3] = 63;
    CHECK(check_runs(m).size() == 2);
  }
}

int main() {
  test_runs();
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
