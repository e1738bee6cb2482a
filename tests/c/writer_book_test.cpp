// writer_book_test.cpp -- the Writer's bookkeeping (glfs_amd/csrc/writer_book.h)
// as a stand-alone program: the index stack's Posts against the oracle's
// streaming writer (oracle/oracle.c, compiled beside this file), its failure
// side, and the fill cursor.  Built with the host compiler under
// AddressSanitizer and UBSan by tests/test_writer_book.py.
#include "writer_book.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "oracle/oracle.h"

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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return g_rng >> 20;
}

struct Post {
  int kind;
  uint8_t ref[64];
  uint64_t len;
  bool operator==(const Post &o) const {
    return kind == o.kind && len == o.len && memcmp(ref, o.ref, 64) == 0;
  }
};
static int sink(void *ctx, int kind, const uint8_t ref[64], const uint8_t *, uint64_t len) {
  Post p{kind, {}, len};
  memcpy(p.ref, ref, 64);
  static_cast<std::vector<Post> *>(ctx)->push_back(p);
  return 0;
}

// The stack's callback over the oracle's post: builds the zero-padded node.
// fail_at > 0: call number fail_at (1-based) fails with kErr instead.
constexpr int kErr = -77;
struct NodePoster {
  const uint8_t *index_salt;
  std::vector<Post> *log;
  uint64_t calls = 0, fail_at = 0;
  int operator()(const uint8_t *refs, uint64_t present, uint64_t len, uint8_t out[64]) {
    if (++calls == fail_at) return kErr;
    CHECK(present <= len && present % 64 == 0 && (refs || present == 0));
    std::vector<uint8_t> node(len, 0), ct(len + 1);
    if (present) memcpy(node.data(), refs, present);
    oracle_post(out, ct.data(), index_salt, node.data(), len, nullptr);
    return sink(log, 1, out, nullptr, len);
  }
};

// The writer's order of Posts for `data` through the index stack: every
// block's post(rawSalt, ...) then addRef, then finishIndexes.  Returns the
// first error (the poster's), 0 otherwise.
static int run_stack(const std::vector<uint8_t> &data, uint64_t bs, const uint8_t salt[32],
                     NodePoster &poster, uint8_t root[64]) {
  uint8_t raw_salt[32];
  oracle_derive_key(raw_salt, salt, reinterpret_cast<const uint8_t *>("raw"), 3);
  IndexStack st;
  st.bf = bs / 64;
  st.node_len = bs;
  std::vector<uint8_t> ct(bs);
  for (uint64_t off = 0; off < data.size(); off += bs) {
    const uint64_t len = std::min<uint64_t>(bs, data.size() - off);
    uint8_t ref[64];
    oracle_post(ref, ct.data(), raw_salt, data.data() + off, len, nullptr);
    sink(poster.log, 0, ref, nullptr, len);
    if (int e = st.add(ref, poster)) return e;
  }
  return st.finish(root, poster);
}

static void test_index_stack_vs_oracle() {
  uint8_t salt[32], index_salt[32];
  for (int i = 0; i < 32; ++i) salt[i] = uint8_t(7 * i + 3);
  oracle_derive_key(index_salt, salt, reinterpret_cast<const uint8_t *>("index"), 5);
  int cases = 0;
  for (uint64_t bs : {128, 130, 192, 256}) {  // bf 2, 2, 3, 4
    for (uint64_t n = 0; n <= 70; ++n) {
      for (uint64_t tail : {uint64_t(0), uint64_t(1), bs - 1}) {
        std::vector<uint8_t> data(n * bs + tail);
        for (uint8_t &b : data) b = uint8_t(rnd());
        std::vector<Post> want, got;
        uint8_t want_root[64], root[64];
        int err = 0;
        oracle_writer *w = oracle_writer_new(bs, bs, salt, nullptr, sink, &want, &err);
        CHECK(w && err == 0);
        if (!data.empty()) CHECK(oracle_writer_write(w, data.data(), data.size()) == 0);
        uint64_t size = 0, obs = 0;
        CHECK(oracle_writer_finish(w, want_root, &size, &obs) == 0);
        oracle_writer_free(w);
        CHECK(size == data.size() && obs == bs);
        NodePoster poster{index_salt, &got};
        CHECK(run_stack(data, bs, salt, poster, root) == 0);
        CHECK(got.size() == want.size());
        for (size_t k = 0; k < want.size(); ++k) CHECK(got[k] == want[k]);
        CHECK(memcmp(root, want_root, 64) == 0);
        ++cases;
      }
    }
  }
  CHECK(cases == 852);
}

// A post that fails at its k-th call: add / finish return that error at once
// and post is not called again.
static void test_index_stack_failures() {
  uint8_t salt[32] = {1, 2, 3}, index_salt[32];
  oracle_derive_key(index_salt, salt, reinterpret_cast<const uint8_t *>("index"), 5);
  std::vector<uint8_t> data(9 * 128 + 1, 0x5A);
  std::vector<Post> log;
  uint8_t root[64];
  NodePoster good{index_salt, &log};
  CHECK(run_stack(data, 128, salt, good, root) == 0);
  const uint64_t posts = good.calls;
  CHECK(posts == 5 + 3 + 2 + 1);  // 10 refs at bf 2: levels of 5, 3, 2, 1 nodes
  const std::vector<Post> full = log;
  for (uint64_t k = 1; k <= posts; ++k) {
    log.clear();
    NodePoster bad{index_salt, &log, 0, k};
    CHECK(run_stack(data, 128, salt, bad, root) == kErr);
    CHECK(bad.calls == k);
    // what was posted before the failure is the full run's prefix
    CHECK(log.size() < full.size());
    for (size_t i = 0; i < log.size(); ++i) CHECK(log[i] == full[i]);
    uint64_t nodes = 0;
    for (const Post &p : log) nodes += p.kind == 1;
    CHECK(nodes == k - 1);
  }
  // the empty blob: one post of no bytes
  log.clear();
  NodePoster empty{index_salt, &log};
  CHECK(run_stack({}, 128, salt, empty, root) == 0);
  CHECK(empty.calls == 1 && log.size() == 1 && log[0].kind == 1 && log[0].len == 0);
  CHECK(memcmp(root, log[0].ref, 64) == 0);
}

static void test_fill_cursor() {
  for (uint64_t bs : {uint64_t(128), uint64_t(1000), uint64_t(1) << 20}) {
    for (uint64_t batch_blocks : {uint64_t(1), uint64_t(3), uint64_t(8192)}) {
      FillCursor f;
      f.bs = bs;
      f.batch_blocks = batch_blocks;
      CHECK(f.used() == 0 && f.cap() == bs * batch_blocks && f.room() == f.cap());
      uint64_t fed = 0, submitted = 0, batches = 0;
      for (int step = 0; step < 20000; ++step) {
        const uint64_t room = f.room();
        CHECK(room >= 1);  // a full batch was carried over at once
        const uint64_t picks[] = {0, 1, bs - 1, bs, bs + 1, room, rnd() % room};
        const uint64_t n = std::min(room, picks[rnd() % 7]);
        const uint64_t before = f.used();
        const bool full = f.add(n);
        fed += n;
        CHECK(f.used() == before + n);
        CHECK(f.used() == f.full * bs + f.partial);
        CHECK(f.partial < bs);
        CHECK(f.used() <= f.cap() && f.room() == f.cap() - f.used());
        CHECK(full == (f.full == batch_blocks));
        if (full) {  // as submit: the blocks go, the partial block is carried over
          CHECK(f.partial == 0);  // (cap is a whole number of blocks)
          submitted += f.full * bs;
          ++batches;
          f.carry();
          CHECK(f.full == 0 && f.used() == f.partial);
        }
        CHECK(submitted + f.used() == fed);
      }
      CHECK(batches > 0);
    }
  }
}

int main() {
  test_index_stack_vs_oracle();
  test_index_stack_failures();
  test_fill_cursor();
  std::printf("writer_book_test: ok (%d checks)\n", g_checks);
  return 0;
}
