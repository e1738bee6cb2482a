// The layout of a batch of one-shot requests (glfs_amd/csrc/one_classes.h),
// stand-alone.  Built by tests/test_one_classes.py with the host compiler
// under -fsanitize=address,undefined; the header has no HIP in it.
#include <cstdio>
#include <cstdlib>

#include "one_classes.h"

using namespace glfsx;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

constexpr uint64_t kSmall = 64 * 1024;

// Every request has one slot of its class's range, the ranges of the two
// arrays tile them, order inside a class is the batch's, and the maxima and
// the medium copies' offsets are what the lengths say.
static void check_layout(const std::vector<OneItem> &items) {
  const OneLayout L = one_layout(items.data(), items.size(), kSmall);
  const size_t n = items.size();
  CHECK(L.cls.size() == n && L.slot.size() == n && L.med_off.size() == n);
  uint32_t count[kOneClasses] = {0, 0, 0, 0};
  uint64_t max_len[kOneClasses] = {0, 0, 0, 0};
  uint64_t med = 0;
  for (size_t k = 0; k < n; ++k) {
    const OneClass c = one_class(items[k], kSmall);
    CHECK(L.cls[k] == c);
    CHECK(L.slot[k] == L.start[c] + count[c]);   // in order, dense
    ++count[c];
    if (items[k].len > max_len[c]) max_len[c] = items[k].len;
    if (c == kOneMed) {
      CHECK(L.med_off[k] == med);
      CHECK(med % 256 == 0);
      med += one_med_span(items[k].len);
    } else {
      CHECK(L.med_off[k] == 0);
    }
  }
  for (int c = 0; c < kOneClasses; ++c) {
    CHECK(L.count[c] == count[c]);
    CHECK(L.max_len[c] == max_len[c]);
  }
  CHECK(L.med_bytes == med);
  // posts: small then medium; opens: unsalted then salted, an array of their own
  CHECK(L.start[kOneSmall] == 0 && L.start[kOneMed] == count[kOneSmall]);
  CHECK(L.start[kOneOpen] == 0 && L.start[kOneOpenSalted] == count[kOneOpen]);
  CHECK(count[0] + count[1] + count[2] + count[3] == n);
}

int main() {
  // the classes of single requests, at the boundaries
  CHECK(one_class({false, false, 0}, kSmall) == kOneSmall);
  CHECK(one_class({false, false, kSmall}, kSmall) == kOneSmall);
  CHECK(one_class({false, false, kSmall + 1}, kSmall) == kOneMed);
  CHECK(one_class({false, true, 5}, kSmall) == kOneSmall);   // salted means nothing to a post
  CHECK(one_class({true, false, 0}, kSmall) == kOneOpen);
  CHECK(one_class({true, true, kSmall}, kSmall) == kOneOpenSalted);
  CHECK(one_med_span(0) == 0 && one_med_span(1) == 256 && one_med_span(256) == 256 &&
        one_med_span(257) == 512);

  check_layout({});
  check_layout({{false, false, 10}});
  check_layout({{true, true, 10}});
  check_layout({{true, false, 0}});
  check_layout({{false, false, kSmall + 1}});
  // every class, interleaved
  check_layout({{true, true, 4096},
                {false, false, 100},
                {false, false, 1 << 20},
                {true, false, 65536},
                {false, false, 65536},
                {true, true, 0},
                {false, false, 65537},
                {true, false, 17},
                {false, false, 0}});
  {
    const std::vector<OneItem> v = {{true, true, 4096}, {false, false, 100},
                                    {false, false, 1 << 20}, {true, false, 65536},
                                    {false, false, 70000}};
    const OneLayout L = one_layout(v.data(), v.size(), kSmall);
    CHECK(L.slot[0] == 1 && L.slot[3] == 0);          // the salted open behind the other
    CHECK(L.slot[1] == 0 && L.slot[2] == 1 && L.slot[4] == 2);
    CHECK(L.med_off[2] == 0 && L.med_off[4] == (1 << 20));
    CHECK(L.med_bytes == (1 << 20) + 70144);
  }
  // a full batch of a pseudo-random mix
  std::vector<OneItem> big;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 1024; ++i) {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    big.push_back({(x & 1) != 0, (x & 2) != 0,
                   (x & 4) && !(x & 1) ? (x >> 8) % (4u << 20) : (x >> 8) % (kSmall + 1)});
  }
  check_layout(big);

  if (g_failed) {
    printf("one_classes_test: %d checks failed\n", g_failed);
    return 1;
  }
  printf("one_classes_test: ok\n");
  return 0;
}
