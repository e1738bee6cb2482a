// one_classes.h -- how a batch of one-shot requests is laid out in a lane's
// descriptor arrays (oneshot.cpp one_launch).  A pure function of the
// requests' kinds and lengths: no HIP, no state.
//
// A batch mixes posts and verified reads ("opens").  Each class present gets
// one launch (launch_plan.h one_rec) over a contiguous descriptor range:
//   posts, lengths <= small_max          the post array, [0, count)
//   posts, longer (two launches each)    the post array, behind the small ones
//   opens without a DEK check            the open array, [0, count)
//   opens with one (salted)              the open array, behind the others
// Request k keeps flag k of the lane whatever its class.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace glfsx {

enum OneClass : uint8_t { kOneSmall = 0, kOneMed = 1, kOneOpen = 2, kOneOpenSalted = 3 };
constexpr int kOneClasses = 4;

// The classes' length limits: one launch up to kMaxOneLen (posts and opens),
// the medium posts' two launches up to kMaxMedLen (kernels.h: OneDesc).
constexpr uint64_t kMaxOneLen = 64ull * 1024;
constexpr uint64_t kMaxMedLen = 4ull << 20;

struct OneItem {
  bool open;     // a verified read, else a post
  bool salted;   // opens only: the DEK is checked too
  uint64_t len;
};

struct OneLayout {
  uint32_t count[kOneClasses] = {0, 0, 0, 0};
  uint32_t start[kOneClasses] = {0, 0, 0, 0};    // first descriptor, in the class's array
  uint64_t max_len[kOneClasses] = {0, 0, 0, 0};
  uint64_t med_bytes = 0;                        // device copies: lengths rounded up to 256
  std::vector<uint8_t> cls;                      // per request
  std::vector<uint32_t> slot;                    // per request: its descriptor in the array
  std::vector<uint64_t> med_off;                 // per request: its device copy (kOneMed)
};

inline uint64_t one_med_span(uint64_t len) { return (len + 255) & ~uint64_t(255); }

inline OneClass one_class(const OneItem &it, uint64_t small_max) {
  if (it.open) return it.salted ? kOneOpenSalted : kOneOpen;
  return it.len <= small_max ? kOneSmall : kOneMed;
}

// Requests keep their order inside a class.
inline OneLayout one_layout(const OneItem *items, size_t n, uint64_t small_max) {
  OneLayout L;
  L.cls.resize(n);
  L.slot.resize(n);
  L.med_off.assign(n, 0);
  for (size_t k = 0; k < n; ++k) {
    const OneClass c = one_class(items[k], small_max);
    L.cls[k] = c;
    ++L.count[c];
    if (items[k].len > L.max_len[c]) L.max_len[c] = items[k].len;
  }
  L.start[kOneSmall] = 0;
  L.start[kOneMed] = L.count[kOneSmall];
  L.start[kOneOpen] = 0;
  L.start[kOneOpenSalted] = L.count[kOneOpen];
  uint32_t next[kOneClasses];
  for (int c = 0; c < kOneClasses; ++c) next[c] = L.start[c];
  for (size_t k = 0; k < n; ++k) {
    const uint8_t c = L.cls[k];
    L.slot[k] = next[c]++;
    if (c == kOneMed) {
      L.med_off[k] = L.med_bytes;
      L.med_bytes += one_med_span(items[k].len);
    }
  }
  return L;
}

}  // namespace glfsx
