// ragged_groups.h -- how glfsx_open_blobs cuts a batch of messages of unequal
// length into the groups it sends through the device, as a pure function of
// the lengths: no HIP, CPU-tested (tests/c/ragged_groups_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace glfsx {

constexpr uint64_t kRaggedGroupBytes = 64ull << 20;  // staging bytes per group
constexpr uint64_t kRaggedStageAlign = 16;           // every message starts on it

// Messages [i0, i1) and the staging bytes they take (the end of the last one).
struct RaggedGroup {
  uint64_t i0, i1, bytes;
};

// Whole consecutive messages, in order, every message in exactly one group
// and no group empty; message i lies at soff[i] of its group's staging, a
// multiple of kRaggedStageAlign at or after the end of message i - 1.  A group
// takes at most `cap` staging bytes, except that a message longer than cap
// is a group of its own.  n == 0: no groups.
inline void ragged_groups(const uint64_t *lens, uint64_t n, uint64_t cap,
                          std::vector<RaggedGroup> *groups, std::vector<uint64_t> *soff) {
  groups->clear();
  soff->assign(size_t(n), 0);
  uint64_t i = 0;
  while (i < n) {
    RaggedGroup g{i, i, 0};
    while (g.i1 < n) {
      const uint64_t len = lens[g.i1];
      uint64_t at = 0;
      if (g.i1 > g.i0) {
        if (g.bytes > cap) break;  // a lone message longer than cap
        at = (g.bytes + kRaggedStageAlign - 1) & ~(kRaggedStageAlign - 1);
        // (at < bytes: the rounding wrapped; len > cap - at covers at + len wrapping)
        if (at < g.bytes || at > cap || len > cap - at) break;
      }
      (*soff)[size_t(g.i1)] = at;
      g.bytes = at + len;
      ++g.i1;
    }
    groups->push_back(g);
    i = g.i1;
  }
}

}  // namespace glfsx
