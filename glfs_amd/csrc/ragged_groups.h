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

// The copies between a batch of messages and its staging: message j lies at
// src_off[j] of the caller's memory and at stage_off[j] of the staging,
// lens[j] bytes.  run(src, stage, len) is called once per maximal run of
// messages contiguous on both sides, in order; messages of length 0 or
// kRaggedAbsent (not staged at all) are skipped.
constexpr uint64_t kRaggedAbsent = ~0ull;
template <class Run>
void ragged_runs(const uint64_t *src_off, const uint64_t *stage_off, const uint64_t *lens,
                 uint64_t n, Run &&run) {
  uint64_t run_src = 0, run_dst = 0, run_len = 0;
  for (uint64_t j = 0; j < n; ++j) {
    const uint64_t len = lens[j];
    if (len == 0 || len == kRaggedAbsent) continue;
    if (run_len && src_off[j] == run_src + run_len && stage_off[j] == run_dst + run_len) {
      run_len += len;
    } else {
      if (run_len) run(run_src, run_dst, run_len);
      run_src = src_off[j];
      run_dst = stage_off[j];
      run_len = len;
    }
  }
  if (run_len) run(run_src, run_dst, run_len);
}

}  // namespace glfsx
