// launch_plan.h -- the shape of a bulk launch (post_kernels.hip) as pure
// functions of its sizes and the two tuning values: no HIP, CPU-tested.
#pragma once
#include <stdint.h>

namespace glfsx {

constexpr uint32_t kMaxSplitLog2 = 8;  // the last workgroup merges <= 256 CVs
constexpr uint64_t kDcMinWgs = 1024;   // see pass_plan

// Chunks per lane (g) and log2 workgroups per message (sl) of a launch over
// n messages of at most maxlen bytes.  split_target, latency_wgs: the
// current values of glfsx_set_split_target / glfsx_set_latency_wgs.
struct PassPlan {
  int g;
  uint32_t sl;
};
inline PassPlan pass_plan(uint64_t n, uint64_t maxlen, uint32_t split_target,
                          uint32_t latency_wgs) {
  const uint64_t C = maxlen ? (maxlen + 1023) >> 10 : 1;
  int g = 1;
  while (256ull * g < C && g < 64) g *= 2;
  // messages above 256 lanes x 64 chunks (16 MiB) always span several
  // workgroups
  uint32_t sl = 0;
  while ((256ull * g << sl) < C) ++sl;
  // few messages: halve the chunks per lane and double the workgroups per
  // message until the launch fills the chip (256 CUs x 8 workgroups)
  const uint64_t target = split_target;
  const int g0 = g;
  const uint32_t sl0 = sl;
  while (g > 1 && sl < kMaxSplitLog2 && (n << sl) < target) {
    g /= 2;
    ++sl;
  }
  // ... but a one-launch split post (k_pass_dc: more than latency_wgs * 5/8
  // workgroups, G <= 4) of fewer than ~1024 workgroups runs its DEK and CID
  // items in about one round each and loses to the two-pass latency form:
  // take the plan with the most workgroups that stays in that form.  Create
  // at 2 MiB blocks, 64 / 115 blocks (the config-4 tree blob): 355 -> 499 /
  // 546 -> 590 GiB/s; 128 x 1 MiB 362 -> 506; 200 x 2 MiB and up, or 256 x
  // 1 MiB and up, keep the one-launch plan (scripts/r4_plan_sweep.py,
  // DESIGN.md section 5)
  const uint64_t lat = uint64_t(latency_wgs) * 5 / 8;
  if (sl > 0 && g <= 4 && (n << sl) > lat && (n << sl) < kDcMinWgs) {
    int bg = 0;
    uint32_t bsl = 0;
    for (int gg = g0, s = int(sl0); gg >= 1 && s <= int(kMaxSplitLog2); gg /= 2, ++s)
      if ((n << s) <= lat) {
        bg = gg;
        bsl = uint32_t(s);
      }
    if (bg && bsl > 0) {
      g = bg;
      sl = bsl;
    }
  }
  return {g, sl};
}

// BLAKE3-only pass in quad layout (k_quad): latency-bound launches of at
// most 16384 chunks, messages of at most 64 x 256 KiB.  Messages of up to
// 64 x 64 KiB (4 MiB: index nodes at 1-4 MiB blocks) use 64 quads per
// workgroup, larger ones 256 (the last workgroup merges <= 64 CVs, one per
// quad of its own).
inline int quad_qpw(uint64_t maxlen) { return maxlen <= (64ull << 16) ? 64 : 256; }

}  // namespace glfsx
