// launch_log.h -- which kernel a launch really ran (the test hooks
// glfsx_debug_pass_log for the bulk passes, glfsx_debug_aux_log for the
// small-blob, decrypt, ragged and one-shot kernels): the record a launch site
// appends and the bounded log that keeps them.  Plain C++ and a mutex: no HIP,
// CPU-tested (tests/c/stream_scratch_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <vector>

namespace glfsx {

// Kernel families of the bulk launches (the pass log) ...
enum : uint32_t { kLaunchPass = 1, kLaunchQuad = 2, kLaunchPassDc = 3, kLaunchOpen = 4 };
// ... and of the aux log: k_small, k_small_q, k_decrypt_lines, k_decrypt;
// the three levels of a ragged pass, post or open (k_rag_chunk / k_rag_merge_a
// / k_rag_merge_b and their k_rag_open_ forms); the one-shot classes (k_one,
// the k_med_dek + k_med_cid pair, k_one_open; by value or over an array).
enum : uint32_t {
  kLaunchSmall = 5,
  kLaunchSmallQ = 6,
  kLaunchDecryptLines = 7,
  kLaunchDecrypt = 8,
  kLaunchRagChunk = 9,
  kLaunchRagMergeA = 10,
  kLaunchRagMergeB = 11,
  kLaunchOne = 12,
  kLaunchMed = 13,
  kLaunchOneOpen = 14
};

// A count as a log word: saturated, never truncated.
inline uint32_t log_word(uint64_t v) { return v < UINT32_MAX ? uint32_t(v) : UINT32_MAX; }

// One launch: the template arguments of the kernel and the grid.  The
// selection (launch_plan.h) returns it; the launch site runs and logs it.
// kLaunchRecWords uint32_t, in this order (include/glfsx.h documents it).
// The aux families use the same ten words (small_rec, lines_rec,
// decrypt_rec, rag_pass_recs, one_rec of launch_plan.h; the word use is in
// include/glfsx.h).
struct LaunchRec {
  uint32_t family;      // kLaunchPass ...
  uint32_t g;           // G; k_quad: quads per workgroup
  uint32_t chacha;      // CHACHA (k_pass_dc, k_open: 1 -- both passes)
  uint32_t aligned;     // ALIGNED
  uint32_t form;        // ARX form A
  uint32_t split_log2;  // log2 workgroups per message
  uint32_t grid;        // workgroups launched
  uint32_t fine_div;    // k_pass_dc: DcState::fine_div, else 0
  uint32_t items;       // k_pass_dc: work items over all lists, else 0
  uint32_t n;           // messages
};
constexpr size_t kLaunchRecWords = sizeof(LaunchRec) / sizeof(uint32_t);
static_assert(kLaunchRecWords == 10, "LaunchRec is ten words, no padding");

// Off until enable(): a launch site asks on() -- one relaxed load -- and
// appends only then.  The log keeps the first `cap` records since the last
// reset and counts the ones after them, so a long run cannot grow it.
class LaunchLog {
 public:
  explicit LaunchLog(size_t cap = 4096) : cap_(cap) {}
  bool on() const { return on_.load(std::memory_order_relaxed); }
  void enable() {
    std::lock_guard<std::mutex> lk(mu_);
    recs_.reserve(cap_);
    on_.store(true, std::memory_order_relaxed);
  }
  void append(const LaunchRec &r) {
    std::lock_guard<std::mutex> lk(mu_);
    if (recs_.size() < cap_) recs_.push_back(r);
    ++total_;
  }
  // The first min(cap, kept) records to out (kLaunchRecWords words each; out
  // may be null with cap 0); returns the number appended since the last
  // reset, the dropped ones included.  reset: empty the log after reading.
  size_t read(bool reset, uint32_t *out, size_t cap) {
    std::lock_guard<std::mutex> lk(mu_);
    const size_t k = out ? (cap < recs_.size() ? cap : recs_.size()) : 0;
    for (size_t i = 0; i < k; ++i) {
      const LaunchRec &r = recs_[i];
      const uint32_t w[kLaunchRecWords] = {r.family, r.g,    r.chacha,   r.aligned, r.form,
                                           r.split_log2, r.grid, r.fine_div, r.items,   r.n};
      for (size_t j = 0; j < kLaunchRecWords; ++j) out[i * kLaunchRecWords + j] = w[j];
    }
    const size_t total = total_;
    if (reset) {
      recs_.clear();
      total_ = 0;
    }
    return total;
  }
  size_t kept() {
    std::lock_guard<std::mutex> lk(mu_);
    return recs_.size();
  }

 private:
  const size_t cap_;
  std::atomic<bool> on_{false};
  std::mutex mu_;
  std::vector<LaunchRec> recs_;
  size_t total_ = 0;
};

}  // namespace glfsx
