// post_kernels.hip -- gfx950 kernels for the bigblob write path.
//
// Per bigblob block ("message"), bigblob/ref.go:98-161 computes
//   DEK  = BLAKE3-keyed(salt, ptext)[0:32]                 (ref.go:146-161)
//   ctext = ChaCha20(DEK, nonce 0^12, counter 0) ^ ptext    (ref.go:137-144)
//   CID  = BLAKE3-256(ctext)   (store.Post, ref.go:103; blobcache [ext])
// Both hashes are BLAKE3 trees over 1 KiB chunks of 64 B blocks.
//
// Mapping (DESIGN.md "Kernels"):
//   * one 256-lane workgroup per message; lane t owns the G consecutive
//     BLAKE3 chunks [t*G, t*G+G) (G = power of two, template parameter) and
//     reduces them in registers to one subtree chaining value;
//   * the 16-word message schedule is applied at compile time (fully unrolled
//     rounds, the permutation is register renaming -- no LDS, no shuffles);
//   * the 256 subtree CVs are merged pairwise through LDS; the pairwise merge
//     with an odd element passing through is exactly BLAKE3's left-complete
//     tree, and the final parent gets ROOT;
//   * the ChaCha20 pass uses the message's DEK as wave-uniform SGPR operands
//     and fuses keystream XOR, the ctext store and the CID compression, so
//     ptext is read once per pass and ctext is never re-read.
// Integer ALU work only (v_add3_u32 / v_xor_b32 / v_alignbit_b32); no MFMA.
//
// The host half below the fragments launches them.  The shape of a bulk
// launch comes from launch_plan.h (pure functions); what a stream's launches
// keep between them is one ScratchSlot per (device, stream) whose members
// own their memory (stream_scratch.h).
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "device_common.h"
#include "launch_log.h"
#include "launch_plan.h"
#include "stream_scratch.h"

// One namespace block holds the fragments and the host side: closing and
// reopening it between them changes the order in which the compiler emits
// the device variables (g_clk, g_one_t).
namespace glfsx {
namespace {

// The kernels, by family (fragments of this translation unit, in this order):
#include "b3_arx.h"
#include "pass_kernels.h"
#include "quad_kernels.h"
#include "one_kernels.h"
#include "one_open_kernels.h"
#include "small_kernels.h"
#include "ragged_kernels.h"
#include "read_kernels.h"
#include "open_kernels.h"
#include "ragged_open_kernels.h"

// The host side: launch plans and launches.

// Latency mode: launches of at most this many 256-lane workgroups (default
// 512 = 2 waves per SIMD) run the compiler-scheduled ARX form, and the CID
// pass splits into a per-block keystream launch + a BLAKE3 pass.
// glfsx_set_latency_wgs overrides it (tuning, tests of both forms).
std::atomic<uint32_t> g_latency_wgs{512};
uint32_t latency_wgs() { return g_latency_wgs.load(std::memory_order_relaxed); }

// The launch log (glfsx_debug_pass_log): off until first asked for; then
// every bulk launch site below appends what it launched.  Never destroyed:
// a launch on another thread may outlive the process's static destructors.
LaunchLog &g_launch_log = *new LaunchLog();
inline void log_launch(uint32_t family, int g, bool chacha, bool aligned, int form,
                       uint32_t split_log2, uint32_t grid, uint64_t n, uint32_t fine_div = 0,
                       uint64_t items = 0) {
  if (!g_launch_log.on()) return;
  g_launch_log.append(LaunchRec{family, uint32_t(g), chacha, aligned, uint32_t(form), split_log2,
                                grid, fine_div, uint32_t(items), uint32_t(n)});
}

// From a runtime g to the template parameter G: f(integral_constant<int, G>)
// for the one of Gs that g equals, hipErrorInvalidValue when it is none.  A
// left fold: the kernels are instantiated, and so laid out in the code
// object, in the order of Gs (a right fold reverses them).
template <int... Gs, class F>
hipError_t with_g(int g, F &&f) {
  hipError_t e = hipErrorInvalidValue;
  (void)(... || (g == Gs && ((e = f(std::integral_constant<int, Gs>{})), true)));
  return e;
}

// ARX form of the launches above the latency bound: the aligned CID pass
// with no split and G >= 4 (the headline's) runs form 1 (quarter-round
// order), everything else form 2 (step-interleaved; both one asm statement
// per instruction).  Measured on one box, 2 interleaved reps: CID form 1
// headline 992-995 vs 979-983 GiB/s with form 2, config 2 unchanged
// (855-860); the DEK pass is indifferent.
template <int G, bool CHACHA>
hipError_t launch_g(const KArgs &a, bool aligned, hipStream_t s) {
  const dim3 grid(uint32_t(a.n << a.split_log2)), block(256);
  // <= 2 waves per SIMD (512 workgroups of 4 waves on 1024 SIMDs): the
  // compiler-scheduled ARX issues faster than the asm form (tools/arx.hip)
  const bool lat = grid.x <= latency_wgs();
  if (aligned && lat) {
    hipLaunchKernelGGL((k_pass<G, CHACHA, true, 0>), grid, block, 0, s, a);
    log_launch(kLaunchPass, G, CHACHA, true, 0, a.split_log2, grid.x, a.n);
  } else if (aligned) {
    if constexpr (CHACHA) {
      if (G >= 4 && a.split_log2 == 0) {
        hipLaunchKernelGGL((k_pass<G, true, true, 1>), grid, block, 0, s, a);
        log_launch(kLaunchPass, G, true, true, 1, a.split_log2, grid.x, a.n);
        return hipGetLastError();
      }
    }
    hipLaunchKernelGGL((k_pass<G, CHACHA, true, 2>), grid, block, 0, s, a);
    log_launch(kLaunchPass, G, CHACHA, true, 2, a.split_log2, grid.x, a.n);
  } else {
    hipLaunchKernelGGL((k_pass<G, CHACHA, false, 2>), grid, block, 0, s, a);
    log_launch(kLaunchPass, G, CHACHA, false, 2, a.split_log2, grid.x, a.n);
  }
  return hipGetLastError();
}

// Split-mode target: workgroups per launch below which a message is spread
// over more workgroups (fewer chunks per lane).  0 disables split mode
// (glfsx_set_split_target: tests of both forms).
std::atomic<uint32_t> g_split_target{2048u};
PassPlan plan_for(uint64_t n, uint64_t maxlen) {
  return pass_plan(n, maxlen, g_split_target.load(std::memory_order_relaxed), latency_wgs());
}

// What the launches on one (device, stream) keep between them: launches on
// one stream are ordered, so a buffer is never shared by two in flight.  The
// stream-ordered pool (an allocation and a free per launch) serialised the
// Writer's three-stream pipeline (host round trip 43.5 -> 24 GiB/s).  A
// buffer only grows when a launch needs more; the old one is released after
// its stream drains (StreamBuf::ensure).  Every member owns its memory, so
// releasing a slot frees all of it.
struct ScratchSlot {
  StreamBuf p;         // split mode: CVs, 32 B per workgroup
  StreamBuf cnt;       // split mode: arrival counters, 4 B per message, zero
                       // between launches (a message's last workgroup resets its own)
  StreamBuf ready;     // k_pass_dc: per-message DEK ready flags (= epoch)
  uint32_t epoch = 0;
  StreamBuf lists;     // k_pass_dc: 2 banks of work-list counters
  PinnedBlock err;     // k_pass_dc: DEK-wait timeouts (first word)
  StreamBuf dcc;       // k_pass_dc's DcConst
  DcConst dcc_host{};  // what was last copied there
  StreamBuf qctr;      // k_small_q: two banks of its item counter
  uint32_t qepoch = 0;
  StreamBuf rplan;     // ragged post: the plan's prefixes (RArgs::pre, wpre)
  StreamBuf rcv;       // ragged post: chunk and group CVs (RArgs::cvs, gcv)
  PinnedBlock rtot;    // ragged post: the plan's three totals
  StreamBuf open;      // verified read, composed route: digests, plaintext
  StreamBuf oplan;     // ragged open: the plan's prefixes (RArgs::pre, wpre)
  StreamBuf ocv;       // ragged open: chunk and group CVs, 64 B each
  PinnedBlock otot;    // ragged open: the plan's three totals
};
// g_scratch_mu guards the registry and every slot, and is held across a
// getter's whole body, the drain of a growing buffer included: narrowing it
// would change behaviour.  Never destroyed: its slots would free through a
// HIP runtime that may be gone at exit.
std::mutex g_scratch_mu;
StreamRegistry<ScratchSlot> &g_scratch = *new StreamRegistry<ScratchSlot>();

// A getter's common start: s's device made current, the lock taken and the
// slot of (device, s) found or made.
struct SlotLock {
  StreamDevice sd;
  std::unique_lock<std::mutex> lk;
  ScratchSlot *sl = nullptr;
  explicit SlotLock(hipStream_t s, bool make = true) : sd(s) {
    if (sd.e != hipSuccess) return;
    lk = std::unique_lock<std::mutex>(g_scratch_mu);
    sl = make ? g_scratch.find_or_make(sd.dev, s) : g_scratch.find(sd.dev, s);
  }
};

// Split-mode scratch for wgs workgroups and msgs messages.
hipError_t scratch_get(KArgs *a, uint64_t wgs, uint64_t msgs, hipStream_t s) {
  SlotLock g(s);
  if (g.sd.e != hipSuccess) return g.sd.e;
  // at least the default target's worst case, so it rarely grows
  hipError_t e = g.sl->p.ensure(s, size_t(wgs) * 32, size_t(2) << 16, 0, false);
  if (e != hipSuccess) return e;
  e = g.sl->cnt.ensure(s, size_t(msgs) * 4, 4096 * 4, 0, true);
  if (e != hipSuccess) return e;
  a->scratch = g.sl->p.as<uint32_t>();
  a->cnt = g.sl->cnt.as<uint32_t>();
  return hipSuccess;
}

// k_pass_dc's state for a launch over msgs messages on stream s: the ready
// flags and this launch's epoch (flags hold the epoch of the launch that set
// them, so they are never reset; zero is never an epoch), the work-list
// counters (bank epoch & 1, at zero), the error word.
std::atomic<uint64_t> g_dc_wait_ticks{100000000ull};  // 1 s of s_memrealtime
std::atomic<uint32_t> g_dc_skip_msg{~0u};
std::atomic<uint64_t> g_dc_timeouts{0};

constexpr size_t kListWords = 2 * kLists * kListStride;

hipError_t dc_get(uint64_t msgs, hipStream_t s, DcState *d) {
  SlotLock g(s);
  if (g.sd.e != hipSuccess) return g.sd.e;
  ScratchSlot *sl = g.sl;
  // each piece on its own: a failure leaves that piece empty, and the next
  // call makes exactly what is missing
  hipError_t e = sl->lists.ensure(s, kListWords * 4, kListWords * 4, 0, true);
  if (e != hipSuccess) return e;
  e = sl->err.ensure();
  if (e != hipSuccess) return e;
  // when the flags grow the epoch goes on: the new flags are zero
  e = sl->ready.ensure(s, size_t(msgs) * 4, 4096 * 4, 0, true);
  if (e != hipSuccess) return e;
  DcConst want{sl->ready.as<uint32_t>(), sl->lists.as<uint32_t>(),
               static_cast<uint32_t *>(sl->err.d),
               g_dc_wait_ticks.load(std::memory_order_relaxed),
               g_dc_skip_msg.exchange(~0u, std::memory_order_relaxed)};
  if (!sl->dcc.p) {
    e = sl->dcc.ensure(s, sizeof(DcConst), sizeof(DcConst), 0, false);
    if (e != hipSuccess) return e;
    sl->dcc_host = DcConst{};
  }
  const DcConst &h = sl->dcc_host;
  if (want.ready != h.ready || want.lists != h.lists || want.err != h.err ||
      want.wait_ticks != h.wait_ticks || want.skip_msg != h.skip_msg) {
    // rare (new buffers, a test hook): ordered on s before the launch; the
    // copy is staged from pageable memory, so `want` may go out of scope
    e = hipMemcpyAsync(sl->dcc.p, &want, sizeof want, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    sl->dcc_host = want;
  }
  // The epoch advances only here, once nothing before the launch can fail
  // (ADVICE r3): a launch with epoch e clears the counter bank of epoch e+1,
  // so an epoch used up without a launch would leave the bank of e+2 stale.
  // Zero is never an epoch; the bank parity must alternate across the wrap.
  if (++sl->epoch == 0) sl->epoch = 2;
  d->epoch = sl->epoch;
  d->c = sl->dcc.as<DcConst>();
  return hipSuccess;
}

// Both banks of s's work-list counters start over at zero.
void dc_lists_zero(ScratchSlot *sl, hipStream_t s) {
  if (sl && sl->lists.p) (void)hipMemsetAsync(sl->lists.p, 0, kListWords * 4, s);
}

// A k_pass_dc launch failed after dc_get: its epoch was used without the
// launch that clears the next bank.
void dc_launch_failed(hipStream_t s) {
  SlotLock g(s, false);
  dc_lists_zero(g.sl, s);
}

hipError_t launch_quad(KArgs a, uint64_t maxlen, hipStream_t s) {
  const int qpw = quad_qpw(maxlen);
  const uint64_t kSpan = uint64_t(qpw) << 10;
  const uint64_t W = maxlen > kSpan ? (maxlen + kSpan - 1) / kSpan : 1;
  uint32_t sl = 0;
  while ((1ull << sl) < W) ++sl;
  a.split_log2 = sl;
  a.scratch = nullptr;
  a.cnt = nullptr;
  if (sl) {
    hipError_t e = scratch_get(&a, a.n << sl, a.n, s);
    if (e != hipSuccess) return e;
  }
  if (qpw == 64)
    hipLaunchKernelGGL(k_quad<64>, dim3(uint32_t(a.n << sl)), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(k_quad<256>, dim3(uint32_t(a.n << sl)), dim3(1024), 0, s, a);
  log_launch(kLaunchQuad, qpw, false, true, 0, sl, uint32_t(a.n << sl), a.n);
  return hipGetLastError();
}

bool quad_ok(const KArgs &a, uint64_t maxlen, bool aligned, uint32_t sl) {
  const uint64_t chunks = a.n * (maxlen ? (maxlen + 1023) >> 10 : 1);
  const bool refs4 = ((reinterpret_cast<uintptr_t>(a.refs) | a.out_off |
                       a.ref_stride) & 3) == 0;
  return aligned && refs4 && (a.n << sl) <= latency_wgs() &&
         chunks <= 16384 && maxlen <= (64ull * 256) << 10;
}

template <bool CHACHA>
hipError_t launch_pass(KArgs a, uint64_t maxlen, bool aligned,
                       hipStream_t s) {
  const auto [g, sl] = plan_for(a.n, maxlen);
  if constexpr (!CHACHA) {
    if (quad_ok(a, maxlen, aligned, sl)) return launch_quad(a, maxlen, s);
  }
  a.split_log2 = sl;
  a.scratch = nullptr;
  a.cnt = nullptr;
  if (sl) {
    hipError_t e = scratch_get(&a, a.n << sl, a.n, s);
    if (e != hipSuccess) return e;
  }
  return with_g<1, 2, 4, 8, 16, 32, 64>(
      g, [&](auto G) { return launch_g<G(), CHACHA>(a, aligned, s); });
}

// k_small_q's counter banks on stream s and this launch's epoch.
hipError_t small_q_get(hipStream_t s, uint32_t **ctr, uint32_t *epoch) {
  SlotLock g(s);
  if (g.sd.e != hipSuccess) return g.sd.e;
  hipError_t e = g.sl->qctr.ensure(s, 64 * 4, 64 * 4, 0, true);
  if (e != hipSuccess) return e;
  *ctr = g.sl->qctr.as<uint32_t>();
  *epoch = ++g.sl->qepoch;
  return hipSuccess;
}

// Workgroups of kernel k the whole chip holds at once.
template <class K>
uint32_t resident_wgs(K k) {
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 256, 0) != hipSuccess ||
      hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return uint32_t(std::max(per_cu, 1) * std::max(cus, 1));
}

// k_small_q hands out the last 1/kSmallFineDiv of the blobs as fine items.
// 1 M x 4 KiB blobs, 3 interleaved reps: small blobs 911 / 919 / 926 GiB/s
// at none / 1/4 / 1/8, config 4 end to end 780 / 791 / 801.
constexpr uint32_t kSmallFineDiv = 8;

template <int G, bool CHACHA, int A>
hipError_t launch_small_q(const SArgs &a0, hipStream_t s) {
  static const uint32_t slots = resident_wgs(k_small_q<G, CHACHA, A>);
  uint32_t *ctr;
  uint32_t epoch;
  hipError_t e = small_q_get(s, &ctr, &epoch);
  if (e != hipSuccess) return e;
  SArgs a = a0;
  const uint64_t fine = G > 1 ? a.n / kSmallFineDiv : 0;
  a.n_coarse = (a.n - fine) >> 6;  // whole coarse items; the rest goes fine
  const uint64_t rest = a.n - (a.n_coarse << 6), bpi = G > 1 ? 64 / G : 64;
  const uint64_t items = a.n_coarse + (rest + bpi - 1) / bpi;
  const uint64_t wgs = (items + 3) / 4;
  const uint32_t grid = uint32_t(std::min<uint64_t>(wgs, slots ? slots : wgs));
  hipLaunchKernelGGL((k_small_q<G, CHACHA, A>), dim3(grid), dim3(256), 0, s, a, ctr, epoch);
  return hipGetLastError();
}

template <bool CHACHA>
hipError_t launch_small_pass(const SArgs &a, uint64_t max_len, hipStream_t s) {
  const uint64_t C = max_len ? (max_len + 1023) >> 10 : 1;
  const dim3 grid(uint32_t((a.n + 255) / 256)), block(256);
  const int gsel = C <= 1 ? 1 : C <= 2 ? 2 : C <= 4 ? 4 : C <= 8 ? 8 : C <= 16 ? 16 : 0;
  if (grid.x <= latency_wgs())  // few blobs: the compiler's ARX form
    return with_g<1, 2, 4, 8, 16>(gsel, [&](auto G) {
      hipLaunchKernelGGL((k_small<G(), CHACHA, false>), grid, block, 0, s, a);
      return hipGetLastError();
    });
  // more workgroups than the chip holds: per-wave items (k_small_q).  The
  // CID pass runs ARX form 1 (quarter-round order), as the headline's CID
  // pass: 928.8 vs 913.3 GiB/s small blobs, config 4 798.1 vs 787.3 (3
  // interleaved reps, after the wave-offset fix; round 2 measured form 2
  // ahead when half the waves took the per-lane path); the DEK pass form 2
  constexpr int F = CHACHA ? 1 : 2;
  return with_g<1, 2, 4, 8, 16>(
      gsel, [&](auto G) { return launch_small_q<G(), CHACHA, F>(a, s); });
}

// The clock probe (g_clk): off until clock_probe is first called.
std::atomic<bool> g_clk_on{false};
std::atomic<unsigned long long *> g_clk_addr[64];
unsigned long long *clk_words() {
  if (!g_clk_on.load(std::memory_order_relaxed)) return nullptr;
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
  unsigned long long *p = g_clk_addr[d].load(std::memory_order_acquire);
  if (!p) {
    void *q = nullptr;
    if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_clk)) != hipSuccess) return nullptr;
    p = static_cast<unsigned long long *>(q);
    g_clk_addr[d].store(p, std::memory_order_release);
  }
  return p;
}

KArgs make_args(const PostJob &job) {
  KArgs a{};
  a.clk = clk_words();
  a.src = job.src;
  a.ctext = job.ctext;
  a.stride = job.stride;
  a.msg_len = job.msg_len;
  a.last_len = job.last_len;
  a.n = job.n;
  a.refs = job.out.refs;
  a.ref_bf = job.out.bf;
  a.ref_stride = job.out.stride;
  return a;
}

bool is_aligned(const PostJob &job) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(job.src) |
                      reinterpret_cast<uintptr_t>(job.ctext) |
                      uintptr_t(job.stride);
  return (x & 15) == 0;
}

}  // namespace

void words_from_key(uint32_t w[8], const uint8_t key[32]) {
  for (int i = 0; i < 8; ++i)
    w[i] = uint32_t(key[4 * i]) | (uint32_t(key[4 * i + 1]) << 8) |
           (uint32_t(key[4 * i + 2]) << 16) | (uint32_t(key[4 * i + 3]) << 24);
}

uint32_t set_split_target(uint32_t wgs) { return g_split_target.exchange(wgs); }

uint32_t set_latency_wgs(uint32_t wgs) { return g_latency_wgs.exchange(wgs); }

void release_stream_scratch(hipStream_t s) {
  SlotLock g(s, false);
  if (g.sl) g_scratch.release(g.sd.dev, s);
}

uint32_t fused_errors_take(hipStream_t s) {
  SlotLock g(s, false);
  if (!g.sl || !g.sl->err.h) return 0;
  const uint32_t v =
      __atomic_exchange_n(static_cast<uint32_t *>(g.sl->err.h), 0u, __ATOMIC_ACQ_REL);
  if (v) {
    g_dc_timeouts.fetch_add(1, std::memory_order_relaxed);
    // a failed launch may leave its counters off zero (it zeroes the other
    // bank)
    dc_lists_zero(g.sl, s);
  }
  return v;
}

void fused_debug(uint32_t skip_msg, uint64_t wait_us) {
  g_dc_skip_msg.store(skip_msg, std::memory_order_relaxed);
  g_dc_wait_ticks.store(wait_us ? wait_us * 100 : 100000000ull, std::memory_order_relaxed);
}

uint64_t fused_timeouts() { return g_dc_timeouts.load(std::memory_order_relaxed); }

void blake3_iv_words(uint32_t w[8]) {
  for (int i = 0; i < 8; ++i) w[i] = kIV[i];
}

hipError_t launch_keyed_hash(const PostJob &job, uint32_t out_off,
                             hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  KArgs a = make_args(job);
  for (int i = 0; i < 8; ++i) a.key[i] = job.salt[i];
  a.base = kKeyed;
  a.out_off = out_off;
  const uint64_t maxlen = job.n > 1 ? std::max(job.msg_len, job.last_len)
                                    : job.last_len;
  return launch_pass<false>(a, maxlen, is_aligned(job), s);
}

// The fine-item share of k_pass_dc's CID items: the last ceil(m / 4)
// messages of each work list.
constexpr uint32_t kDcFineDiv = 4;

// Split-mode post of many-wave size in one launch (k_pass_dc): both passes
// of launch_keyed_hash + launch_cid_pass when each would be one k_pass<G,
// CHACHA, true, 2> launch with the same plan.
hipError_t launch_post_fused(const PostJob &job, hipStream_t s, bool *done) {
  *done = false;
  if (job.n < 2 || !is_aligned(job)) return hipSuccess;
  if ((reinterpret_cast<uintptr_t>(job.out.refs) | job.out.stride) & 3) return hipSuccess;
  const uint64_t maxlen = std::max(job.msg_len, job.last_len);
  const PassPlan plan = plan_for(job.n, maxlen);
  const int g = plan.g;
  const uint32_t sl = plan.sl;
  const uint64_t wgs = job.n << sl;
  // launches of 320-512 workgroups (default threshold) also run fused in the
  // many-wave form: Create of 96 / 128 MiB at 1 MiB blocks (384 / 512
  // workgroups) 359 -> 368 / 451 -> 487 GiB/s, 80 MiB a tie, 64 MiB (256)
  // 6 % slower, so it stays in latency mode (scripts/lat_thr.py)
  if (sl == 0 || wgs * 8 <= uint64_t(latency_wgs()) * 5 || (g != 1 && g != 2 && g != 4))
    return hipSuccess;
  const uint64_t chunks = job.n * ((maxlen + 1023) >> 10);
  KArgs a = make_args(job);
  for (int i = 0; i < 8; ++i) a.key[i] = job.salt[i];
  a.base = kKeyed;
  a.out_off = 32;
  if (quad_ok(a, maxlen, true, sl) || chunks == 0) return hipSuccess;
  a.split_log2 = sl;
  // scratch: DEK CVs (wgs), coarse CID CVs (wgs), fine CID CVs (2 wgs)
  hipError_t e = scratch_get(&a, 4 * wgs, 2 * job.n, s);
  if (e != hipSuccess) return e;
  DcState d{};
  e = dc_get(job.n, s, &d);
  if (e != hipSuccess) return e;
  d.n = uint32_t(job.n);
  d.sl = sl;
  d.fine_div = (g > 1 && sl < kMaxSplitLog2) ? kDcFineDiv : 0u;
  KArgs b = a;
  for (int i = 0; i < 8; ++i) b.key[i] = job.cid_key[i];
  b.base = job.cid_keyed ? kKeyed : 0u;
  b.out_off = 0;
  b.scratch = a.scratch + wgs * 8;
  b.cnt = a.cnt + job.n;
  KArgs c = b;  // fine CID items: twice the workgroups per message
  c.split_log2 = sl + 1;
  c.scratch = b.scratch + wgs * 8;
  uint64_t items = 0;
  for (uint32_t x = 0; x < kLists; ++x) {
    const uint32_t m = dc_list_msgs(d.n, x);
    items += dc_list_items(m, dc_list_fine(m, d.fine_div), sl);
  }
  const dim3 grid{uint32_t(items)}, block{256};
  e = with_g<1, 2, 4>(g, [&](auto G) {
    hipLaunchKernelGGL(k_pass_dc<G()>, grid, block, 0, s, a, b, c, d);
    log_launch(kLaunchPassDc, G(), true, true, 2, sl, grid.x, job.n, d.fine_div, items);
    return hipGetLastError();
  });
  *done = true;
  if (e != hipSuccess) dc_launch_failed(s);
  return e;
}

hipError_t launch_post(const PostJob &job, hipStream_t s, bool fused) {
  if (job.n == 0) return hipSuccess;
  bool done = false;
  hipError_t e = fused ? launch_post_fused(job, s, &done) : hipSuccess;
  if (e != hipSuccess || done) return e;
  e = launch_keyed_hash(job, 32, s);
  if (e != hipSuccess) return e;
  return launch_cid_pass(job, s);
}

hipError_t launch_cid_pass(const PostJob &job, hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  KArgs a = make_args(job);
  for (int i = 0; i < 8; ++i) a.key[i] = job.cid_key[i];
  a.base = job.cid_keyed ? kKeyed : 0u;
  a.out_off = 0;
  const uint64_t maxlen = job.n > 1 ? std::max(job.msg_len, job.last_len)
                                    : job.last_len;
  const uint32_t sl = plan_for(job.n, maxlen).sl;
  // Latency-bound launches (index nodes, single posts, small batches): the
  // fused pass leaves one wave per SIMD running ChaCha20 and BLAKE3 in
  // series.  The keystream has no chaining, so instead every 64-B block gets
  // its own lane (the read side's kernels: ctext = ptext ^ ChaCha20(DEK_j)),
  // and the CID is a BLAKE3 pass over the ctext like the DEK pass.  Needs
  // the ctext in memory, DEKs in dense slots, contiguous messages.
  const bool dense = job.out.bf >= job.n;
  const bool contiguous = job.n == 1 || job.stride == job.msg_len;
  if ((job.n << sl) <= latency_wgs() && job.ctext && dense && contiguous &&
      (job.n == 1 || job.msg_len % 64 == 0)) {
    const uint64_t bs = job.n > 1 ? job.msg_len
                                  : std::max<uint64_t>(4096, (job.last_len + 4095) & ~4095ull);
    hipError_t e = launch_decrypt(job.src, job.ctext, job.n, bs, job.last_len,
                                  job.out.refs, s);
    if (e != hipSuccess) return e;
    KArgs b = a;
    b.src = job.ctext;
    b.ctext = nullptr;
    const bool aligned = ((reinterpret_cast<uintptr_t>(job.ctext) |
                           uintptr_t(job.stride)) & 15) == 0;
    return launch_pass<false>(b, maxlen, aligned, s);
  }
  return launch_pass<true>(a, maxlen, is_aligned(job), s);
}

hipError_t launch_fill(uint8_t *dst, uint64_t offset, uint64_t n, uint64_t seed,
                       hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (offset & 7) return hipErrorInvalidValue;
  const uint64_t words = (n + 7) >> 3;
  uint64_t grid = (words + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(k_fill, dim3(uint32_t(grid)), dim3(256), 0, s, dst, offset,
                     n, seed);
  return hipGetLastError();
}

hipError_t launch_post_small(const SmallJob &job, hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  // blobs above small_max are skipped by k_small (posted elsewhere)
  const uint64_t small_max = job.small_max ? std::min(job.small_max, kMaxSmallLen)
                                           : kMaxSmallLen;
  const uint64_t max_len = std::min(job.max_len, small_max);
  SArgs a{};
  a.small_max = small_max;
  a.src = job.src;
  a.ctext = job.ctext;
  a.offs = job.offs;
  a.lens = job.lens;
  a.n = job.n;
  a.refs = job.refs;
  for (int i = 0; i < 8; ++i) {
    a.key[i] = job.raw_salt[i];
    a.key0[i] = job.index_salt[i];
  }
  a.base = kKeyed;
  a.out_off = 32;
  hipError_t e = hipSuccess;
  if (job.passes != 2) {
    e = launch_small_pass<false>(a, max_len, s);
    if (e != hipSuccess || job.passes == 1) return e;
  }
  for (int i = 0; i < 8; ++i) a.key[i] = a.key0[i] = job.cid_key[i];
  a.base = job.cid_keyed ? kKeyed : 0u;
  a.out_off = 0;
  a.hex_out = job.hex_out;
  a.hex_pos = job.hex_pos;
  if (job.cid_wait) {  // e.g. the tree lines' static parts, on another stream
    e = hipStreamWaitEvent(s, job.cid_wait, 0);
    if (e != hipSuccess) return e;
  }
  return launch_small_pass<true>(a, max_len, s);
}

// The buffers sized by a call's data (ragged post, verified read) start at
// 1 MiB and grow with a quarter of headroom.
constexpr size_t kGrowFloor = size_t(1) << 20;

// The ragged post's buffers on stream s: `plan` / `cv` bytes (0: leave that
// one alone) and the pinned words for the plan's totals.
static hipError_t rag_get(hipStream_t s, size_t plan, size_t cv, uint8_t **d_plan,
                          uint8_t **d_cv, uint64_t **tot, uint64_t **d_tot) {
  SlotLock g(s);
  if (g.sd.e != hipSuccess) return g.sd.e;
  hipError_t e = g.sl->rtot.ensure();
  if (e != hipSuccess) return e;
  e = g.sl->rplan.ensure(s, plan, kGrowFloor, 4, false);
  if (e != hipSuccess) return e;
  e = g.sl->rcv.ensure(s, cv, kGrowFloor, 4, false);
  if (e != hipSuccess) return e;
  *d_plan = g.sl->rplan.as<uint8_t>();
  *d_cv = g.sl->rcv.as<uint8_t>();
  *tot = static_cast<uint64_t *>(g.sl->rtot.h);
  *d_tot = static_cast<uint64_t *>(g.sl->rtot.d);
  return hipSuccess;
}

template <bool CHACHA>
static hipError_t launch_rag_chunk(const RArgs &a, hipStream_t s) {
  const uint64_t tiles = (a.total + 255) >> 8;
  const dim3 grid(uint32_t(std::min<uint64_t>(tiles, 1u << 20))), block(256);
  // few tiles: the compiler's ARX form, as launch_g
  if (tiles <= latency_wgs())
    hipLaunchKernelGGL((k_rag_chunk<CHACHA, 0>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_rag_chunk<CHACHA, 2>), grid, block, 0, s, a);
  return hipGetLastError();
}

// One pass of the ragged post: the chunks, then the merge levels that have
// work (tot: chunks, merge groups, messages of more than 256 chunks).
template <bool CHACHA>
static hipError_t launch_rag_pass(RArgs a, const uint64_t tot[3], hipStream_t s) {
  a.total = tot[0];
  hipError_t e = launch_rag_chunk<CHACHA>(a, s);
  if (e != hipSuccess) return e;
  if (tot[1]) {
    a.total = tot[1];
    hipLaunchKernelGGL(k_rag_merge_a, dim3(uint32_t(std::min<uint64_t>(tot[1], 1u << 20))),
                       dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (tot[2]) {
    a.total = tot[2];
    hipLaunchKernelGGL(k_rag_merge_b, dim3(uint32_t(std::min<uint64_t>(tot[2], 1u << 20))),
                       dim3(256), 0, s, a);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_post_ragged(const RaggedJob &job, hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  if (job.hi > kMaxRaggedLen) return hipErrorInvalidValue;
  RArgs a{};
  a.src = job.src;
  a.ctext = job.ctext;
  a.offs = job.offs;
  a.lens = job.lens;
  a.n = job.n;
  a.lo = job.lo;
  a.hi = job.hi;
  a.refs = job.refs;
  a.m = (job.n + kRagWG - 1) / kRagWG;
  uint8_t *d_plan, *d_cv;
  uint64_t *tot, *d_tot;
  hipError_t e = rag_get(s, 8 * (job.n + 3 * (a.m + 1)), 0, &d_plan, &d_cv, &tot, &d_tot);
  if (e != hipSuccess) return e;
  a.pre = reinterpret_cast<uint64_t *>(d_plan);
  a.wpre = a.pre + job.n;
  hipLaunchKernelGGL(k_rag_count<false>, dim3(uint32_t(a.m)), dim3(kRagWG), 0, s, a,
                     static_cast<uint32_t *>(nullptr), 0u);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rag_prefix<1024>, dim3(3), dim3(1024), 0, s, a.wpre, a.m, d_tot);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the one host wait of the call: the totals size the CV scratch and the
  // launches below
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  const uint64_t totals[3] = {__atomic_load_n(tot + 0, __ATOMIC_RELAXED),
                              __atomic_load_n(tot + 1, __ATOMIC_RELAXED),
                              __atomic_load_n(tot + 2, __ATOMIC_RELAXED)};
  if (totals[0] == 0) return hipSuccess;  // nothing selected
  e = rag_get(s, 0, 32 * (totals[0] + totals[1]), &d_plan, &d_cv, &tot, &d_tot);
  if (e != hipSuccess) return e;
  a.cvs = reinterpret_cast<uint32_t *>(d_cv);
  a.gcv = a.cvs + 8 * totals[0];
  for (int i = 0; i < 8; ++i) a.key[i] = job.salt[i];
  a.base = kKeyed;
  a.out_off = 32;
  e = launch_rag_pass<false>(a, totals, s);
  if (e != hipSuccess) return e;
  for (int i = 0; i < 8; ++i) a.key[i] = job.cid_key[i];
  a.base = job.cid_keyed ? kKeyed : 0u;
  a.out_off = 0;
  return launch_rag_pass<true>(a, totals, s);
}

#if GLFSX_ONE_TIMING
extern "C" int glfsx_debug_one_timing(int reset, uint64_t out[16]) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_one_t), 16 * sizeof(uint64_t), 0,
                          hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  if (!reset) return 0;
  const unsigned long long z[16] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_one_t), z, sizeof z, 0, hipMemcpyHostToDevice) ==
                 hipSuccess ? 0 : -1;
}
#endif

size_t pass_log(int reset, uint32_t *out, size_t cap) {
  if (!g_launch_log.on()) g_launch_log.enable();
  return g_launch_log.read(reset != 0, out, cap);
}

hipError_t clock_probe(int reset, uint64_t out[2]) {
  g_clk_on.store(true, std::memory_order_relaxed);
  unsigned long long v[2] = {0, 0};
  hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(g_clk), sizeof v, 0, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  if (out) {
    out[0] = v[0];
    out[1] = v[1];
  }
  if (!reset) return hipSuccess;
  const unsigned long long z[2] = {0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_clk), z, sizeof z, 0, hipMemcpyHostToDevice);
}

#if GLFSX_WGTIME
hipError_t debug_wgtime(uint64_t *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgtime), sizeof(g_wgtime), 0,
                             hipMemcpyDeviceToHost);
}
#endif

hipError_t launch_med(const OneDesc *descs, uint32_t n, uint64_t max_len,
                      hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (max_len > kMaxMedLen || max_len <= kMaxOneLen) return hipErrorInvalidValue;
  const uint32_t wmax = uint32_t((max_len + 65535) >> 16);
  hipLaunchKernelGGL(k_med_dek, dim3(n * wmax), dim3(256), 0, s, descs, wmax);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_med_cid, dim3(n * wmax), dim3(256), 0, s, descs, wmax);
  return hipGetLastError();
}

hipError_t launch_one(const OneDesc *descs, uint32_t n, uint64_t max_len,
                      hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (max_len > kMaxOneLen) return hipErrorInvalidValue;
  if (max_len <= 16 * 1024)
    hipLaunchKernelGGL(k_one<16>, dim3(n), dim3(64), 0, s, descs);
  else
    hipLaunchKernelGGL(k_one<64>, dim3(n), dim3(256), 0, s, descs);
  return hipGetLastError();
}

hipError_t launch_med_v(const OneDesc &d, hipStream_t s) {
  if (d.len > kMaxMedLen || d.len <= kMaxOneLen) return hipErrorInvalidValue;
  const uint32_t wmax = uint32_t((uint64_t(d.len) + 65535) >> 16);
  hipLaunchKernelGGL(k_med_dek_v, dim3(wmax), dim3(256), 0, s, d, wmax);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_med_cid_v, dim3(wmax), dim3(256), 0, s, d, wmax);
  return hipGetLastError();
}

hipError_t launch_one_v(const OneDesc &d, hipStream_t s) {
  if (d.len > kMaxOneLen) return hipErrorInvalidValue;
  if (d.len <= 16 * 1024)
    hipLaunchKernelGGL(k_one_v<16>, dim3(1), dim3(64), 0, s, d);
  else
    hipLaunchKernelGGL(k_one_v<64>, dim3(1), dim3(256), 0, s, d);
  return hipGetLastError();
}

// k_one_open's workgroup: four lanes per quad, two trees when salted.
template <int QUADS, bool SALTED>
constexpr uint32_t one_open_lanes() {
  return QUADS * (SALTED ? 8 : 4);
}

hipError_t launch_one_open(const OneOpenDesc *descs, uint32_t n, uint64_t max_len, bool salted,
                           hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (max_len > kMaxOneLen) return hipErrorInvalidValue;
  const bool small = max_len <= 16 * 1024;
  if (salted && small)
    hipLaunchKernelGGL((k_one_open<16, true>), dim3(n), dim3(one_open_lanes<16, true>()), 0, s,
                       descs);
  else if (salted)
    hipLaunchKernelGGL((k_one_open<64, true>), dim3(n), dim3(one_open_lanes<64, true>()), 0, s,
                       descs);
  else if (small)
    hipLaunchKernelGGL((k_one_open<16, false>), dim3(n), dim3(one_open_lanes<16, false>()), 0, s,
                       descs);
  else
    hipLaunchKernelGGL((k_one_open<64, false>), dim3(n), dim3(one_open_lanes<64, false>()), 0, s,
                       descs);
  return hipGetLastError();
}

hipError_t launch_one_open_v(const OneOpenDesc &d, bool salted, hipStream_t s) {
  if (d.len > kMaxOneLen) return hipErrorInvalidValue;
  const bool small = d.len <= 16 * 1024;
  if (salted && small)
    hipLaunchKernelGGL((k_one_open_v<16, true>), dim3(1), dim3(one_open_lanes<16, true>()), 0, s,
                       d);
  else if (salted)
    hipLaunchKernelGGL((k_one_open_v<64, true>), dim3(1), dim3(one_open_lanes<64, true>()), 0, s,
                       d);
  else if (small)
    hipLaunchKernelGGL((k_one_open_v<16, false>), dim3(1), dim3(one_open_lanes<16, false>()), 0,
                       s, d);
  else
    hipLaunchKernelGGL((k_one_open_v<64, false>), dim3(1), dim3(one_open_lanes<64, false>()), 0,
                       s, d);
  return hipGetLastError();
}

hipError_t launch_decrypt(const uint8_t *ctext, uint8_t *ptext, uint64_t n,
                          uint64_t bs, uint64_t last_len, const uint8_t *refs,
                          hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (bs % 64) return hipErrorInvalidValue;
  KArgs a{};
  a.src = ctext;
  a.ctext = ptext;
  a.msg_len = bs;
  a.last_len = last_len;
  a.n = n;
  a.refs = const_cast<uint8_t *>(refs);
  const uint64_t total = (n - 1) * bs + last_len;
  const uint64_t kbs = (total + 63) >> 6;
  // bulk: whole 4 KiB units through the line kernel (uniform DEK per unit)
  uint64_t units = 0;
  if (bs % 4096 == 0 && ((reinterpret_cast<uintptr_t>(ctext) |
                          reinterpret_cast<uintptr_t>(ptext)) & 15) == 0)
    units = total >> 12;
  if (units) {
    const uint64_t upb = bs >> 12;
    const uint32_t upb_shift =
        (upb & (upb - 1)) == 0 ? uint32_t(__builtin_ctzll(upb)) : 64u;
    // runs of 2^run_shift units per wave (inside one block), as long as
    // there are still >= 65536 runs: the grid (<= 16384 workgroups of 4
    // waves) stays as fine-grained as with one unit per step
    uint32_t run_shift = 0;
    if (upb_shift < 64)
      while (run_shift < upb_shift && (units >> (run_shift + 1)) >= 65536) ++run_shift;
    const uint64_t runs = (units + (1ull << run_shift) - 1) >> run_shift;
    uint64_t grid = (runs + 3) / 4;
    if (grid > 16384) grid = 16384;
    if (grid <= latency_wgs())
      hipLaunchKernelGGL(k_decrypt_lines<0>, dim3(uint32_t(grid)), dim3(256), 0, s,
                         a, units, upb_shift, run_shift);
    else
      hipLaunchKernelGGL(k_decrypt_lines<2>, dim3(uint32_t(grid)), dim3(256), 0, s,
                         a, units, upb_shift, run_shift);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  a.stride = units << 6;  // first keystream block left for k_decrypt
  if (a.stride >= kbs) return hipSuccess;
  uint64_t grid = (kbs - a.stride + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(k_decrypt, dim3(uint32_t(grid)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_chacha_xor(const uint32_t k[8], const uint8_t *src,
                             uint8_t *dst, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  KArgs a{};
  a.src = src;
  a.ctext = dst;
  a.msg_len = n;
  for (int i = 0; i < 8; ++i) a.key[i] = k[i];
  const uint64_t nblk = (n + 63) >> 6;
  uint64_t grid = (nblk + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(k_chacha_xor, dim3(uint32_t(grid)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- The verified read (open_kernels.h) ----

// Route of launch_open: 0 auto, 1 always composed, 2 fused wherever k_open
// is able (glfsx_set_open_route: tests and measurements of both).
static std::atomic<int> g_open_route{0};
int set_open_route(int route) {
  if (route < 0 || route > 2) return g_open_route.load(std::memory_order_relaxed);
  return g_open_route.exchange(route, std::memory_order_relaxed);
}

// Where auto takes the fused route: only at shapes whose neighbours in the
// sweep of scripts/open_rate.py had k_open's median at or above the composed
// route's in the same run (profiles/open/open_rate.json, DESIGN.md "k_open --
// the verified read").  From 1024 blocks on (one workgroup per block then
// fills every CU's four slots; at 512 the two routes tie and at 256 the
// composed one wins by a fifth), blocks of at least 256 KiB (at 64 KiB only
// one wave of a workgroup has chunks: 0.84 of composed), and 1 GiB in all
// (the smallest total measured at each block size).
constexpr uint64_t kOpenFusedMinBlocks = 1024;
constexpr uint64_t kOpenFusedMinBs = 256ull << 10;
constexpr uint64_t kOpenFusedMinBytes = 1ull << 30;
constexpr uint64_t kOpenFusedMaxBs = 2ull << 20;  // 256 lanes x 8 chunks

// The composed route's scratch on stream s: `bytes`.
static hipError_t open_get(hipStream_t s, size_t bytes, uint8_t **p) {
  SlotLock g(s);
  if (g.sd.e != hipSuccess) return g.sd.e;
  hipError_t e = g.sl->open.ensure(s, bytes, kGrowFloor, 4, false);
  *p = g.sl->open.as<uint8_t>();
  return e;
}

template <int G>
static hipError_t launch_open_g(const OArgs &a, bool aligned, hipStream_t s) {
  const dim3 grid(uint32_t(a.n)), block(256);
  if (aligned)
    hipLaunchKernelGGL((k_open<G, true, 2>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_open<G, false, 2>), grid, block, 0, s, a);
  log_launch(kLaunchOpen, G, true, aligned, 2, 0, grid.x, a.n);
  return hipGetLastError();
}

// Existing launches plus k_open_compare: the CID of the ctext and, when
// salted, the DEK of the decrypted plaintext go to a 64-B slot per block,
// which the last kernel compares with the refs.
static hipError_t launch_open_composed(const OpenJob &job, hipStream_t s) {
  const uint64_t total = (job.n - 1) * job.bs + job.last_len;
  const bool own_pt = !job.ptext && job.salted;
  const size_t dig = size_t(job.n) * 64;
  uint8_t *scr;
  hipError_t e = open_get(s, dig + (own_pt ? size_t(total) + 64 : 0), &scr);
  if (e != hipSuccess) return e;
  uint8_t *pt = own_pt ? scr + dig : job.ptext;
  const uint64_t maxlen = job.n > 1 ? job.bs : job.last_len;
  PostJob pj{};
  pj.src = job.ctext;
  pj.stride = pj.msg_len = job.bs;
  pj.last_len = job.last_len;
  pj.n = job.n;
  pj.out = RefLayout{scr, ~0ull, 0};
  KArgs a = make_args(pj);
  for (int i = 0; i < 8; ++i) a.key[i] = job.cid_key[i];
  a.base = job.cid_keyed ? kKeyed : 0u;
  a.out_off = 0;
  e = launch_pass<false>(a, maxlen, is_aligned(pj), s);
  if (e != hipSuccess) return e;
  if (pt) {
    e = launch_decrypt(job.ctext, pt, job.n, job.bs, job.last_len, job.refs, s);
    if (e != hipSuccess) return e;
  }
  if (job.salted) {
    pj.src = pt;
    for (int i = 0; i < 8; ++i) pj.salt[i] = job.salt[i];
    e = launch_keyed_hash(pj, 32, s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_open_compare, dim3(uint32_t((job.n + 255) / 256)), dim3(256), 0, s,
                     scr, job.refs, job.status, job.n, job.salted ? 1u : 0u);
  return hipGetLastError();
}

hipError_t launch_open(const OpenJob &job, hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  if (job.bs % 64 || job.bs > kMaxMsgLen || job.last_len > job.bs || job.n > 0x7fffffffull)
    return hipErrorInvalidValue;
  const int route = g_open_route.load(std::memory_order_relaxed);
  const bool able = job.salted && job.bs <= kOpenFusedMaxBs;
  const bool wins = job.n >= kOpenFusedMinBlocks && job.bs >= kOpenFusedMinBs &&
                    job.n * job.bs >= kOpenFusedMinBytes;
  if (!able || route == 1 || (route == 0 && !wins)) return launch_open_composed(job, s);
  OArgs a{};
  a.ctext = job.ctext;
  a.ptext = job.ptext;
  a.n = job.n;
  a.bs = job.bs;
  a.last_len = job.last_len;
  a.refs = job.refs;
  a.status = job.status;
  for (int i = 0; i < 8; ++i) {
    a.salt[i] = job.salt[i];
    a.cid_key[i] = job.cid_key[i];
  }
  a.cid_base = job.cid_keyed ? kKeyed : 0u;
  const bool aligned = ((reinterpret_cast<uintptr_t>(job.ctext) |
                         reinterpret_cast<uintptr_t>(job.ptext) | uintptr_t(job.bs)) & 15) == 0;
  const uint64_t C = (job.bs + 1023) >> 10;
  const int g = C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8;
  return with_g<1, 2, 4, 8>(g, [&](auto G) { return launch_open_g<G()>(a, aligned, s); });
}

// ---- The ragged open (ragged_open_kernels.h) ----

// The ragged open's buffers on stream s, in rag_get's form.
static hipError_t rag_open_get(hipStream_t s, size_t plan, size_t cv, uint8_t **d_plan,
                               uint8_t **d_cv, uint64_t **tot, uint64_t **d_tot) {
  SlotLock g(s);
  if (g.sd.e != hipSuccess) return g.sd.e;
  hipError_t e = g.sl->otot.ensure();
  if (e != hipSuccess) return e;
  e = g.sl->oplan.ensure(s, plan, kGrowFloor, 4, false);
  if (e != hipSuccess) return e;
  e = g.sl->ocv.ensure(s, cv, kGrowFloor, 4, false);
  if (e != hipSuccess) return e;
  *d_plan = g.sl->oplan.as<uint8_t>();
  *d_cv = g.sl->ocv.as<uint8_t>();
  *tot = static_cast<uint64_t *>(g.sl->otot.h);
  *d_tot = static_cast<uint64_t *>(g.sl->otot.d);
  return hipSuccess;
}

// The chunk pass and the merge levels that have work, in mode MODE.
template <int MODE>
static hipError_t launch_rag_open_pass(ROArgs a, const uint64_t tot[3], hipStream_t s) {
  a.r.total = tot[0];
  const uint64_t tiles = (tot[0] + 255) >> 8;
  const dim3 grid(uint32_t(std::min<uint64_t>(tiles, 1u << 20))), block(256);
  // few tiles: the compiler's ARX form, as launch_rag_chunk
  if (tiles <= latency_wgs())
    hipLaunchKernelGGL((k_rag_open_chunk<MODE, 0>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_rag_open_chunk<MODE, 2>), grid, block, 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (tot[1]) {
    a.r.total = tot[1];
    hipLaunchKernelGGL(k_rag_open_merge_a<MODE == 2>,
                       dim3(uint32_t(std::min<uint64_t>(tot[1], 1u << 20))), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (tot[2]) {
    a.r.total = tot[2];
    hipLaunchKernelGGL(k_rag_open_merge_b<MODE == 2>,
                       dim3(uint32_t(std::min<uint64_t>(tot[2], 1u << 20))), dim3(256), 0, s, a);
    e = hipGetLastError();
  }
  return e;
}

hipError_t launch_open_ragged(const OpenRaggedJob &job, hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  if (job.max_len > kMaxRaggedLen) return hipErrorInvalidValue;
  ROArgs a{};
  a.r.src = job.ctext;
  a.r.ctext = job.ptext;
  a.r.offs = job.offs;
  a.r.lens = job.lens;
  a.r.n = job.n;
  a.r.lo = kRaggedAll;
  a.r.hi = job.max_len;
  a.r.refs = const_cast<uint8_t *>(job.refs);
  a.r.m = (job.n + kRagWG - 1) / kRagWG;
  a.status = job.status;
  uint8_t *d_plan, *d_cv;
  uint64_t *tot, *d_tot;
  hipError_t e = rag_open_get(s, 8 * (job.n + 3 * (a.r.m + 1)), 0, &d_plan, &d_cv, &tot, &d_tot);
  if (e != hipSuccess) return e;
  a.r.pre = reinterpret_cast<uint64_t *>(d_plan);
  a.r.wpre = a.r.pre + job.n;
  // a message above max_len is neither read nor written: it fails closed
  hipLaunchKernelGGL(k_rag_count<true>, dim3(uint32_t(a.r.m)), dim3(kRagWG), 0, s, a.r,
                     job.status, 1u /* GLFSX_BAD_CID */);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rag_prefix<1024>, dim3(3), dim3(1024), 0, s, a.r.wpre, a.r.m, d_tot);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the one host wait of the call: the totals size the CV scratch and the
  // launches below
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  const uint64_t totals[3] = {__atomic_load_n(tot + 0, __ATOMIC_RELAXED),
                              __atomic_load_n(tot + 1, __ATOMIC_RELAXED),
                              __atomic_load_n(tot + 2, __ATOMIC_RELAXED)};
  if (totals[0] == 0) return hipSuccess;  // nothing selected
  e = rag_open_get(s, 0, 64 * (totals[0] + totals[1]), &d_plan, &d_cv, &tot, &d_tot);
  if (e != hipSuccess) return e;
  a.r.cvs = reinterpret_cast<uint32_t *>(d_cv);
  a.r.gcv = a.r.cvs + 16 * totals[0];
  for (int i = 0; i < 8; ++i) {
    a.r.key[i] = job.cid_key[i];
    a.salt[i] = job.salt[i];
  }
  a.r.base = job.cid_keyed ? kKeyed : 0u;
  if (job.salted) return launch_rag_open_pass<2>(a, totals, s);
  if (job.ptext) return launch_rag_open_pass<1>(a, totals, s);
  return launch_rag_open_pass<0>(a, totals, s);
}

}  // namespace glfsx
