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
// The host half below the fragments builds the kernel arguments, asks
// launch_plan.h (pure functions) which kernel runs with what shape, fetches
// scratch and launches.  What a stream's launches keep between them is one
// ScratchSlot per (device, stream) whose members own their memory.
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <utility>

#include "device_common.h"
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

// The tuning values (launch_plan.h: Knobs), read once per call.
std::atomic<uint32_t> g_latency_wgs{512}, g_split_target{2048u};
Knobs knobs() {
  return {g_split_target.load(std::memory_order_relaxed),
          g_latency_wgs.load(std::memory_order_relaxed)};
}

// The launch log (glfsx_debug_pass_log): off until first asked for; then
// every bulk launch appends the record it was made from.  Never destroyed:
// a launch on another thread may outlive the process's static destructors.
LaunchLog &g_launch_log = *new LaunchLog();
// The aux log (glfsx_debug_aux_log), a log of its own so that the pass log
// keeps its content: the small-blob launches (launch_small_pass), the
// decrypt launches (decrypt_with, the latency-mode posts' keystream leg too),
// the ragged levels (launch_rag_levels) and the one-shot classes
// (launch_one_class).
LaunchLog &g_aux_log = *new LaunchLog();

// f(integral_constant<int, G>) for the G of Gs (a constexpr array of
// launch_plan.h) that g equals, hipErrorInvalidValue when it is none.
template <const auto &Gs, class F, size_t... I>
hipError_t with_g(uint32_t g, F &&f, std::index_sequence<I...>) {
  hipError_t e = hipErrorInvalidValue;
  (void)(... || (g == uint32_t(Gs[I]) && ((e = f(std::integral_constant<int, Gs[I]>{})), true)));
  return e;
}
template <const auto &Gs, class F>
hipError_t with_g(uint32_t g, F &&f) {
  return with_g<Gs>(g, f, std::make_index_sequence<std::size(Gs)>{});
}

// k_pass<G, CHACHA, ALIGNED, A> when that is r's instantiation and launchable.
template <int G, bool CHACHA, bool ALIGNED, int A>
bool try_pass(const LaunchRec &r, const KArgs &a, hipStream_t s) {
  if constexpr (pass_form_ok(G, CHACHA, ALIGNED, A)) {
    if (r.chacha == CHACHA && r.aligned == ALIGNED && r.form == A) {
      hipLaunchKernelGGL((k_pass<G, CHACHA, ALIGNED, A>), dim3(r.grid), dim3(256), 0, s, a);
      return true;
    }
  }
  return false;
}
template <int G, bool CHACHA>
bool try_pass_g(const LaunchRec &r, const KArgs &a, hipStream_t s) {
  return try_pass<G, CHACHA, true, 0>(r, a, s) || try_pass<G, CHACHA, true, 1>(r, a, s) ||
         try_pass<G, CHACHA, true, 2>(r, a, s) || try_pass<G, CHACHA, false, 2>(r, a, s);
}

// What the launches on one (device, stream) keep between them: launches on
// one stream are ordered, so a buffer is never shared by two in flight.  The
// stream-ordered pool (an allocation and a free per launch) serialised the
// Writer's three-stream pipeline (host round trip 43.5 -> 24 GiB/s).  A
// buffer only grows when a launch needs more; the old one is released after
// its stream drains (StreamBuf::ensure).  Every member owns its memory, so
// releasing a slot frees all of it.
struct RagBufs {
  StreamBuf plan;   // the plan's prefixes (RArgs::pre, wpre)
  StreamBuf cv;     // chunk and group CVs (RArgs::cvs, gcv)
  PinnedBlock tot;  // the plan's three totals
};
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
  RagBufs rag;         // ragged post (CVs of 32 B)
  StreamBuf open;      // verified read, composed route: digests, plaintext
  RagBufs orag;        // ragged open (CVs of 64 B)
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

// The one launch-and-log site of k_pass and k_quad: r's instantiation over a,
// with split-mode scratch when r splits.
hipError_t launch_rec(const LaunchRec &r, KArgs a, hipStream_t s) {
  if (!launchable(r)) return hipErrorInvalidValue;
  a.split_log2 = r.split_log2;
  a.scratch = nullptr;
  a.cnt = nullptr;
  if (r.split_log2) {
    hipError_t e = scratch_get(&a, r.grid, a.n, s);
    if (e != hipSuccess) return e;
  }
  hipError_t e = hipErrorInvalidValue;
  if (r.family == kLaunchQuad)
    e = with_g<kQuadQpws>(r.g, [&](auto Q) {
      hipLaunchKernelGGL(k_quad<Q()>, dim3(r.grid), dim3(Q() == 64 ? 256 : 1024), 0, s, a);
      return hipSuccess;
    });
  else if (r.family == kLaunchPass)
    e = with_g<kPassGs>(r.g, [&](auto G) {
      const bool ok = try_pass_g<G(), false>(r, a, s) || try_pass_g<G(), true>(r, a, s);
      return ok ? hipSuccess : hipErrorInvalidValue;
    });
  if (e != hipSuccess) return e;
  if (g_launch_log.on()) g_launch_log.append(r);
  return hipGetLastError();
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

// One pass over the small blobs, as small_plan says: k_small, or k_small_q
// with its counters and at most the resident workgroups.
template <bool CHACHA>
hipError_t launch_small_pass(SArgs a, uint64_t max_len, hipStream_t s) {
  const SmallPlan p = small_plan(a.n, max_len, CHACHA, knobs().latency_wgs);
  a.n_coarse = p.n_coarse;
  return with_g<kSmallGs>(uint32_t(p.g), [&](auto G) {
    if (!p.queue) {
      hipLaunchKernelGGL((k_small<G(), CHACHA, 0>), dim3(uint32_t(p.wgs)), dim3(256), 0, s, a);
      if (g_aux_log.on()) g_aux_log.append(small_rec(p, CHACHA, uint32_t(p.wgs), a.n));
      return hipGetLastError();
    }
    constexpr int A = CHACHA ? 1 : 2;  // small_plan's form
    static const uint32_t slots = resident_wgs(k_small_q<G(), CHACHA, A>);
    uint32_t *ctr, epoch;
    hipError_t e = small_q_get(s, &ctr, &epoch);
    if (e != hipSuccess) return e;
    const uint32_t grid = capped_grid(p.wgs, slots);
    hipLaunchKernelGGL((k_small_q<G(), CHACHA, A>), dim3(grid), dim3(256), 0, s, a, ctr, epoch);
    if (g_aux_log.on()) g_aux_log.append(small_rec(p, CHACHA, grid, a.n));
    return hipGetLastError();
  });
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

// The arguments of a pass over job under `key`, digests at out_off of each slot.
KArgs pass_args(const PostJob &job, const uint32_t key[8], uint32_t base, uint32_t out_off) {
  KArgs a{};
  a.clk = clk_words();
  for (int i = 0; i < 8; ++i) a.key[i] = key[i];
  a.base = base;
  a.out_off = out_off;
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

uint32_t low_bits(const void *p) { return uint32_t(reinterpret_cast<uintptr_t>(p)) & 15u; }

PostShape shape_of(const PostJob &job, bool fuse = false) {
  return {job.n,  job.msg_len, job.last_len, job.stride, low_bits(job.src), low_bits(job.ctext),
          low_bits(job.out.refs), job.ctext != nullptr, job.out.bf, job.out.stride, fuse};
}

KArgs dek_args(const PostJob &job, uint32_t out_off) {
  return pass_args(job, job.salt, kKeyed, out_off);
}
KArgs cid_args(const PostJob &job) {
  return pass_args(job, job.cid_key, job.cid_keyed ? kKeyed : 0u, 0);
}

// launch_decrypt at a latency bound already read.
hipError_t decrypt_with(const uint8_t *ctext, uint8_t *ptext, uint64_t n, uint64_t bs,
                        uint64_t last_len, const uint8_t *refs, uint32_t latency_wgs,
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
  const bool aligned = ((low_bits(ctext) | low_bits(ptext)) & 15) == 0;
  const DecryptPlan p = decrypt_plan(n, bs, last_len, aligned, latency_wgs);
  if (p.units) {
    if (p.lines.form == 0)
      hipLaunchKernelGGL(k_decrypt_lines<0>, dim3(p.lines.grid), dim3(256), 0, s, a, p.units,
                         p.upb_shift, p.run_shift);
    else
      hipLaunchKernelGGL(k_decrypt_lines<2>, dim3(p.lines.grid), dim3(256), 0, s, a, p.units,
                         p.upb_shift, p.run_shift);
    if (g_aux_log.on()) g_aux_log.append(lines_rec(p, n));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (!p.grid) return hipSuccess;
  a.stride = p.first_kb;  // first keystream block left for k_decrypt
  hipLaunchKernelGGL(k_decrypt, dim3(p.grid), dim3(256), 0, s, a);
  if (g_aux_log.on()) g_aux_log.append(decrypt_rec(p, aligned, n));
  return hipGetLastError();
}

// The CID side as cid_route says: the one k_pass launch, or the keystream
// launch and a BLAKE3 pass over the ctext.
hipError_t launch_cid(const PostJob &job, const CidRoute &c, uint32_t latency_wgs, hipStream_t s) {
  KArgs a = cid_args(job);
  if (c.keystream) {
    hipError_t e = decrypt_with(job.src, job.ctext, job.n, c.ks_bs, job.last_len, job.out.refs,
                                latency_wgs, s);
    if (e != hipSuccess) return e;
    a.src = job.ctext;
    a.ctext = nullptr;
  }
  return launch_rec(c.pass, a, s);
}

// The one launch-and-log site of k_pass_dc: post_route's fused record r.
hipError_t launch_dc(const LaunchRec &r, const PostJob &job, hipStream_t s) {
  if (r.family != kLaunchPassDc || !launchable(r)) return hipErrorInvalidValue;
  const uint32_t sl = r.split_log2;
  const uint64_t wgs = job.n << sl;
  KArgs a = dek_args(job, 32);
  a.split_log2 = sl;
  // scratch: DEK CVs (wgs), coarse CID CVs (wgs), fine CID CVs (2 wgs)
  hipError_t e = scratch_get(&a, 4 * wgs, 2 * job.n, s);
  if (e != hipSuccess) return e;
  DcState d{};
  e = dc_get(job.n, s, &d);
  if (e != hipSuccess) return e;
  d.n = r.n;
  d.sl = sl;
  d.fine_div = r.fine_div;
  KArgs b = cid_args(job);
  b.split_log2 = sl;
  b.scratch = a.scratch + wgs * 8;
  b.cnt = a.cnt + job.n;
  KArgs c = b;  // fine CID items: twice the workgroups per message
  c.split_log2 = sl + 1;
  c.scratch = b.scratch + wgs * 8;
  e = with_g<kDcGs>(r.g, [&](auto G) {
    hipLaunchKernelGGL(k_pass_dc<G()>, dim3(r.grid), dim3(256), 0, s, a, b, c, d);
    if (g_launch_log.on()) g_launch_log.append(r);
    return hipGetLastError();
  });
  if (e != hipSuccess) {  // the epoch was used without the launch that clears the next bank
    SlotLock g(s, false);
    dc_lists_zero(g.sl, s);
  }
  return e;
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

hipError_t launch_keyed_hash(const PostJob &job, uint32_t out_off, hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  const Knobs k = knobs();
  const PostShape j = shape_of(job);
  return launch_rec(dek_rec(j, plan_of(j, k), out_off, k), dek_args(job, out_off), s);
}

hipError_t launch_post(const PostJob &job, hipStream_t s, bool fused) {
  if (job.n == 0) return hipSuccess;
  const Knobs k = knobs();
  const PostRoute r = post_route(shape_of(job, fused), k);
  if (r.fused) return launch_dc(r.dek, job, s);
  hipError_t e = launch_rec(r.dek, dek_args(job, 32), s);
  if (e != hipSuccess) return e;
  return launch_cid(job, r.cid, k.latency_wgs, s);
}

hipError_t launch_cid_pass(const PostJob &job, hipStream_t s) {
  if (job.n == 0) return hipSuccess;
  const Knobs k = knobs();
  const PostShape j = shape_of(job);
  return launch_cid(job, cid_route(j, plan_of(j, k), k), k.latency_wgs, s);
}

hipError_t launch_fill(uint8_t *dst, uint64_t offset, uint64_t n, uint64_t seed,
                       hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (offset & 7) return hipErrorInvalidValue;
  const uint32_t grid = capped_grid((((n + 7) >> 3) + 255) / 256, 65536);
  hipLaunchKernelGGL(k_fill, dim3(grid), dim3(256), 0, s, dst, offset, n, seed);
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

// The plan of a ragged call over a (src, offs, lens, n, lo, hi set) in the
// post's or the open's buffers: count, prefix, the totals (chunks, merge
// groups, messages of more than 256 chunks), CV scratch of cv_words words per
// chunk and group.  MARK: a message not selected gets status `mark` in unsel.
template <bool MARK>
static hipError_t rag_plan(RArgs &a, RagBufs ScratchSlot::*set, uint32_t cv_words, uint32_t *unsel,
                           uint32_t mark, uint64_t totals[3], hipStream_t s) {
  a.m = (a.n + kRagWG - 1) / kRagWG;
  uint64_t *tot = nullptr, *d_tot = nullptr;
  // `plan` / `cv` bytes (0: leave that one alone) and the pinned totals
  auto get = [&](size_t plan, size_t cv) {
    SlotLock g(s);
    if (g.sd.e != hipSuccess) return g.sd.e;
    RagBufs &b = g.sl->*set;
    hipError_t e = b.tot.ensure();
    if (e == hipSuccess) e = b.plan.ensure(s, plan, kGrowFloor, 4, false);
    if (e == hipSuccess) e = b.cv.ensure(s, cv, kGrowFloor, 4, false);
    a.pre = b.plan.as<uint64_t>();
    a.wpre = a.pre + a.n;
    if (cv) a.cvs = b.cv.as<uint32_t>();
    tot = static_cast<uint64_t *>(b.tot.h);
    d_tot = static_cast<uint64_t *>(b.tot.d);
    return e;
  };
  hipError_t e = get(8 * (a.n + 3 * (a.m + 1)), 0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rag_count<MARK>, dim3(uint32_t(a.m)), dim3(kRagWG), 0, s, a, unsel, mark);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rag_prefix<1024>, dim3(3), dim3(1024), 0, s, a.wpre, a.m, d_tot);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the one host wait of the call: the totals size the CV scratch and the
  // launches that follow
  e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  for (int i = 0; i < 3; ++i) totals[i] = __atomic_load_n(tot + i, __ATOMIC_RELAXED);
  if (totals[0] == 0) return hipSuccess;  // nothing selected
  e = get(0, 4 * size_t(cv_words) * (totals[0] + totals[1]));
  a.gcv = a.cvs + cv_words * totals[0];
  return e;
}

// The kernel of one level of a ragged pass, r.  Defined behind their callers,
// launch_post_ragged and launch_open_ragged: the compiler emits kernels in the
// order it meets them, and the code object keeps the order it had.
static hipError_t rag_level(const LaunchRec &r, const RArgs &a, hipStream_t s);
static hipError_t rag_level(const LaunchRec &r, const ROArgs &a, hipStream_t s);
static RArgs &rag_args(RArgs &a) { return a; }
static RArgs &rag_args(ROArgs &a) { return a.r; }

// The one launch-and-log site of the ragged levels: the records of one pass
// (rag_pass_recs over the plan's totals `tot`), in order.
template <class Args>
static hipError_t launch_rag_levels(const RagPlan &p, const uint64_t tot[3], Args a, hipStream_t s) {
  for (uint32_t i = 0; i < p.n; ++i) {
    const LaunchRec &r = p.rec[i];
    if (!launchable(r)) return hipErrorInvalidValue;
    rag_args(a).total = tot[r.family - kLaunchRagChunk];
    hipError_t e = rag_level(r, a, s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (g_aux_log.on()) g_aux_log.append(r);
  }
  return hipSuccess;
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
  uint64_t totals[3];
  hipError_t e = rag_plan<false>(a, &ScratchSlot::rag, 8, nullptr, 0u, totals, s);
  if (e != hipSuccess || totals[0] == 0) return e;
  for (int i = 0; i < 8; ++i) a.key[i] = job.salt[i];
  a.base = kKeyed;
  a.out_off = 32;
  e = launch_rag_levels(rag_pass_recs(totals, kRagPostDek, knobs().latency_wgs), totals, a, s);
  if (e != hipSuccess) return e;
  for (int i = 0; i < 8; ++i) a.key[i] = job.cid_key[i];
  a.base = job.cid_keyed ? kKeyed : 0u;
  a.out_off = 0;
  return launch_rag_levels(rag_pass_recs(totals, kRagPostCid, knobs().latency_wgs), totals, a, s);
}

static hipError_t rag_level(const LaunchRec &r, const RArgs &a, hipStream_t s) {
  const dim3 grid(r.grid), block(256);
  return with_g<kRagPostKinds>(r.g, [&](auto K) {
    if (r.family == kLaunchRagChunk)
      return with_g<kRagForms>(r.form, [&](auto A) {
        hipLaunchKernelGGL((k_rag_chunk<K() == kRagPostCid, A()>), grid, block, 0, s, a);
        return hipSuccess;
      });
    if (r.family == kLaunchRagMergeA) hipLaunchKernelGGL(k_rag_merge_a, grid, block, 0, s, a);
    if (r.family == kLaunchRagMergeB) hipLaunchKernelGGL(k_rag_merge_b, grid, block, 0, s, a);
    return hipSuccess;
  });
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

size_t aux_log(int reset, uint32_t *out, size_t cap) {
  if (!g_aux_log.on()) g_aux_log.enable();
  return g_aux_log.read(reset != 0, out, cap);
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

// ---- The one-shot classes (one_kernels.h, one_open_kernels.h) ----

// ka over the array at d, or -- r goes by value -- kv over the one descriptor
// at h.
template <class KA, class KV, class D, class... X>
static hipError_t one_go(const LaunchRec &r, KA ka, KV kv, const D *h, const D *d, hipStream_t s,
                         X... x) {
  if (r.fine_div)
    hipLaunchKernelGGL(kv, dim3(r.grid), dim3(one_block(r)), 0, s, *h, x...);
  else
    hipLaunchKernelGGL(ka, dim3(r.grid), dim3(one_block(r)), 0, s, d, x...);
  return hipGetLastError();
}
// The kernels of a launchable r, [QUADS == 64]: kOneQuads.
static hipError_t one_kernels(const LaunchRec &r, const OneDesc *h, const OneDesc *d,
                              hipStream_t s) {
  if (r.family == kLaunchOne) {
    void (*const ka[])(const OneDesc *) = {k_one<16>, k_one<64>};
    void (*const kv[])(const OneDesc) = {k_one_v<16>, k_one_v<64>};
    return one_go(r, ka[r.g == 64], kv[r.g == 64], h, d, s);
  }
  if (r.family != kLaunchMed) return hipErrorInvalidValue;
  const uint32_t wmax = r.grid / r.n;  // workgroups per message, one per 64 KiB
  const hipError_t e = one_go(r, k_med_dek, k_med_dek_v, h, d, s, wmax);
  return e != hipSuccess ? e : one_go(r, k_med_cid, k_med_cid_v, h, d, s, wmax);
}
static hipError_t one_kernels(const LaunchRec &r, const OneOpenDesc *h, const OneOpenDesc *d,
                              hipStream_t s) {
  if (r.family != kLaunchOneOpen) return hipErrorInvalidValue;
  void (*const ka[2][2])(const OneOpenDesc *) = {{k_one_open<16, true>, k_one_open<64, true>},
                                                 {k_one_open<16, false>, k_one_open<64, false>}};
  void (*const kv[2][2])(const OneOpenDesc) = {{k_one_open_v<16, true>, k_one_open_v<64, true>},
                                               {k_one_open_v<16, false>, k_one_open_v<64, false>}};
  return one_go(r, ka[!r.chacha][r.g == 64], kv[!r.chacha][r.g == 64], h, d, s);
}

// The one launch-and-log site of the one-shot classes: one_rec's record.
template <class D>
static hipError_t launch_one_rec(OneClass c, const D *h, const D *d, uint32_t n, uint64_t max_len,
                                 hipStream_t s) {
  LaunchRec r;
  if (!one_rec(c, n, max_len, &r)) return hipErrorInvalidValue;
  if (!r.grid) return hipSuccess;
  if (!launchable(r)) return hipErrorInvalidValue;
  const hipError_t e = one_kernels(r, h, d, s);
  if (e == hipSuccess && g_aux_log.on()) g_aux_log.append(r);
  return e;
}
hipError_t launch_one_class(OneClass c, const OneDesc *h, const OneDesc *d, uint32_t n,
                            uint64_t max_len, hipStream_t s) {
  return launch_one_rec(c, h, d, n, max_len, s);
}
hipError_t launch_one_class(OneClass c, const OneOpenDesc *h, const OneOpenDesc *d, uint32_t n,
                            uint64_t max_len, hipStream_t s) {
  return launch_one_rec(c, h, d, n, max_len, s);
}

hipError_t launch_decrypt(const uint8_t *ctext, uint8_t *ptext, uint64_t n, uint64_t bs,
                          uint64_t last_len, const uint8_t *refs, hipStream_t s) {
  return decrypt_with(ctext, ptext, n, bs, last_len, refs, knobs().latency_wgs, s);
}

hipError_t launch_chacha_xor(const uint32_t k[8], const uint8_t *src,
                             uint8_t *dst, uint64_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  KArgs a{};
  a.src = src;
  a.ctext = dst;
  a.msg_len = n;
  for (int i = 0; i < 8; ++i) a.key[i] = k[i];
  const uint32_t grid = capped_grid((((n + 63) >> 6) + 255) / 256, 65536);
  hipLaunchKernelGGL(k_chacha_xor, dim3(grid), dim3(256), 0, s, a);
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

// The composed route's scratch on stream s: `bytes`.
static hipError_t open_get(hipStream_t s, size_t bytes, uint8_t **p) {
  SlotLock g(s);
  if (g.sd.e != hipSuccess) return g.sd.e;
  hipError_t e = g.sl->open.ensure(s, bytes, kGrowFloor, 4, false);
  *p = g.sl->open.as<uint8_t>();
  return e;
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
  PostJob pj{};
  pj.src = job.ctext;
  pj.stride = pj.msg_len = job.bs;
  pj.last_len = job.last_len;
  pj.n = job.n;
  pj.out = RefLayout{scr, ~0ull, 0};
  for (int i = 0; i < 8; ++i) pj.cid_key[i] = job.cid_key[i];
  pj.cid_keyed = job.cid_keyed;
  const Knobs k = knobs();
  PostShape j = shape_of(pj);
  const PassPlan p = plan_of(j, k);
  e = launch_rec(dek_rec(j, p, 0, k), cid_args(pj), s);  // BLAKE3 only, the CID's key
  if (e != hipSuccess) return e;
  if (pt) {
    e = decrypt_with(job.ctext, pt, job.n, job.bs, job.last_len, job.refs, k.latency_wgs, s);
    if (e != hipSuccess) return e;
  }
  if (job.salted) {
    pj.src = pt;
    for (int i = 0; i < 8; ++i) pj.salt[i] = job.salt[i];
    j.src_lo = low_bits(pt);
    e = launch_rec(dek_rec(j, p, 32, k), dek_args(pj, 32), s);
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
  const bool aligned = ((low_bits(job.ctext) | low_bits(job.ptext) | job.bs) & 15) == 0;
  LaunchRec r;
  if (!open_rec(job.n, job.bs, job.salted, aligned, g_open_route.load(std::memory_order_relaxed),
                &r))
    return launch_open_composed(job, s);
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
  // the one launch-and-log site of k_open
  if (!launchable(r)) return hipErrorInvalidValue;
  return with_g<kOpenGs>(r.g, [&](auto G) {
    if (r.aligned)
      hipLaunchKernelGGL((k_open<G(), true, 2>), dim3(r.grid), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((k_open<G(), false, 2>), dim3(r.grid), dim3(256), 0, s, a);
    if (g_launch_log.on()) g_launch_log.append(r);
    return hipGetLastError();
  });
}

// ---- The ragged open (ragged_open_kernels.h) ----

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
  a.status = job.status;
  // a message above max_len is neither read nor written: it fails closed
  uint64_t totals[3];
  hipError_t e = rag_plan<true>(a.r, &ScratchSlot::orag, 16, job.status, 1u /* GLFSX_BAD_CID */,
                                totals, s);
  if (e != hipSuccess || totals[0] == 0) return e;
  for (int i = 0; i < 8; ++i) {
    a.r.key[i] = job.cid_key[i];
    a.salt[i] = job.salt[i];
  }
  a.r.base = job.cid_keyed ? kKeyed : 0u;
  const RagKind kind = job.salted ? kRagOpen2 : job.ptext ? kRagOpen1 : kRagOpen0;
  return launch_rag_levels(rag_pass_recs(totals, kind, knobs().latency_wgs), totals, a, s);
}

static hipError_t rag_level(const LaunchRec &r, const ROArgs &a, hipStream_t s) {
  const dim3 grid(r.grid), block(256);
  return with_g<kRagOpenKinds>(r.g, [&](auto K) {
    constexpr int MODE = K() - kRagOpen0;
    if (r.family == kLaunchRagChunk)
      return with_g<kRagForms>(r.form, [&](auto A) {
        hipLaunchKernelGGL((k_rag_open_chunk<MODE, A()>), grid, block, 0, s, a);
        return hipSuccess;
      });
    if (r.family == kLaunchRagMergeA)
      hipLaunchKernelGGL(k_rag_open_merge_a<MODE == 2>, grid, block, 0, s, a);
    if (r.family == kLaunchRagMergeB)
      hipLaunchKernelGGL(k_rag_open_merge_b<MODE == 2>, grid, block, 0, s, a);
    return hipSuccess;
  });
}

}  // namespace glfsx
