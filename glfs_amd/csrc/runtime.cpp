// runtime.cpp -- the definitions behind host.h (error text, per-thread
// contexts, stream waits, salts) and the small entry points of the C ABI.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <sched.h>

#include "host.h"

namespace glfsx {
namespace host {

static thread_local std::string tls_err;

const std::string &last_error_text() { return tls_err; }

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  tls_err = buf;
  return code;
}

// One context per device the thread has used (a thread may switch devices,
// e.g. one driving several GPUs; switching back finds its stream and
// buffers again instead of leaking them).  Contexts live as long as the
// thread (see ~Ctx).
static thread_local std::vector<Ctx *> tls_ctxs;
static thread_local int tls_dev = 0;

void set_thread_device(int dev) { tls_dev = dev; }

int ctx_get(Ctx **out) {
  if (tls_dev >= 0 && size_t(tls_dev) < tls_ctxs.size() && tls_ctxs[tls_dev]) {
    Ctx &c = *tls_ctxs[tls_dev];
    HIP_TRY(hipSetDevice(c.dev));
    *out = &c;
    return 0;
  }
  {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
      return fail(GLFSX_E_DEVICE,
                  "no HIP device available (%s); the glfsx path has no CPU "
                  "fallback",
                  e != hipSuccess ? hipGetErrorString(e) : "count = 0");
    if (tls_dev >= n)
      return fail(GLFSX_E_DEVICE, "device %d out of range (%d devices)",
                  tls_dev, n);
    HIP_TRY(hipSetDevice(tls_dev));
    auto *c = new Ctx();  // lives as long as the thread's use of the device
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return fail(GLFSX_E_DEVICE, "hipStreamCreate on device %d failed", tls_dev);
    }
    c->dev = tls_dev;
    if (tls_ctxs.size() <= size_t(tls_dev)) tls_ctxs.resize(tls_dev + 1, nullptr);
    tls_ctxs[tls_dev] = c;
    *out = c;
    return 0;
  }
}

// Wait for a stream whose results the caller is about to return.  Polls
// for up to kSpinNs first: a blocking hipStreamSynchronize wakes the thread
// tens to hundreds of microseconds after the GPU finishes, which is most of
// the host overhead of a short call (a 1 GiB Create takes ~1.3 ms, config
// 4's one call ~5 ms: at a 2 ms bound it waited its last ~3 ms blocked and
// lost ~0.1 ms to the wake-up); longer waits block.  At most kMaxSpinners
// threads poll at once (glfs.Machine is used concurrently; N pollers would
// pin N host cores); the rest block at once, and a poller yields its core
// between queries.  GLFSX_SPIN_US overrides the poll bound (default 20 ms).
static const int64_t kSpinNs = [] {
  const char *e = getenv("GLFSX_SPIN_US");
  return e ? int64_t(strtoll(e, nullptr, 10)) * 1000 : int64_t(20000000);
}();
constexpr int kMaxSpinners = 4;
static std::atomic<int> g_spinners{0};
hipError_t stream_wait(hipStream_t s) {
  if (g_spinners.fetch_add(1, std::memory_order_relaxed) >= kMaxSpinners) {
    g_spinners.fetch_sub(1, std::memory_order_relaxed);
    return hipStreamSynchronize(s);
  }
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e;
  for (;;) {
    e = hipStreamQuery(s);
    if (e != hipErrorNotReady) break;
    if (std::chrono::duration_cast<std::chrono::nanoseconds>(
            std::chrono::steady_clock::now() - t0).count() > kSpinNs) {
      e = hipStreamSynchronize(s);
      break;
    }
    sched_yield();
  }
  g_spinners.fetch_sub(1, std::memory_order_relaxed);
  return e;
}

static thread_local bool tls_fused = true;
static thread_local bool tls_fused_failed = false;

bool fused_posts() { return tls_fused; }

int fused_retry(int (*f)(void *), void *arg) {
  tls_fused_failed = false;
  int rc = f(arg);
  if (rc && tls_fused_failed) {
    tls_fused_failed = false;
    tls_fused = false;
    rc = f(arg);
    tls_fused = true;
  }
  return rc;
}

int fused_check(hipStream_t s) {
  if (const uint32_t v = fused_errors_take(s)) {
    tls_fused_failed = true;
    return fail(GLFSX_E_DEVICE,
                "one-launch split post on stream %p: %s; its results were discarded",
                static_cast<void *>(s),
                v == 1 ? "a DEK wait timed out" : "a workgroup found no work item");
  }
  return 0;
}

namespace {
// DeriveKey on the GPU (ref.go:152-161): keyed BLAKE3 of `in`, 32 bytes.
int derive_key_dev(Ctx *c, uint8_t out[32], const uint8_t salt[32],
                   const void *in, size_t n) {
  if (n > kMaxMsgLen)
    return fail(GLFSX_E_UNSUPPORTED, "derive_key input of %zu bytes exceeds %llu",
                n, (unsigned long long)kMaxMsgLen);
  if (int e = c->d_small.ensure(64 + n + 64)) return e;
  if (int e = c->h_small.ensure(64)) return e;
  uint8_t *d_out = c->d_small.u8();
  uint8_t *d_in = c->d_small.u8() + 64;
  if (n) HIP_TRY(hipMemcpyAsync(d_in, in, n, hipMemcpyHostToDevice, c->stream));
  PostJob j = single_job(d_in, n, nullptr, d_out);
  set_keys(j, salt, nullptr);
  HIP_TRY(launch_keyed_hash(j, 0, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_small.p, d_out, 32, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(stream_wait(c->stream));
  memcpy(out, c->h_small.p, 32);
  return 0;
}

// DeriveKey's full contract (ref.go:152-161): any input length, any output
// length -- the streaming one-workgroup hasher of xof_kernels.hip, input in
// slabs of 256 MiB through device staging.
int derive_key_xof(Ctx *c, uint8_t *out, size_t out_len, const uint8_t salt[32],
                   const void *in, size_t n) {
  constexpr uint64_t kGroup = 256ull << 10, kSlabGroups = 1024;
  if (int e = c->d_small.ensure(sizeof(B3State) + out_len + 64)) return e;
  if (int e = c->d_in.ensure(std::min<uint64_t>(n, kSlabGroups * kGroup) + 64)) return e;
  B3State h{};
  words_from_key(h.key, salt);
  h.base = 16;  // KEYED_HASH (BLAKE3 spec 2.1)
  auto *st = reinterpret_cast<B3State *>(c->d_small.p);
  uint8_t *d_out = c->d_small.u8() + ((sizeof(B3State) + 63) & ~size_t(63));
  HIP_TRY(hipMemcpyAsync(st, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
  const uint8_t *p = static_cast<const uint8_t *>(in);
  // every whole group that does not hold the last byte
  const uint64_t groups = n ? (n - 1) / kGroup : 0;
  for (uint64_t g0 = 0; g0 < groups; g0 += kSlabGroups) {
    const uint64_t k = std::min(kSlabGroups, groups - g0);
    HIP_TRY(hipMemcpyAsync(c->d_in.p, p + g0 * kGroup, k * kGroup, hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(launch_b3_absorb(st, c->d_in.u8(), k, c->stream));
  }
  const uint64_t rem = n - groups * kGroup;
  if (rem)
    HIP_TRY(hipMemcpyAsync(c->d_in.p, p + groups * kGroup, rem, hipMemcpyHostToDevice,
                           c->stream));
  HIP_TRY(launch_b3_final(st, c->d_in.u8(), rem, d_out, out_len, c->stream));
  std::vector<uint8_t> tmp(out_len);
  HIP_TRY(hipMemcpyAsync(tmp.data(), d_out, out_len, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(stream_wait(c->stream));
  memcpy(out, tmp.data(), out_len);
  return 0;
}
}  // namespace

int check_batch_block_size(uint64_t bs) {
  if (bs == 0 || bs > kMaxMsgLen)
    return fail(GLFSX_E_UNSUPPORTED, "block size %llu unsupported", (unsigned long long)bs);
  return 0;
}

int check_block_size(uint64_t bs) {
  if (bs < GLFSX_MIN_BLOCK_SIZE)
    return fail(GLFSX_E_BLOCKSIZE_LT_MIN, "blockSize cannot be < %d",
                GLFSX_MIN_BLOCK_SIZE);
  if (bs > kMaxMsgLen)
    return fail(GLFSX_E_UNSUPPORTED,
                "block size %llu above the kernels' limit %llu",
                (unsigned long long)bs, (unsigned long long)kMaxMsgLen);
  return 0;
}

// blob.go:99-101.  DeriveKey is a pure function, so the (salt -> indexSalt,
// rawSalt) pairs are memoised (process-wide): NewWriter is called once per
// blob by glfs.PostBlob (machine.go:64) and would otherwise cost two launches
// each.
namespace {
struct SaltCacheEntry {
  uint8_t salt[32];
  Salts s;
};
std::mutex g_salts_mu;
std::vector<SaltCacheEntry> g_salts;
}  // namespace

int derive_salts(Ctx *c, const uint8_t *salt, Salts *s) {
  static const uint8_t zero[32] = {0};
  const uint8_t *sl = salt ? salt : zero;
  // the calling thread's last salt first: concurrent PostBlob callers (one
  // salt per type) never touch the process-wide lock
  thread_local SaltCacheEntry last{};
  thread_local bool have_last = false;
  if (have_last && memcmp(last.salt, sl, 32) == 0) {
    *s = last.s;
    return 0;
  }
  {
    std::lock_guard<std::mutex> lk(g_salts_mu);
    for (const auto &e : g_salts)
      if (memcmp(e.salt, sl, 32) == 0) {
        *s = e.s;
        last = e;
        have_last = true;
        return 0;
      }
  }
  if (int e = derive_key_dev(c, s->index, sl, "index", 5)) return e;
  if (int e = derive_key_dev(c, s->raw, sl, "raw", 3)) return e;
  SaltCacheEntry ent;
  memcpy(ent.salt, sl, 32);
  ent.s = *s;
  last = ent;
  have_last = true;
  std::lock_guard<std::mutex> lk(g_salts_mu);
  if (g_salts.size() >= 64) g_salts.erase(g_salts.begin());
  g_salts.push_back(ent);
  return 0;
}

}  // namespace host
}  // namespace glfsx

using namespace glfsx;
using namespace glfsx::host;

extern "C" {

const char *glfsx_last_error(void) { return tls_err.c_str(); }

const char *glfsx_version(void) { return "glfsx 0.1 gfx950"; }

uint32_t glfsx_set_split_target(uint32_t wgs) { return set_split_target(wgs); }
uint32_t glfsx_set_latency_wgs(uint32_t wgs) { return set_latency_wgs(wgs); }

uint64_t glfsx_debug_fused(uint32_t skip_msg, uint64_t wait_us) {
  fused_debug(skip_msg, wait_us);
  return fused_timeouts();
}

uint64_t glfsx_fused_failures(void) { return fused_timeouts(); }

int glfsx_clock_probe(int reset, uint64_t out[2]) {
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  HIP_TRY(clock_probe(reset, out));
  return 0;
}

int glfsx_debug_pass_log(int reset, uint32_t *out, size_t cap, size_t *n) {
  if (cap && !out) return fail(GLFSX_E_ARG, "null log buffer");
  const size_t total = pass_log(reset, out, cap);
  if (n) *n = total;
  return 0;
}

int glfsx_debug_aux_log(int reset, uint32_t *out, size_t cap, size_t *n) {
  if (cap && !out) return fail(GLFSX_E_ARG, "null log buffer");
  const size_t total = aux_log(reset, out, cap);
  if (n) *n = total;
  return 0;
}

#if GLFSX_WGTIME
// diagnostic builds only (tools/build_variant.sh): the bulk passes' phase
// timestamps, 8192 x 16 words
int glfsx_debug_wgtime(uint64_t *out) {
  HIP_TRY(debug_wgtime(out));
  return 0;
}
#endif

int glfsx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int glfsx_set_device(int dev) {
  if (dev < 0) return fail(GLFSX_E_ARG, "negative device");
  tls_dev = dev;
  Ctx *c;
  return ctx_get(&c);
}

int glfsx_derive_key(uint8_t *out, size_t out_len, const uint8_t salt[32],
                     const void *input, size_t n) {
  if ((out_len && !out) || !salt || (n && !input)) return fail(GLFSX_E_ARG, "null argument");
  if (out_len == 0) return 0;
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  if (out_len > 32 || n > kMaxMsgLen)
    return derive_key_xof(c, static_cast<uint8_t *>(out), out_len, salt, input, n);
  uint8_t full[32];
  if (int e = derive_key_dev(c, full, salt, input, n)) return e;
  memcpy(out, full, out_len);
  return 0;
}

int glfsx_chacha20_xor(const uint8_t dek[32], const void *src, void *dst,
                       uint64_t n) {
  if (!dek || (n && (!src || !dst))) return fail(GLFSX_E_ARG, "null argument");
  if (n == 0) return 0;
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  if (int e = c->d_in.ensure(n)) return e;
  if (int e = c->d_ct.ensure(n)) return e;
  HIP_TRY(hipMemcpyAsync(c->d_in.p, src, n, hipMemcpyHostToDevice, c->stream));
  uint32_t k[8];
  words_from_key(k, dek);
  HIP_TRY(launch_chacha_xor(k, c->d_in.u8(), c->d_ct.u8(), n, c->stream));
  HIP_TRY(hipMemcpyAsync(dst, c->d_ct.p, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(stream_wait(c->stream));
  return 0;
}

int glfsx_fill_splitmix_device(void *d_dst, uint64_t offset, uint64_t n,
                               uint64_t seed, void *stream) {
  if (n && !d_dst) return fail(GLFSX_E_ARG, "null argument");
  if (offset & 7) return fail(GLFSX_E_ARG, "offset must be a multiple of 8");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  HIP_TRY(launch_fill(static_cast<uint8_t *>(d_dst), offset, n, seed,
                      pick_stream(c, stream)));
  return 0;
}

int glfsx_fill_splitmix_blobs_device(void *d_dst, uint64_t n, uint64_t len,
                                     uint64_t seed0, void *stream) {
  if (n && len && !d_dst) return fail(GLFSX_E_ARG, "null argument");
  if (len % 8 || (reinterpret_cast<uintptr_t>(d_dst) & 7))
    return fail(GLFSX_E_ARG, "blob length and pointer must be multiples of 8");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  HIP_TRY(launch_fill_blobs(static_cast<uint8_t *>(d_dst), n, len, seed0,
                            pick_stream(c, stream)));
  return 0;
}

// A store sink that only counts (benchmarks, tests): ctx -> uint64_t[2] =
// {posts, bytes}.  Stands in for a native store's Post at ~zero cost.
int glfsx_sink_count(void *ctx, int kind, const uint8_t *ref, const void *ctext,
                     uint64_t len) {
  (void)kind;
  (void)ref;
  (void)ctext;
  uint64_t *c = static_cast<uint64_t *>(ctx);
  if (c) {
    c[0] += 1;
    c[1] += len;
  }
  return 0;
}

// blob.go:219-268 (pure integer shape math, no hashing)
static uint64_t log2_ceil(uint64_t x) {
  int l = 64 - __builtin_clzll(x);
  if (__builtin_popcountll(x) > 1) l++;
  return uint64_t(l) - 1;
}
static uint64_t div_ceil(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

uint64_t glfsx_branching_factor(uint64_t block_size) { return block_size / 64; }

int glfsx_depth(uint64_t size, uint64_t block_size) {
  if (size == 0) return 0;
  const uint64_t blocks = div_ceil(size, block_size);
  const uint64_t bf = glfsx_branching_factor(block_size);
  return int(div_ceil(log2_ceil(blocks), log2_ceil(bf)));
}

}  // extern "C"
