// The launch layer's per-stream scratch (glfs_amd/csrc/stream_scratch.h),
// launch plans (launch_plan.h) and launch log (launch_log.h), stand-alone.
// Built by tests/test_host_units.py with the host compiler under
// -fsanitize=address,undefined.  No HIP library
// is linked: the few runtime entry points the header calls are fakes over
// malloc, defined here, that log their calls and fail on request.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "launch_log.h"
#include "launch_plan.h"
#include "stream_scratch.h"

using namespace glfsx;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

// ---- the fake runtime ----
struct Fake {
  std::string log;  // one letter per call: M malloc, F free, H host malloc,
                    // h host free, P device pointer, Z memset, S synchronize
  std::map<char, int> fail;  // fail the k-th call from now of that letter
  std::set<void *> dev, pin;  // live allocations
  int mallocs = 0, frees = 0, host_mallocs = 0, host_frees = 0;
  size_t last_malloc = 0, last_memset = 0;
  void *last_memset_p = nullptr;
  hipStream_t last_memset_stream = nullptr, last_sync_stream = nullptr;
  unsigned last_host_flags = 0;
  int cur = 0;
  std::map<hipStream_t, int> stream_dev;
  std::string set_device_log;
  bool call(char c) {  // false: this call is to fail
    log += c;
    auto it = fail.find(c);
    return it == fail.end() || --it->second != 0 || (fail.erase(it), false);
  }
};
static Fake F;
static hipStream_t stream(uintptr_t i) { return reinterpret_cast<hipStream_t>(i << 4); }

extern "C" {
hipError_t hipMalloc(void **p, size_t n) {
  if (!F.call('M')) return hipErrorOutOfMemory;
  *p = malloc(n);
  F.dev.insert(*p);
  ++F.mallocs;
  F.last_malloc = n;
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  F.call('F');
  CHECK(F.dev.erase(p) == 1);  // live, and freed once
  free(p);
  ++F.frees;
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned int flags) {
  if (!F.call('H')) return hipErrorOutOfMemory;
  *p = malloc(n);
  memset(*p, 0xa5, n);
  F.pin.insert(*p);
  ++F.host_mallocs;
  F.last_host_flags = flags;
  return hipSuccess;
}
hipError_t hipHostFree(void *p) {
  F.call('h');
  CHECK(F.pin.erase(p) == 1);
  free(p);
  ++F.host_frees;
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned int) {
  if (!F.call('P')) return hipErrorInvalidValue;
  CHECK(F.pin.count(h) == 1);
  *d = h;
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t s) {
  if (!F.call('Z')) return hipErrorInvalidValue;
  CHECK(F.dev.count(p) == 1);
  memset(p, v, n);  // out of bounds: the sanitizer reports it
  F.last_memset = n;
  F.last_memset_p = p;
  F.last_memset_stream = s;
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  F.last_sync_stream = s;
  return F.call('S') ? hipSuccess : hipErrorUnknown;
}
hipError_t hipGetDevice(int *d) {
  *d = F.cur;
  return hipSuccess;
}
hipError_t hipSetDevice(int d) {
  F.cur = d;
  F.set_device_log += char('0' + d);
  return hipSuccess;
}
hipError_t hipStreamGetDevice(hipStream_t s, hipDevice_t *d) {
  auto it = F.stream_dev.find(s);
  if (it == F.stream_dev.end()) return hipErrorInvalidHandle;
  *d = it->second;
  return hipSuccess;
}
}

static void test_ensure() {
  F = Fake{};
  const hipStream_t s = stream(1);
  {
    StreamBuf b;
    // first allocation: no drain; the floor; not zeroed
    CHECK(b.ensure(s, 100, 128 << 10, 0, false) == hipSuccess);
    CHECK(F.log == "M" && b.p && b.cap == (128u << 10) && F.last_malloc == b.cap);
    // capacity suffices: no call
    CHECK(b.ensure(s, 128 << 10, 128 << 10, 0, false) == hipSuccess && F.log == "M");
    CHECK(b.ensure(s, 0, 0, 0, true) == hipSuccess && F.log == "M");
    // growth: drain, free, allocate; above the floor the size asked for
    CHECK(b.ensure(s, (128 << 10) + 1, 128 << 10, 0, false) == hipSuccess);
    CHECK(F.log == "MSFM" && F.last_sync_stream == s && b.cap == (128u << 10) + 1);
    // moved: the source is empty, one owner
    StreamBuf c(std::move(b));
    CHECK(!b.p && b.cap == 0 && c.p && c.cap == (128u << 10) + 1);
    b = std::move(c);
    CHECK(!c.p && b.p && F.log == "MSFM");
  }
  CHECK(F.log == "MSFMF" && F.dev.empty());
  {
    // zeroed buffers: the memset covers the whole new allocation, on s
    F = Fake{};
    StreamBuf cnt;
    CHECK(cnt.ensure(s, 10 * 4, 4096 * 4, 0, true) == hipSuccess);
    CHECK(F.log == "MZ" && cnt.cap == 4096 * 4 && F.last_memset == cnt.cap);
    CHECK(F.last_memset_p == cnt.p && F.last_memset_stream == s);
    CHECK(cnt.ensure(s, 5000 * 4, 4096 * 4, 0, true) == hipSuccess);
    CHECK(F.log == "MZSFMZ" && cnt.cap == 5000 * 4 && F.last_memset == 5000 * 4);
    // "zeroed once": the floor is the size, the second call does nothing
    StreamBuf q;
    CHECK(q.ensure(s, 64 * 4, 64 * 4, 0, true) == hipSuccess && q.cap == 256);
    const std::string l = F.log;
    CHECK(q.ensure(s, 64 * 4, 64 * 4, 0, true) == hipSuccess && F.log == l);
    // a quarter of headroom, 1 MiB floor
    StreamBuf r;
    CHECK(r.ensure(s, 1000, 1 << 20, 4, false) == hipSuccess && r.cap == (1u << 20));
    CHECK(r.ensure(s, 4 << 20, 1 << 20, 4, false) == hipSuccess && r.cap == (5u << 20));
    CHECK(r.ensure(s, 5 << 20, 1 << 20, 4, false) == hipSuccess && r.cap == (5u << 20));
    // just under the floor with headroom: the floor; just over: the sum
    StreamBuf t;
    CHECK(t.ensure(s, 800 << 10, 1 << 20, 4, false) == hipSuccess && t.cap == (1u << 20));
    StreamBuf u;
    CHECK(u.ensure(s, 900 << 10, 1 << 20, 4, false) == hipSuccess && u.cap == (1125u << 10));
  }
  CHECK(F.dev.empty() && F.mallocs == F.frees);
}

static void test_failures() {
  F = Fake{};
  const hipStream_t s = stream(2);
  {
    StreamBuf b;
    F.fail['M'] = 1;  // the first allocation
    CHECK(b.ensure(s, 100, 4096, 0, true) == hipErrorOutOfMemory && !b.p && b.cap == 0);
    CHECK(b.ensure(s, 100, 4096, 0, true) == hipSuccess && b.p && b.cap == 4096);
    F.fail['Z'] = 1;  // the memset of a grown buffer: nothing is kept
    CHECK(b.ensure(s, 8192, 4096, 0, true) == hipErrorInvalidValue && !b.p && b.cap == 0);
    CHECK(F.dev.empty());
    CHECK(b.ensure(s, 8192, 4096, 0, true) == hipSuccess && b.cap == 8192);
    F.fail['M'] = 1;  // the allocation after the old one was freed
    CHECK(b.ensure(s, 10000, 4096, 0, true) == hipErrorOutOfMemory && !b.p && b.cap == 0);
    CHECK(F.dev.empty());
    CHECK(b.ensure(s, 10000, 4096, 0, true) == hipSuccess && b.cap == 10000);
    F.fail['S'] = 1;  // the drain: the old buffer stays, whole
    void *old = b.p;
    CHECK(b.ensure(s, 20000, 4096, 0, true) == hipErrorUnknown && b.p == old && b.cap == 10000);
    CHECK(b.ensure(s, 20000, 4096, 0, true) == hipSuccess && b.cap == 20000);
  }
  CHECK(F.dev.empty() && F.mallocs == F.frees);
  {
    PinnedBlock e;
    F.fail['H'] = 1;
    CHECK(e.ensure() == hipErrorOutOfMemory && !e.h && !e.d);
    F.fail['P'] = 1;  // the device-pointer lookup: the host block is given back
    CHECK(e.ensure() == hipErrorInvalidValue && !e.h && !e.d && F.pin.empty());
    CHECK(e.ensure() == hipSuccess && e.h && e.d);
    CHECK(F.last_host_flags == hipHostMallocCoherent);
    for (int i = 0; i < 64; ++i) CHECK(static_cast<uint8_t *>(e.h)[i] == 0);
    const std::string l = F.log;
    CHECK(e.ensure() == hipSuccess && F.log == l);  // made once
    PinnedBlock f(std::move(e));
    CHECK(!e.h && !e.d && f.h && f.d);
  }
  CHECK(F.pin.empty() && F.host_mallocs == F.host_frees && F.host_mallocs == 2);
}

struct Slot {
  StreamBuf a, b;
  PinnedBlock pin;
  int tag = 0;
};

static void test_registry() {
  F = Fake{};
  const hipStream_t s = stream(3), s2 = stream(4);
  {
    StreamRegistry<Slot> reg;
    CHECK(reg.find(0, s) == nullptr);
    Slot *x = reg.find_or_make(0, s);
    CHECK(x && reg.find_or_make(0, s) == x && reg.find(0, s) == x && reg.size() == 1);
    // the same handle on another device, another stream on the same device
    Slot *y = reg.find_or_make(1, s);
    Slot *z = reg.find_or_make(0, s2);
    CHECK(y != x && z != x && z != y && reg.size() == 3);
    CHECK(x->a.ensure(s, 100, 4096, 0, true) == hipSuccess && x->pin.ensure() == hipSuccess);
    CHECK(y->a.ensure(s, 100, 4096, 0, true) == hipSuccess && y->pin.ensure() == hipSuccess);
    CHECK(y->b.ensure(s, 9000, 4096, 0, false) == hipSuccess);
    x->tag = 7;
    void *xa = x->a.p, *ya = y->a.p, *yb = y->b.p, *yh = y->pin.h;
    // 100 more slots: the first ones and their buffers stay where they are
    for (uintptr_t i = 0; i < 100; ++i) {
      Slot *n = reg.find_or_make(int(i % 3), stream(100 + i));
      CHECK(n->a.ensure(stream(100 + i), 64, 64, 0, false) == hipSuccess);
    }
    CHECK(reg.size() == 103 && reg.find(0, s) == x && reg.find(1, s) == y);
    CHECK(x->tag == 7 && x->a.p == xa && x->a.cap == 4096 && y->a.p == ya);
    memset(xa, 1, 4096);  // still ours
    // release on device 0 leaves device 1's slot and allocations alone
    const int frees = F.frees, host_frees = F.host_frees;
    reg.release(0, s);
    CHECK(F.frees == frees + 1 && F.host_frees == host_frees + 1 && !F.dev.count(xa));
    CHECK(reg.find(0, s) == nullptr && reg.find(1, s) == y && reg.size() == 102);
    CHECK(y->a.p == ya && y->b.p == yb && y->pin.h == yh);
    CHECK(F.dev.count(ya) && F.dev.count(yb) && F.pin.count(yh));
    memset(yb, 2, 9000);
    reg.release(0, s);  // no such slot: nothing happens
    reg.release(2, s);
    CHECK(reg.size() == 102 && F.frees == frees + 1);
    // a released key makes a fresh, empty slot
    Slot *x2 = reg.find_or_make(0, s);
    CHECK(x2->tag == 0 && !x2->a.p && !x2->pin.h);
    // release everything
    reg.release(0, s);
    reg.release(1, s);
    reg.release(0, s2);
    for (uintptr_t i = 0; i < 100; ++i) reg.release(int(i % 3), stream(100 + i));
    CHECK(reg.size() == 0);
    CHECK(F.dev.empty() && F.pin.empty());
    CHECK(F.mallocs == F.frees && F.mallocs == 103);
    CHECK(F.host_mallocs == F.host_frees && F.host_mallocs == 2);
    // what is left at the registry's end goes with it
    CHECK(reg.find_or_make(0, s)->a.ensure(s, 1, 64, 0, false) == hipSuccess);
  }
  CHECK(F.dev.empty() && F.mallocs == F.frees);
}

static void test_stream_device() {
  F = Fake{};
  const hipStream_t s = stream(5);
  F.stream_dev[s] = 1;
  {
    StreamDevice sd(s);  // a stream of device 1 while device 0 is current
    CHECK(sd.e == hipSuccess && sd.dev == 1 && sd.prev == 0 && F.cur == 1);
  }
  CHECK(F.cur == 0 && F.set_device_log == "10");
  {
    StreamDevice sd(nullptr);  // the null stream: the current device
    CHECK(sd.dev == 0 && F.cur == 0);
  }
  F.cur = 1;
  {
    StreamDevice sd(s);
    CHECK(sd.dev == 1);
  }
  CHECK(F.cur == 1 && F.set_device_log == "10");  // nothing to switch
}

static void test_pass_plan() {
  const uint64_t ns[] = {1, 2, 63, 64, 65, 511, 512, 513, 2048, 65536};
  const uint64_t lens[] = {0, 1, 1 << 10, (1 << 10) + 1, 64 << 10, 1 << 20, 2 << 20,
                           16 << 20, (16 << 20) + 1, 32 << 20, 4ull << 30};
  const uint32_t targets[] = {0, 2048};
  for (uint64_t n : ns)
    for (uint64_t len : lens)
      for (uint32_t target : targets) {
        const PassPlan p = pass_plan(n, len, target, 512);
        const uint64_t C = len ? (len + 1023) >> 10 : 1;
        CHECK(p.g >= 1 && p.g <= 64 && (p.g & (p.g - 1)) == 0);
        CHECK(((256ull * p.g) << p.sl) >= C);  // every chunk has a lane
        if (target == 0)  // no split: the fewest workgroups that cover it
          CHECK(p.sl == 0 || ((256ull * p.g) << (p.sl - 1)) < C);
        if (C <= 256ull * 256 * 64) CHECK(p.sl <= kMaxSplitLog2);
      }
  // spot values at the defaults (split target 2048, latency bound 512)
  struct {
    uint64_t n, len;
    uint32_t target;
    int g;
    uint32_t sl;
  } spots[] = {{65536, 1 << 20, 2048, 4, 0}, {1, 1 << 20, 2048, 1, 2},
               {64, 2 << 20, 2048, 2, 2},    {512, 1 << 20, 2048, 1, 2},
               {1, 32 << 20, 2048, 1, 7},    {1, 1 << 20, 0, 4, 0}};
  for (const auto &c : spots) {
    const PassPlan p = pass_plan(c.n, c.len, c.target, 512);
    CHECK(p.g == c.g && p.sl == c.sl);
  }
  CHECK(quad_qpw(4 << 20) == 64 && quad_qpw((4 << 20) + 1) == 256);
}

// The families outside the log: values worked out by hand from the launch
// code as it stood before the plans moved into launch_plan.h.
static void test_other_plans() {
  CHECK(arx_form(512, 512) == 0 && arx_form(513, 512) == 2 && arx_form(513, 512, 1) == 1);
  {  // the ragged chunk passes: 256 chunks per tile, at most 2^20 workgroups
    GridForm p = rag_chunk_plan(131072, 512);
    CHECK(p.grid == 512 && p.form == 0);
    p = rag_chunk_plan(131073, 512);
    CHECK(p.grid == 513 && p.form == 2);
    p = rag_chunk_plan((1ull << 28) + 1, 512);
    CHECK(p.grid == (1u << 20) && p.form == 2);
    p = rag_chunk_plan(1, 0);
    CHECK(p.grid == 1 && p.form == 2);
  }
  {  // the small pass, either side of 256 * latency_wgs blobs
    SmallPlan p = small_plan(131072, 4096, false, 512);
    CHECK(p.g == 4 && !p.queue && p.form == 0 && p.wgs == 512 && p.n_coarse == 0);
    p = small_plan(131072, 4096, true, 512);
    CHECK(p.g == 4 && !p.queue && p.form == 0 && p.wgs == 512);
    // G = 4: an eighth (16384) held back, 1792 coarse items, 16385 blobs in
    // fine items of 16
    p = small_plan(131073, 4096, false, 512);
    CHECK(p.g == 4 && p.queue && p.form == 2 && p.n_coarse == 1792 && p.items == 2817 &&
          p.wgs == 705);
    p = small_plan(131073, 4096, true, 512);
    CHECK(p.queue && p.form == 1 && p.n_coarse == 1792 && p.items == 2817 && p.wgs == 705);
    // G = 1: nothing held back, the one blob left over is an item of its own
    p = small_plan(131073, 1024, true, 512);
    CHECK(p.g == 1 && p.queue && p.form == 1 && p.n_coarse == 2048 && p.items == 2049 &&
          p.wgs == 513);
    p = small_plan(131073, 1024, false, 131073);
    CHECK(p.g == 1 && !p.queue && p.wgs == 513);
    CHECK(small_plan(1, 0, false, 512).g == 1 && small_plan(1, 1025, false, 512).g == 2);
    CHECK(small_plan(1, 2049, false, 512).g == 4 && small_plan(1, 16384, false, 512).g == 16);
    CHECK(small_plan(1, 16385, false, 512).g == 0 && small_plan(1 << 20, 16385, true, 512).g == 0);
    CHECK(capped_grid(705, 0) == 705 && capped_grid(705, 512) == 512);
    CHECK(capped_grid(300, 512) == 300);
  }
  {  // launch_decrypt
    // blocks of 65 keystream blocks: no 4 KiB units, 132 keystream blocks in all
    DecryptPlan p = decrypt_plan(3, 4160, 100, true, 512);
    CHECK(p.units == 0 && p.first_kb == 0 && p.grid == 1);
    // 64 KiB blocks: 16 units each, a run per unit, nothing left for k_decrypt
    p = decrypt_plan(4, 65536, 65536, true, 512);
    CHECK(p.units == 64 && p.upb_shift == 4 && p.run_shift == 0 && p.lines.grid == 16 &&
          p.lines.form == 0 && p.first_kb == 4096 && p.grid == 0);
    CHECK(decrypt_plan(4, 65536, 65536, true, 16).lines.form == 0);
    CHECK(decrypt_plan(4, 65536, 65536, true, 15).lines.form == 2);
    // ... a short last block: 63 units, then 63 keystream blocks
    p = decrypt_plan(4, 65536, 65536 - 100, true, 512);
    CHECK(p.units == 63 && p.lines.grid == 16 && p.first_kb == 4032 && p.grid == 1);
    // 1 MiB blocks, 2^20 units: runs of 16 leave exactly 65536 runs
    p = decrypt_plan(4096, 1 << 20, 1 << 20, true, 512);
    CHECK(p.units == (1u << 20) && p.upb_shift == 8 && p.run_shift == 4 &&
          p.lines.grid == 16384 && p.lines.form == 2 && p.first_kb == (1u << 26) && p.grid == 0);
    // ... a block fewer: runs of 16 would be 65520, so runs of 8
    p = decrypt_plan(4095, 1 << 20, 1 << 20, true, 512);
    CHECK(p.units == 1048320 && p.run_shift == 3 && p.lines.grid == 16384);
    p = decrypt_plan(4097, 1 << 20, 1 << 20, true, 512);
    CHECK(p.units == 1048832 && p.run_shift == 4 && p.lines.grid == 16384);
    // three units per block: no shift, a run per unit
    p = decrypt_plan(10, 12288, 12288, true, 512);
    CHECK(p.units == 30 && p.upb_shift == 64 && p.run_shift == 0 && p.lines.grid == 8 &&
          p.lines.form == 0 && p.first_kb == 1920 && p.grid == 0);
    // unaligned buffers: k_decrypt alone, at most 65536 workgroups
    p = decrypt_plan(2, 65536, 65536, false, 512);
    CHECK(p.units == 0 && p.lines.grid == 0 && p.first_kb == 0 && p.grid == 8);
    p = decrypt_plan(4096, 1 << 20, 1 << 20, false, 512);
    CHECK(p.units == 0 && p.grid == 65536);
  }
  {  // a whole post at the defaults: the headline, config 2 and a latency-bound Create level
    const Knobs k{2048, 512};
    PostShape j{2048, 1 << 20, 1 << 20, 1 << 20, 0, 0, 0, true, ~0ull, 0, true};
    PostRoute r = post_route(j, k);
    CHECK(!r.fused && !r.cid.keystream && r.dek.family == kLaunchPass && r.dek.g == 4 &&
          r.dek.form == 2 && r.cid.pass.g == 4 && r.cid.pass.chacha == 1 && r.cid.pass.form == 1 &&
          r.cid.pass.grid == 2048);
    j.n = 512;
    j.msg_len = j.last_len = j.stride = 2 << 20;
    r = post_route(j, k);  // 8 chunks per lane halved twice: 2048 workgroups, one launch
    CHECK(r.fused && r.dek.family == kLaunchPassDc && r.dek.g == 2 && r.dek.split_log2 == 2 &&
          r.dek.fine_div == 4 && r.dek.n == 512 && r.dek.grid == r.dek.items);
    j.fuse = false;
    r = post_route(j, k);
    CHECK(!r.fused && r.dek.g == 2 && r.dek.split_log2 == 2 && r.dek.form == 2 &&
          r.cid.pass.form == 2 && r.cid.pass.grid == 2048);
    j.n = 1;  // one 2 MiB node: quad DEK pass, keystream + quad CID pass
    r = post_route(j, k);
    CHECK(!r.fused && r.dek.family == kLaunchQuad && r.dek.g == 64 && r.dek.split_log2 == 5 &&
          r.cid.keystream && r.cid.ks_bs == (2u << 20) && r.cid.pass.family == kLaunchQuad);
    j.has_ctext = false;  // no ctext in memory: the one k_pass launch
    r = post_route(j, k);
    CHECK(!r.cid.keystream && r.cid.pass.family == kLaunchPass && r.cid.pass.form == 0);
  }
}

static LaunchRec rec(uint32_t tag) {
  return LaunchRec{kLaunchPass, tag, tag & 1, 1, 2, 0, tag + 1, 0, 0, tag + 2};
}

static void test_launch_log() {
  {
    LaunchLog log(4);
    CHECK(!log.on());  // off until enabled: the launch sites append nothing
    log.enable();
    CHECK(log.on() && log.kept() == 0);
    uint32_t out[8 * kLaunchRecWords];
    memset(out, 0xee, sizeof out);
    CHECK(log.read(false, out, 8) == 0 && out[0] == 0xeeeeeeeeu);
    // append: the records come back in order, every word in its place
    const LaunchRec dc{kLaunchPassDc, 4, 1, 1, 2, 1, 4608, 4, 4608, 1024};
    log.append(rec(7));
    log.append(dc);
    CHECK(log.read(false, out, 8) == 2);
    const uint32_t want0[kLaunchRecWords] = {kLaunchPass, 7, 1, 1, 2, 0, 8, 0, 0, 9};
    const uint32_t want1[kLaunchRecWords] = {kLaunchPassDc, 4, 1, 1, 2, 1, 4608, 4, 4608, 1024};
    CHECK(memcmp(out, want0, sizeof want0) == 0);
    CHECK(memcmp(out + kLaunchRecWords, want1, sizeof want1) == 0);
    CHECK(out[2 * kLaunchRecWords] == 0xeeeeeeeeu);  // nothing past the records
    // a reader's buffer smaller than the log: only that many, the count whole
    memset(out, 0xee, sizeof out);
    CHECK(log.read(false, out, 1) == 2 && out[kLaunchRecWords] == 0xeeeeeeeeu);
    CHECK(log.read(false, nullptr, 0) == 2);
    // the cap: the first four are kept, the rest only counted
    for (uint32_t i = 0; i < 5; ++i) log.append(rec(100 + i));
    CHECK(log.kept() == 4);
    memset(out, 0xee, sizeof out);
    CHECK(log.read(true, out, 8) == 7);
    CHECK(out[3 * kLaunchRecWords + 1] == 101 && out[4 * kLaunchRecWords] == 0xeeeeeeeeu);
    // reset: empty, still on, and it fills again
    CHECK(log.on() && log.kept() == 0 && log.read(false, out, 8) == 0);
    log.append(rec(1));
    CHECK(log.read(true, out, 8) == 1 && out[1] == 1);
    CHECK(log.read(false, out, 8) == 0);
  }
  {
    // two threads append at once: every record whole, each thread's in order
    LaunchLog log(4096);
    log.enable();
    auto work = [&log](uint32_t base) {
      for (uint32_t i = 0; i < 1500; ++i) log.append(rec(base + i));
    };
    std::thread a(work, 0u), b(work, 1u << 20);
    a.join();
    b.join();
    std::vector<uint32_t> out(4096 * kLaunchRecWords);
    CHECK(log.read(false, out.data(), 4096) == 3000 && log.kept() == 3000);
    uint32_t next[2] = {0, 0};
    for (size_t i = 0; i < 3000; ++i) {
      const uint32_t *w = &out[i * kLaunchRecWords];
      const uint32_t tag = w[1], who = tag >> 20, k = tag & ((1u << 20) - 1);
      CHECK(who < 2 && k == next[who]);
      CHECK(w[0] == kLaunchPass && w[2] == (tag & 1) && w[6] == tag + 1 && w[9] == tag + 2);
      if (who < 2) ++next[who];
    }
    CHECK(next[0] == 1500 && next[1] == 1500);
    // past the cap from two threads: the count is exact, the log is full
    std::thread c(work, 0u), d(work, 1u << 20);
    c.join();
    d.join();
    CHECK(log.read(true, out.data(), 4096) == 6000);
    CHECK(log.kept() == 0);
  }
}

int main() {
  test_launch_log();
  test_ensure();
  test_failures();
  test_registry();
  test_stream_device();
  test_pass_plan();
  test_other_plans();
  if (g_failed) {
    fprintf(stderr, "stream_scratch_test: %d checks failed\n", g_failed);
    return 1;
  }
  printf("stream_scratch_test: ok\n");
  return 0;
}
