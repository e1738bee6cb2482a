// oneshot.cpp -- the coalescing one-shot poster, and the two ways one
// message from host memory is posted (one-shot, or through device staging).
#include <chrono>
#include <sched.h>
#include <sys/prctl.h>
#include <thread>

#include "host.h"
#include "one_classes.h"

namespace glfsx {
namespace host {

// ---- One-shot posts (launch_one_class) ----
// A post of one message of at most kMaxMedLen bytes from host memory: the
// bytes sit in pinned staging, the kernel reads them there and writes ctext
// and ref straight back into pinned staging, then sets the request's flag
// (pinned, OneDesc::flag) to the launch's sequence number, so a post is one
// launch and a wait on a host word -- no stream query.
// Concurrent callers (glfs.Machine is used from many goroutines) are
// coalesced, group-commit style: a caller that finds the leadership free
// and a free launch lane takes every pending request into one launch (one
// workgroup each) and hands the leadership on at once; every caller then
// waits for its own flag.  A lane is free again once its launch has
// completed (its descriptors and flags are read and written until then):
// up to kOneLanes launches are in flight, each carrying whatever queued
// while the earlier ones ran.
constexpr uint32_t kOneBatch = 1024;
constexpr int kOneLanes = 8;
struct OneLane {
  bool busy = false;          // a launch in flight (read and written by the leader only)
  hipStream_t s = nullptr;
  hipEvent_t ev = nullptr;    // recorded after the launch
  uint32_t seq = 0;           // the last launch's sequence number
  OneDesc *h_desc = nullptr;  // pinned, kOneBatch descriptors
  OneDesc *d_desc = nullptr;  // the kernel's view of h_desc
  OneOpenDesc *h_odesc = nullptr;  // pinned, kOneBatch open descriptors
  OneOpenDesc *d_odesc = nullptr;
  // pinned, kOneBatch flags + one nobody waits on (glfsx_debug_one_drop)
  uint32_t *h_flag = nullptr, *d_flag = nullptr;
  // medium posts: device copies of the messages, and per descriptor
  // kMedAuxWords words of CVs / arrival counter / DEK (zeroed when grown;
  // the kernels leave every counter at zero)
  DevBuf med_msg, med_aux;
  size_t aux_zeroed = 0;
};
namespace {
constexpr size_t kMedAuxWords = 64 * 8 + 8 + 8;   // cvs, dek, cnt (+ pad)
struct OnePoster {
  int dev = -1;
  // requests not yet launched: a lock-free stack (many callers push, the
  // leader takes it whole)
  std::atomic<OneReq *> pending{nullptr};
  std::atomic<bool> leader{false};
  std::atomic<int> spinners{0};  // callers polling their flag without sleeping
  OneLane lane[kOneLanes];
};
// glfsx_one_stats: launches, requests launched, lane-full events
std::atomic<uint64_t> g_one_stats[3];
constexpr int kMaxPosterDevs = 64;
std::mutex g_posters_mu;                               // creation only
std::atomic<OnePoster *> g_posters[kMaxPosterDevs];    // one per device, process lifetime

int poster_get(int dev, OnePoster **out) {
  if (dev < 0 || dev >= kMaxPosterDevs) return fail(GLFSX_E_DEVICE, "device %d", dev);
  if ((*out = g_posters[dev].load(std::memory_order_acquire))) return 0;
  std::lock_guard<std::mutex> lk(g_posters_mu);
  if ((*out = g_posters[dev].load(std::memory_order_acquire))) return 0;
  auto *p = new OnePoster();
  p->dev = dev;
  for (OneLane &l : p->lane) {
    void *h = nullptr, *d = nullptr, *hf = nullptr, *df = nullptr, *ho = nullptr, *dox = nullptr;
    if (hipStreamCreateWithFlags(&l.s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&l.ev, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&h, sizeof(OneDesc) * kOneBatch, hipHostMallocDefault) != hipSuccess ||
        hipHostGetDevicePointer(&d, h, 0) != hipSuccess ||
        hipHostMalloc(&ho, sizeof(OneOpenDesc) * kOneBatch, hipHostMallocDefault) != hipSuccess ||
        hipHostGetDevicePointer(&dox, ho, 0) != hipSuccess ||
        hipHostMalloc(&hf, sizeof(uint32_t) * (kOneBatch + 1), hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(&df, hf, 0) != hipSuccess) {
      for (OneLane &x : p->lane) {
        if (x.h_desc) (void)hipHostFree(x.h_desc);
        if (x.h_odesc) (void)hipHostFree(x.h_odesc);
        if (x.h_flag) (void)hipHostFree(x.h_flag);
        if (x.s) (void)hipStreamDestroy(x.s);
        if (x.ev) (void)hipEventDestroy(x.ev);
      }
      if (h && h != static_cast<void *>(l.h_desc)) (void)hipHostFree(h);
      if (ho) (void)hipHostFree(ho);
      if (hf) (void)hipHostFree(hf);
      delete p;
      return fail(GLFSX_E_DEVICE, "one-shot post setup failed on device %d", dev);
    }
    l.h_desc = static_cast<OneDesc *>(h);
    l.d_desc = static_cast<OneDesc *>(d);
    l.h_odesc = static_cast<OneOpenDesc *>(ho);
    l.d_odesc = static_cast<OneOpenDesc *>(dox);
    l.h_flag = static_cast<uint32_t *>(hf);
    l.d_flag = static_cast<uint32_t *>(df);
    memset(hf, 0, sizeof(uint32_t) * (kOneBatch + 1));
  }
  g_posters[dev].store(p, std::memory_order_release);
  *out = p;
  return 0;
}

void pending_push(OnePoster *P, OneReq *r) {
  OneReq *h = P->pending.load(std::memory_order_relaxed);
  do {
    r->next = h;
  } while (!P->pending.compare_exchange_weak(h, r, std::memory_order_release,
                                             std::memory_order_relaxed));
}

// Test hook (glfsx_debug_one_drop): the next launch sends request k's
// result flag to the lane's spare word, as a launch that failed on the
// device would leave it: the request's caller must see the error, and no
// caller may return while a request of its call is still queued.
std::atomic<uint32_t> g_one_drop{~0u};

// The batch's classes (one_classes.h) each in their own descriptor range,
// and one launch_one_class per class present on the lane's stream: k_one over
// the small posts, the medium pair over the medium ones, k_one_open over the
// opens without and with a DEK check; request k's flag is lane.h_flag[k], set
// to `seq` when its results are in place.
int one_launch(OneLane &L, const std::vector<OneReq *> &batch, uint32_t seq) {
  const uint32_t drop = g_one_drop.exchange(~0u, std::memory_order_relaxed);
  std::vector<OneItem> items(batch.size());
  for (size_t k = 0; k < batch.size(); ++k)
    items[k] = OneItem{batch[k]->open, batch[k]->salted, batch[k]->len()};
  const OneLayout lay = one_layout(items.data(), items.size(), kMaxOneLen);
  if (const uint32_t nm = lay.count[kOneMed]) {
    if (int e = L.med_msg.ensure(lay.med_bytes)) return e;
    if (int e = L.med_aux.ensure(nm * kMedAuxWords * 4)) return e;
    if (L.med_aux.cap > L.aux_zeroed) {  // new buffer: counters must start at zero
      HIP_TRY(hipMemsetAsync(L.med_aux.p, 0, L.med_aux.cap, L.s));
      L.aux_zeroed = L.med_aux.cap;
    }
  }
  for (size_t k = 0; k < batch.size(); ++k) {
    const OneReq *r = batch[k];
    uint32_t *const flag = L.d_flag + (k == drop ? kOneBatch : k);
    const uint32_t slot = lay.slot[k];
    if (r->open) {
      OneOpenDesc o = r->o;
      o.flag = flag;
      o.seq = seq;
      L.h_odesc[slot] = o;
      continue;
    }
    OneDesc d = r->d;
    d.flag = flag;
    d.seq = seq;
    if (lay.cls[k] == kOneMed) {
      uint32_t *aux = reinterpret_cast<uint32_t *>(L.med_aux.p) +
                      size_t(slot - lay.start[kOneMed]) * kMedAuxWords;
      d.dmsg = L.med_msg.u8() + lay.med_off[k];
      d.cvs = aux;
      d.dek = aux + 64 * 8;
      d.cnt = aux + 64 * 8 + 8;
    }
    L.h_desc[slot] = d;
  }
  for (const OneClass c : {kOneSmall, kOneMed, kOneOpen, kOneOpenSalted}) {
    const uint32_t n = lay.count[c], at = lay.start[c];
    if (c == kOneSmall || c == kOneMed)
      HIP_TRY(launch_one_class(c, L.h_desc + at, L.d_desc + at, n, lay.max_len[c], L.s));
    else
      HIP_TRY(launch_one_class(c, L.h_odesc + at, L.d_odesc + at, n, lay.max_len[c], L.s));
  }
  HIP_TRY(hipEventRecord(L.ev, L.s));
  return 0;
}

// Request r has its results: its flag reached its launch's sequence number.
bool one_finished(const OneReq *r) {
  if (!r->armed.load(std::memory_order_acquire)) return false;
  const uint32_t v = __atomic_load_n(r->flag, __ATOMIC_ACQUIRE);
  return int32_t(v - r->seq) >= 0;
}

const int kOneSpinners = [] {
  const int h = int(std::thread::hardware_concurrency());
  return std::min(16, std::max(4, h / 2));
}();
constexpr int64_t kOneSpinNs = 300000;
// A sleeping waiter's 10 us sleeps would otherwise end up to the default
// 50 us timer slack late: while a caller's thread sleeps in a one-shot wait
// its slack is 1 us, and the thread's own slack is restored when the wait
// returns (the caller's thread -- a Go runtime M, an application thread --
// is not the library's to retune).
struct SleepSlack {
  long saved = -1;
  void on() {
    if (saved >= 0) return;
    saved = prctl(PR_GET_TIMERSLACK, 0UL, 0UL, 0UL, 0UL);
    if (saved < 0) {
      saved = -2;  // unknown: leave it alone
      return;
    }
    prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL);
  }
  ~SleepSlack() {
    if (saved >= 0) prctl(PR_SET_TIMERSLACK, static_cast<unsigned long>(saved), 0UL, 0UL, 0UL);
  }
};

}  // namespace

int one_post_many(int dev, OneReq *const *rs, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const OneReq *r = rs[i];
    const bool bad = r->open ? r->o.len > kMaxOneLen || !r->o.status ||
                                   ((reinterpret_cast<uintptr_t>(r->o.src) |
                                     reinterpret_cast<uintptr_t>(r->o.ptext)) & 15)
                             : r->d.len > kMaxMedLen ||
                                   (reinterpret_cast<uintptr_t>(r->d.src) & 15);
    if (bad) return fail(GLFSX_E_ARG, "one-shot post: bad descriptor");
  }
  OnePoster *P;
  if (int e = poster_get(dev, &P)) return e;
  for (size_t i = 0; i < n; ++i) pending_push(P, rs[i]);
  // Waiting: at most kOneSpinners callers (half the host's threads, 4-16)
  // poll with `pause` (a post is ~45-190 us; up to kOneSpinNs); the others,
  // and a spinner past that bound, sleep between polls.  Yielding instead (round 4) kept
  // every waiting caller runnable: at 64-256 callers on a 16-core share
  // the callers that had work (the leader, a caller whose post finished)
  // waited for a core.
  bool spin = P->spinners.fetch_add(1, std::memory_order_relaxed) < kOneSpinners;
  if (!spin) P->spinners.fetch_sub(1, std::memory_order_relaxed);
  struct Unspin {
    OnePoster *P;
    bool &spin;
    ~Unspin() {
      if (spin) P->spinners.fetch_sub(1, std::memory_order_relaxed);
    }
  } unspin{P, spin};
  SleepSlack slack;
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t sleeps = 0;
  // Once a launch of ours is seen to have failed on the device (frc), the
  // call still returns only when no request of it can be touched again: each
  // is failed before launch, finished, or armed on a lane whose launch has
  // completed.  A request still on the pending stack would otherwise be
  // launched -- its descriptor read, its flag and staging written -- after
  // its caller freed it.
  int frc = 0;
  std::string ferr;
  auto settled = [&frc](const OneReq *r) {
    if (r->done.load(std::memory_order_acquire) || one_finished(r)) return true;
    return frc && r->armed.load(std::memory_order_acquire) &&
           hipEventQuery(r->lane->ev) != hipErrorNotReady;
  };
  size_t ndone = 0;  // rs[0..ndone) are settled
  for (uint32_t spins = 0;; ++spins) {
    while (ndone < n && settled(rs[ndone])) ++ndone;
    if (ndone == n) {
      if (frc) return fail(frc, "%s", ferr.c_str());
      for (size_t i = 0; i < n; ++i)
        if (rs[i]->rc) return fail(rs[i]->rc, "%s", rs[i]->err.c_str());
      return 0;
    }
    // leadership only when there is something to launch and nobody holds it
    // (many waiting callers must not bounce the word between cores)
    bool idle = false;
    if (P->pending.load(std::memory_order_relaxed) &&
        !P->leader.load(std::memory_order_relaxed) &&
        P->leader.compare_exchange_strong(idle, true, std::memory_order_acq_rel)) {
      // a lane whose last launch has completed
      OneLane *L = nullptr;
      int rc = 0;
      for (OneLane &l : P->lane) {
        if (l.busy) {
          const hipError_t q = hipEventQuery(l.ev);
          if (q == hipErrorNotReady) continue;
          if (q != hipSuccess && !rc)
            rc = fail(GLFSX_E_DEVICE, "one-shot post: %s", hipGetErrorString(q));
          l.busy = false;
        }
        L = &l;
        break;
      }
      std::vector<OneReq *> batch;
      if (!L) g_one_stats[2].fetch_add(1, std::memory_order_relaxed);
      if (L) {
        // up to kOneBatch requests, at most kMedBatchBytes of medium ones
        // (always at least one request); the rest goes back on the stack
        OneReq *r = P->pending.exchange(nullptr, std::memory_order_acquire);
        uint64_t mb = 0;
        while (r) {
          OneReq *nx = r->next;
          const uint64_t len = r->len();
          const bool fits = batch.size() < kOneBatch &&
                            (len <= kMaxOneLen || batch.empty() || mb + len <= kMedBatchBytes);
          if (fits) {
            if (len > kMaxOneLen) mb += len;
            batch.push_back(r);
          } else {
            pending_push(P, r);
          }
          r = nx;
        }
      }
      if (!batch.empty()) {
        const uint32_t seq = ++L->seq;
        if (!rc) rc = one_launch(*L, batch, seq);
        if (!rc) {
          g_one_stats[0].fetch_add(1, std::memory_order_relaxed);
          g_one_stats[1].fetch_add(batch.size(), std::memory_order_relaxed);
          L->busy = true;
          for (size_t k = 0; k < batch.size(); ++k) {
            batch[k]->flag = L->h_flag + k;
            batch[k]->seq = seq;
            batch[k]->lane = L;
            batch[k]->armed.store(1, std::memory_order_release);
          }
        } else {
          // nothing of this batch runs: its owners get the error (a
          // request's owner may return, and free it, once done is set)
          (void)hipStreamSynchronize(L->s);
          const std::string msg = last_error_text();
          for (OneReq *b : batch) {
            b->rc = rc;
            b->err = msg;
            b->done.store(1, std::memory_order_release);
          }
        }
      }
      P->leader.store(false, std::memory_order_release);
      continue;
    }
    if (spin) {
      if ((spins & 31) != 0) {
        for (int k = 0; k < 8; ++k) __builtin_ia32_pause();
        continue;
      }
      // every 32 polls: the core goes to any runnable thread (the HIP
      // runtime's own, a caller with work), and the spin bound is checked
      sched_yield();
      if (std::chrono::duration_cast<std::chrono::nanoseconds>(
              std::chrono::steady_clock::now() - t0).count() < kOneSpinNs)
        continue;
      spin = false;
      P->spinners.fetch_sub(1, std::memory_order_relaxed);
    }
    // sleepers back off 10 -> 40 us: hundreds of them must not wake 100 k
    // times a second each
    slack.on();
    std::this_thread::sleep_for(std::chrono::microseconds(10u << std::min(sleeps, 2u)));
    if (!frc && ++sleeps % 1024 == 0) {
      // a long wait: a launch that failed on the device never sets its flags
      for (size_t i = ndone; i < n; ++i) {
        const OneReq *r = rs[i];
        if (!r->armed.load(std::memory_order_acquire) || one_finished(r)) continue;
        // (the lane's event is ours or a later launch's: either way ours
        // has completed when it has)
        const hipError_t q = hipEventQuery(r->lane->ev);
        if (q == hipErrorNotReady || one_finished(r)) continue;
        frc = GLFSX_E_DEVICE;
        ferr = std::string("one-shot post: ") +
               (q == hipSuccess ? "the launch completed without its result flag"
                                : hipGetErrorString(q));
        break;
      }
    }
  }
}

int post_host_message(int dev, OneStaging st, const uint8_t salt[32], const uint8_t *cid_key,
                      const uint8_t *data, uint64_t n, bool want_ctext, uint8_t ref[64],
                      glfsx_post_fn post, void *post_ctx, int kind, const PinBuf *pin,
                      uint64_t present) {
  if (int e = st.h_ct.ensure(n + 64)) return e;
  if (int e = st.h_ref.ensure(64)) return e;
  const uint64_t have = std::min(n, present);
  OneReq r;
  if (pin && pin->dp && ((data - pin->u8()) & 15) == 0) {
    r.d.src = pin->dptr() + (data - pin->u8());
  } else {
    if (int e = st.h_in.ensure(n + 64)) return e;
    if (have) par_memcpy(st.h_in.u8(), data, have);
    r.d.src = st.h_in.dptr();
  }
  r.d.ctext = want_ctext ? st.h_ct.dptr() : nullptr;
  r.d.ref = st.h_ref.dptr();
  r.d.len = uint32_t(n);
  r.d.present = uint32_t(have);
  set_keys(r.d, salt, cid_key);
  OneReq *rp = &r;
  if (int e = one_post_many(dev, &rp, 1)) return e;
  memcpy(ref, st.h_ref.p, 64);
  return deliver(post, post_ctx, kind, ref, st.h_ct.p, n);
}

int open_host_message(int dev, OneStaging st, const uint8_t *salt, const uint8_t *cid_key,
                      const uint8_t ref[64], const uint8_t *ctext, uint64_t n, void *ptext,
                      uint32_t *status) {
  if (int e = st.h_in.ensure(n + 64)) return e;
  if (ptext)
    if (int e = st.h_ct.ensure(n + 64)) return e;
  if (int e = st.h_ref.ensure(64)) return e;
  if (n) par_memcpy(st.h_in.u8(), ctext, n);
  OneReq r;
  r.open = true;
  r.salted = salt != nullptr;
  r.o.src = st.h_in.dptr();
  r.o.ptext = ptext ? st.h_ct.dptr() : nullptr;
  r.o.status = reinterpret_cast<uint32_t *>(st.h_ref.dptr());
  words_from_key(r.o.ref, ref);
  words_from_key(r.o.ref + 8, ref + 32);
  r.o.len = uint32_t(n);
  if (salt) words_from_key(r.o.salt, salt);
  set_cid_key(r.o, cid_key);
  OneReq *rp = &r;
  if (int e = one_post_many(dev, &rp, 1)) return e;
  *status = *reinterpret_cast<const uint32_t *>(st.h_ref.p);
  if (ptext && n) memcpy(ptext, st.h_ct.p, n);
  return 0;
}

int post_staged_message(hipStream_t s, DevStaging st, const uint8_t salt[32],
                        const uint8_t *cid_key, const uint8_t *data, uint64_t n, void *ct_dst,
                        void *ref_dst, hipEvent_t src_ready, hipStream_t src_stream) {
  if (int e = st.d_in.ensure(n + 64)) return e;
  if (int e = st.d_ct.ensure(n + 64)) return e;
  if (int e = st.d_ref.ensure(64)) return e;
  if (src_ready) {
    HIP_TRY(hipEventRecord(src_ready, src_stream));
    HIP_TRY(hipStreamWaitEvent(s, src_ready, 0));
  } else if (n) {
    HIP_TRY(hipMemcpyAsync(st.d_in.p, data, n, hipMemcpyHostToDevice, s));
  }
  PostJob j = single_job(src_ready ? data : st.d_in.u8(), n, st.d_ct.u8(), st.d_ref.u8());
  set_keys(j, salt, cid_key);
  HIP_TRY(launch_post(j, s, fused_posts()));
  if (ct_dst && n) HIP_TRY(hipMemcpyAsync(ct_dst, st.d_ct.p, n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(ref_dst, st.d_ref.p, 64, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  return 0;
}

}  // namespace host
}  // namespace glfsx

using namespace glfsx;
using namespace glfsx::host;

extern "C" {

void glfsx_debug_one_drop(uint32_t k) { g_one_drop.store(k, std::memory_order_relaxed); }

int glfsx_one_stats(int reset, uint64_t out[3]) {
  for (int i = 0; i < 3; ++i) {
    const uint64_t v = reset ? g_one_stats[i].exchange(0, std::memory_order_relaxed)
                             : g_one_stats[i].load(std::memory_order_relaxed);
    if (out) out[i] = v;
  }
  return 0;
}

}  // extern "C"
