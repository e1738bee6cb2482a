// host.h -- what the units of the host runtime behind include/glfsx.h share.
//
// C++ mirror of the reference's bigblob write-path interface (the reference is
// Go; with no Go toolchain in this image the host side above the C-ABI is C++,
// see DESIGN.md "Boundary").  All hashing/encryption runs in the gfx950
// kernels of post_kernels.hip; the host units only stage bytes, sequence
// launches and keep the reference's Writer bookkeeping (blob.go:71-206); one
// unit per family (DESIGN.md "Host language").  Internal: hidden visibility.
// writer_book.h: that bookkeeping (fill cursor, index stack) as pure state.
// ragged_groups.h: a batch's groups and the run copier (ragged_runs).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/glfsx.h"
#include "kernels.h"

namespace glfsx {
namespace host __attribute__((visibility("hidden"))) {

// The calling thread's state (error text, device, contexts, fused mode) is
// thread-local in runtime.cpp alone: a hidden thread_local shared between
// units goes through a weak init hook a shared library cannot resolve to null.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const std::string &last_error_text();  // what fail() recorded (glfsx_last_error)
void set_thread_device(int dev);       // the device ctx_get serves next

#define HIP_TRY(expr)                                                     \
  do {                                                                    \
    hipError_t e_ = (expr);                                               \
    if (e_ != hipSuccess)                                                 \
      return fail(GLFSX_E_DEVICE, "%s: %s (%s:%d)", #expr,                \
                  hipGetErrorString(e_), __FILE__, __LINE__);             \
  } while (0)

// A store's Post of one message (ref.go:98 sink).
inline int deliver(glfsx_post_fn post, void *post_ctx, int kind, const uint8_t *ref,
                   const void *ctext, uint64_t len) {
  if (!post) return 0;
  const int rc = post(post_ctx, kind, ref, ctext, len);
  return rc ? fail(GLFSX_E_STORE, "store.Post failed with code %d", rc) : 0;
}

// Grow-only device / pinned-host buffer, owning its allocation (move-only).
// `dirty`: how far from the start the bytes may be non-zero (index-node
// images, level_prepare); SIZE_MAX = unknown.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  size_t dirty = SIZE_MAX;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
      dirty = std::exchange(o.dirty, SIZE_MAX);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    dirty = SIZE_MAX;
  }
  int ensure(size_t n) {
    if (n <= cap) return 0;
    reset();
    size_t want = std::max<size_t>(n, 4096);
    HIP_TRY(hipMalloc(&p, want));
    cap = want;
    return 0;
  }
  uint8_t *u8() const { return static_cast<uint8_t *>(p); }
};
struct PinBuf {
  void *p = nullptr;
  void *dp = nullptr;  // the same memory as the kernels address it
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(PinBuf &&o) noexcept { *this = std::move(o); }
  PinBuf &operator=(PinBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      dp = std::exchange(o.dp, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~PinBuf() { reset(); }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = dp = nullptr;
    cap = 0;
  }
  int ensure(size_t n) {
    if (n <= cap) return 0;
    reset();
    size_t want = std::max<size_t>(n, 4096);
    HIP_TRY(hipHostMalloc(&p, want, hipHostMallocPortable));
    cap = want;
    HIP_TRY(hipHostGetDevicePointer(&dp, p, 0));
    return 0;
  }
  // Grow (at least doubling) keeping the first `keep` bytes.
  int grow(size_t need, size_t keep) {
    if (need <= cap) return 0;
    PinBuf b;
    b.cap = std::max(need, cap * 2);
    HIP_TRY(hipHostMalloc(&b.p, b.cap, hipHostMallocPortable));
    if (hipHostGetDevicePointer(&b.dp, b.p, 0) != hipSuccess)
      return fail(GLFSX_E_DEVICE, "hipHostGetDevicePointer failed");
    if (p && keep) memcpy(b.p, p, keep);
    *this = std::move(b);
    return 0;
  }
  uint8_t *u8() const { return static_cast<uint8_t *>(p); }
  uint8_t *dptr() const { return static_cast<uint8_t *>(dp); }
};
// An event (timing disabled) made on first use, owned likewise.
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
  Event &operator=(Event &&o) noexcept {
    if (this != &o) {
      reset();
      e = std::exchange(o.e, nullptr);
    }
    return *this;
  }
  ~Event() { reset(); }
  void reset() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  int ensure() {
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return 0;
  }
  operator hipEvent_t() const { return e; }
};

// Resources that outlive their users, keyed by device (T::dev; an empty T has
// dev < 0): take() hands out one pooled for the device or an empty T, give()
// keeps up to `cap` of them and destroys the rest.  The pool only moves and
// destroys T.  The process-wide pools are never destroyed (see ~Ctx): each is
// allocated once behind a function-local static pointer and leaked.
template <class T>
class DevicePool {
 public:
  explicit DevicePool(size_t cap) : cap_(cap) {}
  T take(int dev) {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = v_.size(); i-- > 0;)
      if (v_[i].dev == dev) {
        T x = std::move(v_[i]);
        v_.erase(v_.begin() + i);
        return x;
      }
    return T();
  }
  void give(T &&x) {
    T drop;  // destroyed after the lock is released
    std::lock_guard<std::mutex> lk(mu_);
    if (x.dev >= 0 && v_.size() < cap_)
      v_.push_back(std::move(x));
    else
      drop = std::move(x);
  }
  size_t size() {
    std::lock_guard<std::mutex> lk(mu_);
    return v_.size();
  }

 private:
  std::mutex mu_;
  std::vector<T> v_;
  const size_t cap_;
};

// Per-thread device context: the library is reentrant because every host
// thread gets its own stream and staging (bigblob.Writer is single-goroutine,
// glfs.Machine is used concurrently: SURVEY 8b "Threading").
struct Ctx {
  int dev = -1;
  hipStream_t stream = nullptr;
  DevBuf d_in, d_ct, d_refs, d_lvl_a, d_lvl_b, d_small, d_tree;
  PinBuf h_small, h_root;      // h_root: a root ref written by the kernels
  PinBuf h_oin, h_oct, h_oref;  // glfsx_post's one-shot staging
  // glfsx_post_blobs' single-block blobs from host memory: groups of <= 64 MiB
  // through three pinned slots, upload / hash / download on three streams
  struct BlobSlot {
    PinBuf h_in, h_ct, h_meta, h_refs;  // h_meta: local offsets then lengths
    DevBuf d_in, d_ct, d_meta, d_refs;
    Event done, up, hashed;
    uint64_t i0 = 0, i1 = 0;            // the group's blob index range
    std::vector<uint64_t> loff;         // local offset of each blob in the range
    bool busy = false;
  } bslot[3];
  hipStream_t s_up = nullptr, s_down = nullptr;
  // glfsx_post_tree_device: a second stream for the tree blob's posts, its
  // events, and the tree layout on the host
  hipStream_t stream2 = nullptr;
  Event events[3];
  PinBuf h_tree;
  ~Ctx() {
    // Process teardown may already have unloaded the HIP runtime; leak.
    // (Contexts are new'ed per thread and never deleted, so the owning
    // members above free nothing then.)
  }
};
// The calling thread's context on its device, made current.
int ctx_get(Ctx **out);

inline hipStream_t pick_stream(Ctx *c, void *stream) {
  return stream ? static_cast<hipStream_t>(stream) : c->stream;
}

// Wait for a stream whose results the caller is about to return (polls
// first, see runtime.cpp).
hipError_t stream_wait(hipStream_t s);

// One-launch split posts (k_pass_dc) report a failed DEK wait through a
// word the host reads after the stream drains (fused_errors_take); the
// calls that sync check it and repeat the work with two launches per post.
// fused_posts() is false while repeating; fused_check marks the failure.
bool fused_posts();
int fused_check(hipStream_t s);

// Run f(); if it failed because a one-launch split post failed, run it again
// with two launches per post.
int fused_retry(int (*f)(void *), void *arg);
template <class F>
int with_fused_retry(F &&f) {
  return fused_retry([](void *p) { return (*static_cast<std::remove_reference_t<F> *>(p))(); },
                     &f);
}

// Make `dev` current for a scope and the device that was current before it
// current again at its end (a writer's lanes may live on other devices than
// its home).  The device actually current is read, not assumed: scopes nest
// (submit on lane k completes a batch of lane j, whose replay posts on the
// home device), and a scope that trusted a `home` argument skipped the
// switch while another lane's device was current.
struct DevScope {
  int prev = -1, dev;
  explicit DevScope(int dev_) : dev(dev_) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DevScope() {
    if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
  }
};

// blob.go:99-101: the (indexSalt, rawSalt) pair of a salt (null: zeros),
// memoised.
struct Salts {
  uint8_t raw[32], index[32];
};
int derive_salts(Ctx *c, const uint8_t *salt, Salts *s);

// blob.go:93-95 and the kernels' limit; the batch entry points' looser check.
int check_block_size(uint64_t bs);
int check_batch_block_size(uint64_t bs);

// ---- Job builders: the one place a PostJob / key words are filled in ----
// Dense refs (ref j at byte 64j) and index-node refs (index.go:33-38).
inline RefLayout dense_refs(void *p) { return RefLayout{static_cast<uint8_t *>(p), ~0ull, 0}; }
inline RefLayout node_refs(void *p, uint64_t bs) {
  return RefLayout{static_cast<uint8_t *>(p), bs / 64, bs};
}
// ceil(total / bs) blocks of bs bytes back to back at src, the last one short.
inline PostJob block_job(const void *src, uint64_t total, uint64_t bs, void *ctext,
                         RefLayout out) {
  PostJob j{};
  j.src = static_cast<const uint8_t *>(src);
  j.ctext = static_cast<uint8_t *>(ctext);
  j.stride = j.msg_len = bs;
  j.n = (total + bs - 1) / bs;
  j.last_len = j.n ? total - (j.n - 1) * bs : 0;
  j.out = out;
  return j;
}
// One message of len bytes (0: the empty message, one empty chunk).
inline PostJob single_job(const void *src, uint64_t len, void *ctext, void *out) {
  PostJob j{};
  j.src = static_cast<const uint8_t *>(src);
  j.ctext = static_cast<uint8_t *>(ctext);
  j.msg_len = j.last_len = len;
  j.n = 1;
  j.out = dense_refs(out);
  return j;
}
// The CID key's words (the IV when unkeyed) and the DEK salt's, for PostJob,
// OneDesc and SmallJob (which carries both salts of a blob).
template <class J>
void set_cid_key(J &j, const uint8_t *cid_key) {
  if (cid_key)
    words_from_key(j.cid_key, cid_key);
  else
    blake3_iv_words(j.cid_key);
  j.cid_keyed = cid_key != nullptr;
}
template <class J>
void set_keys(J &j, const uint8_t salt[32], const uint8_t *cid_key) {
  words_from_key(j.salt, salt);
  set_cid_key(j, cid_key);
}
inline void set_keys(SmallJob &j, const Salts &s, const uint8_t *cid_key) {
  words_from_key(j.raw_salt, s.raw);
  words_from_key(j.index_salt, s.index);
  set_cid_key(j, cid_key);
}
// The read side's keys (OpenJob, OpenRaggedJob): salt null = the CID check only.
template <class J>
void open_keys(J &j, const uint8_t *salt, const uint8_t *cid_key) {
  j.salted = salt != nullptr;
  if (salt) words_from_key(j.salt, salt);
  set_cid_key(j, cid_key);
}
// n blobs, blob i the lens[i] bytes at offs[i] of src (device arrays), its
// root to refs + 64 i: those of at most small_max bytes, one lane each.
inline SmallJob small_job(const void *src, void *ctext, const uint64_t *offs,
                          const uint64_t *lens, uint64_t n, uint64_t max_len,
                          uint64_t small_max, void *refs) {
  SmallJob j{};
  j.src = static_cast<const uint8_t *>(src);
  j.ctext = static_cast<uint8_t *>(ctext);
  j.offs = offs;
  j.lens = lens;
  j.n = n;
  j.max_len = max_len;
  j.small_max = small_max;
  j.refs = static_cast<uint8_t *>(refs);
  return j;
}
// The same layout, the messages of lo < lens[i] <= hi bytes in throughput form.
inline RaggedJob ragged_job(const void *src, void *ctext, const uint64_t *offs,
                            const uint64_t *lens, uint64_t n, uint64_t lo, uint64_t hi,
                            void *refs) {
  RaggedJob j{};
  j.src = static_cast<const uint8_t *>(src);
  j.ctext = static_cast<uint8_t *>(ctext);
  j.offs = offs;
  j.lens = lens;
  j.n = n;
  j.lo = lo;
  j.hi = hi;
  j.refs = static_cast<uint8_t *>(refs);
  return j;
}
// The verified read of ceil(total / bs) blocks of bs bytes back to back at
// ctext, the last one short (total 0: one empty block).
inline OpenJob open_job(const void *ctext, void *ptext, uint64_t total, uint64_t bs,
                        const void *refs, uint32_t *status) {
  OpenJob j{};
  j.ctext = static_cast<const uint8_t *>(ctext);
  j.ptext = static_cast<uint8_t *>(ptext);
  j.n = total ? (total + bs - 1) / bs : 1;
  j.bs = bs;
  j.last_len = total - (j.n - 1) * bs;
  j.refs = static_cast<const uint8_t *>(refs);
  j.status = status;
  return j;
}
// The same of n messages, message i the lens[i] bytes at offs[i] of ctext.
inline OpenRaggedJob open_ragged_job(const void *ctext, void *ptext, const uint64_t *offs,
                                     const uint64_t *lens, uint64_t n, uint64_t max_len,
                                     const void *refs, uint32_t *status) {
  OpenRaggedJob j{};
  j.ctext = static_cast<const uint8_t *>(ctext);
  j.ptext = static_cast<uint8_t *>(ptext);
  j.offs = offs;
  j.lens = lens;
  j.n = n;
  j.max_len = max_len;
  j.refs = static_cast<const uint8_t *>(refs);
  j.status = status;
  return j;
}
// The columns of n tree entries, the `words` words of scratch their lines'
// layout takes (the total in the last one) and the cap bytes at out.
inline TreeJob tree_job(uint64_t n, const uint8_t *names, const uint64_t *name_offs,
                        const uint32_t *modes, const uint8_t *types, const uint64_t *type_offs,
                        const void *roots, const uint64_t *sizes, const uint64_t *block_sizes,
                        void *scratch, uint64_t words, void *out, uint64_t cap) {
  TreeJob j{};
  j.n = n;
  j.names = names;
  j.name_offs = name_offs;
  j.modes = modes;
  j.types = types;
  j.type_offs = type_offs;
  j.roots = static_cast<const uint8_t *>(roots);
  j.sizes = sizes;
  j.block_sizes = block_sizes;
  j.scratch = static_cast<uint64_t *>(scratch);
  j.total = j.scratch + words - 1;
  j.out = static_cast<uint8_t *>(out);
  j.cap = cap;
  return j;
}

// The text of a failed verified read: "failed its CID and DEK checks", ...
inline const char *failed_checks(uint32_t status) {
  return status == 3 ? "failed its CID and DEK checks"
                     : status == 1 ? "failed its CID check" : "failed its DEK check";
}
// GLFSX_E_CORRUPT for a batch of n `what`s (block, message), bad of them bad.
inline int corrupt_fail(const char *what, uint64_t first_bad, uint64_t n, uint32_t status,
                        uint64_t bad) {
  return fail(GLFSX_E_CORRUPT, "%s %llu of %llu %s (%llu bad in all)", what,
              (unsigned long long)first_bad, (unsigned long long)n, failed_checks(status),
              (unsigned long long)bad);
}

// ---- oneshot.cpp ----
// A one-shot request: a post -- fill in d (src, ctext, ref, len, present and
// the keys) -- or, with open set, a verified read -- fill in o (src, ptext,
// status, ref, len and the keys) and salted; the rest belongs to the poster.
struct OneLane;
struct OneReq {
  OneDesc d{};
  bool open = false;    // the request's kind
  bool salted = false;  // an open that checks the DEK too
  OneOpenDesc o{};
  uint32_t len() const { return open ? o.len : d.len; }
  OneReq *next = nullptr;     // the pending stack
  std::atomic<int> armed{0};  // flag / seq / lane below are set (by the leader)
  std::atomic<int> done{0};   // failed before launch (rc, err)
  const uint32_t *flag = nullptr;
  uint32_t seq = 0;
  OneLane *lane = nullptr;
  int rc = 0;
  std::string err;
};
constexpr uint64_t kMedBatchBytes = 64ull << 20;  // device copies per launch
// Run rs[0..n) on device dev (the calling thread's current device); returns
// when every request's results (ctext and ref; plaintext and status) are in
// its staging.  Posts and opens of concurrent callers share launches.
int one_post_many(int dev, OneReq *const *rs, size_t n);

// Post one message of at most kMaxMedLen bytes from host memory (ref.go:98
// post + sink) as a one-shot post through the pinned staging h_in / h_ct /
// h_ref: the ref goes to `ref`, the ctext (if want_ctext) stays in h_ct and
// goes to `post`.  `data` is read in place when it lies 16-B aligned in the
// pinned buffer `pin`; bytes [present, n) of the message are zero.
struct OneStaging {
  PinBuf &h_in, &h_ct, &h_ref;
};
int post_host_message(int dev, OneStaging st, const uint8_t salt[32], const uint8_t *cid_key,
                      const uint8_t *data, uint64_t n, bool want_ctext, uint8_t ref[64],
                      glfsx_post_fn post = nullptr, void *post_ctx = nullptr, int kind = 0,
                      const PinBuf *pin = nullptr, uint64_t present = ~0ull);
// getF with its checks (ref.go:113-126) for one block of at most kMaxOneLen
// bytes from host memory, as a one-shot open: the ctext is copied into h_in,
// the plaintext (if ptext) comes back through h_ct and the status word
// through h_ref.  salt null: the CID check only.  ptext may equal ctext.
int open_host_message(int dev, OneStaging st, const uint8_t *salt, const uint8_t *cid_key,
                      const uint8_t ref[64], const uint8_t *ctext, uint64_t n, void *ptext,
                      uint32_t *status);
// The same for a message of any length through device staging on stream s:
// the ref is downloaded to ref_dst and the ctext to ct_dst (nullable), and
// the stream waited for.  src_ready set: `data` is device memory written on
// stream src_stream, which the post waits for through that event.
struct DevStaging {
  DevBuf &d_in, &d_ct, &d_ref;
};
int post_staged_message(hipStream_t s, DevStaging st, const uint8_t salt[32],
                        const uint8_t *cid_key, const uint8_t *data, uint64_t n, void *ct_dst,
                        void *ref_dst, hipEvent_t src_ready = nullptr,
                        hipStream_t src_stream = nullptr);

// ---- copy_pool.cpp ----
// dev: the device whose staging dst is (-1: the current device), which
// picks the copy pool of its NUMA node.
void par_memcpy(uint8_t *dst, const uint8_t *src, size_t n, int dev = -1);
void gather_start(std::atomic<int> *left, uint8_t *dst, const void *const *blocks, uint64_t k,
                  uint64_t bs, uint64_t last, int dev = -1);
void gather_wait(std::atomic<int> *left);
int64_t par_read_at(glfsx_read_at_fn fn, void *ctx, uint8_t *dst, uint64_t n, uint64_t off,
                    unsigned max_threads, int dev = -1);

// ---- create.cpp ----
int level_prepare(DevBuf &b, uint64_t n, uint64_t nodes, uint64_t bs, hipStream_t s);
int build_up(Ctx *c, hipStream_t s, const Salts &salts, const uint8_t *cid_key, uint64_t bs,
             uint8_t *cur, uint64_t nodes, DevBuf *spare, uint8_t root_ref[64],
             uint64_t *posts);

}  // namespace host
}  // namespace glfsx
