// create.cpp -- index levels, the single and batched posts, Create from host
// memory, on one device, in shards and over several devices.
#include <condition_variable>
#include <functional>
#include <thread>

#include "host.h"

namespace glfsx {
namespace host {

// The zero-padded node images of a level of n refs (index.go:33-38: slot i
// of node k at k*bs + 64i, everything else zero).  With bs a multiple of 64,
// ref j lands at byte 64j, so a level writes exactly [0, 64n): instead of
// zeroing all nodes*bs bytes before every level, only the bytes an earlier
// use may have left non-zero past 64n are cleared (config 2 posts 512 refs
// into a 2 MiB node: a 5.3 us memset per step went).
int level_prepare(DevBuf &b, uint64_t n, uint64_t nodes, uint64_t bs, hipStream_t s) {
  if (int e = b.ensure(nodes * bs)) return e;
  const size_t used = size_t(64) * n;
  if (bs % 64 || b.dirty == SIZE_MAX) {
    HIP_TRY(hipMemsetAsync(b.p, 0, b.cap, s));
    b.dirty = bs % 64 ? SIZE_MAX : used;
    return 0;
  }
  if (b.dirty > used) HIP_TRY(hipMemsetAsync(b.u8() + used, 0, b.dirty - used, s));
  b.dirty = used;
  return 0;
}

// Post `nodes` index nodes (each exactly bs bytes) starting at d_nodes;
// refs go into the next level's node buffer (or dense when out.bf = max).
static int post_level(hipStream_t s, const uint8_t salt[32], const uint8_t *cid_key,
                      const uint8_t *d_nodes, uint64_t nodes, uint64_t bs, uint8_t *d_ctext,
                      RefLayout out) {
  PostJob j = block_job(d_nodes, nodes * bs, bs, d_ctext, out);
  set_keys(j, salt, cid_key);
  HIP_TRY(launch_post(j, s, fused_posts()));
  return 0;
}

// Build the levels above a level whose refs sit in `cur` as `nodes` zero-
// padded index nodes (closed form of blob.go:165-206).
int build_up(Ctx *c, hipStream_t s, const Salts &salts, const uint8_t *cid_key,
             uint64_t bs, uint8_t *cur, uint64_t nodes, DevBuf *spare,
             uint8_t root_ref[64], uint64_t *posts) {
  const uint64_t bf = bs / 64;
  for (;;) {
    if (int e = c->d_ct.ensure(nodes * bs)) return e;
    if (nodes == 1) {
      // the root ref goes straight to pinned host memory (no D2H copy)
      if (int e = c->h_root.ensure(64)) return e;
      if (int e = post_level(s, salts.index, cid_key, cur, 1, bs, c->d_ct.u8(),
                             dense_refs(c->h_root.dptr())))
        return e;
      *posts += 1;
      HIP_TRY(stream_wait(s));
      memcpy(root_ref, c->h_root.p, 64);
      return fused_check(s);
    }
    const uint64_t m = (nodes + bf - 1) / bf;
    if (int e = level_prepare(*spare, nodes, m, bs, s)) return e;
    if (int e = post_level(s, salts.index, cid_key, cur, nodes, bs, c->d_ct.u8(),
                           node_refs(spare->u8(), bs)))
      return e;
    *posts += nodes;
    cur = spare->u8();
    nodes = m;
    spare = (spare == &c->d_lvl_a) ? &c->d_lvl_b : &c->d_lvl_a;
  }
}

}  // namespace host
}  // namespace glfsx

using namespace glfsx;
using namespace glfsx::host;

namespace {
int create_device_impl(uint64_t block_size, const uint8_t *salt,
                       const uint8_t *cid_key, const void *d_data,
                       uint64_t size, void *d_ctext, glfsx_root *out,
                       uint64_t *n_posts, void *stream) {
  if (!out || (size && !d_data)) return fail(GLFSX_E_ARG, "null argument");
  if (int e = check_block_size(block_size)) return e;
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  hipStream_t s = pick_stream(c, stream);
  Salts salts;
  if (int e = derive_salts(c, salt, &salts)) return e;
  const uint64_t bs = block_size, bf = bs / 64;
  const uint64_t n0 = (size + bs - 1) / bs;
  uint64_t posts = 0;
  if (n0 <= 1) {
    // n0 == 0: post(indexSalt, nil) (blob.go:187-189); n0 == 1: the only
    // data block's ref is the root (blob.go:190-193).
    if (int e = c->d_refs.ensure(64)) return e;
    if (int e = c->d_small.ensure(64)) return e;
    if (int e = c->h_root.ensure(64)) return e;
    PostJob j = single_job(n0 ? d_data : c->d_small.p, size, n0 ? d_ctext : nullptr,
                           c->h_root.dptr());  // written straight to the host
    set_keys(j, n0 ? salts.raw : salts.index, cid_key);
    HIP_TRY(launch_post(j, s, fused_posts()));
    HIP_TRY(stream_wait(s));
    memcpy(out->ref, c->h_root.p, 64);
    posts = 1;
  } else {
    const uint64_t n1 = (n0 + bf - 1) / bf;
    if (int e = level_prepare(c->d_lvl_a, n0, n1, bs, s)) return e;
    PostJob j = block_job(d_data, size, bs, d_ctext, node_refs(c->d_lvl_a.u8(), bs));
    set_keys(j, salts.raw, cid_key);
    HIP_TRY(launch_post(j, s, fused_posts()));
    posts = n0;
    if (int e = build_up(c, s, salts, cid_key, bs, c->d_lvl_a.u8(), n1,
                         &c->d_lvl_b, out->ref, &posts))
      return e;
  }
  out->size = size;
  out->block_size = bs;
  if (n_posts) *n_posts = posts;
  return 0;
}

int shard_device_impl(uint64_t block_size, const uint8_t *salt,
                      const uint8_t *cid_key, const void *d_range,
                      uint64_t size, uint64_t first_block, uint64_t nb,
                      void *d_ctext, uint8_t *level1_out, void *stream) {
  if (!level1_out || (nb && !d_range)) return fail(GLFSX_E_ARG, "null argument");
  if (int e = check_block_size(block_size)) return e;
  const uint64_t bs = block_size, bf = bs / 64;
  const uint64_t n0 = (size + bs - 1) / bs;
  if (first_block % bf)
    return fail(GLFSX_E_ARG, "shard start %llu not a multiple of bf=%llu",
                (unsigned long long)first_block, (unsigned long long)bf);
  if (nb == 0 || first_block + nb > n0 || n0 < 2)
    return fail(GLFSX_E_ARG, "bad shard range");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  hipStream_t s = pick_stream(c, stream);
  Salts salts;
  if (int e = derive_salts(c, salt, &salts)) return e;
  // the range's bytes: whole blocks, but for the blob's last block
  const uint64_t bytes = first_block + nb == n0 ? size - first_block * bs : nb * bs;
  const uint64_t m = (nb + bf - 1) / bf;
  if (int e = level_prepare(c->d_lvl_a, nb, m, bs, s)) return e;
  if (int e = c->d_ct.ensure(m * bs)) return e;
  if (int e = c->d_refs.ensure(m * 64)) return e;
  PostJob j = block_job(d_range, bytes, bs, d_ctext, node_refs(c->d_lvl_a.u8(), bs));
  set_keys(j, salts.raw, cid_key);
  HIP_TRY(launch_post(j, s, fused_posts()));
  if (int e = post_level(s, salts.index, cid_key, c->d_lvl_a.u8(), m, bs, c->d_ct.u8(),
                         dense_refs(c->d_refs.u8())))
    return e;
  HIP_TRY(hipMemcpyAsync(level1_out, c->d_refs.p, m * 64, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  return fused_check(s);
}

int root_from_level1_impl(uint64_t block_size, const uint8_t *salt,
                          const uint8_t *cid_key, const uint8_t *level1,
                          uint64_t n1, uint64_t size, glfsx_root *out) {
  if (!level1 || !out || n1 == 0) return fail(GLFSX_E_ARG, "null argument");
  if (int e = check_block_size(block_size)) return e;
  const uint64_t bs = block_size, bf = bs / 64;
  const uint64_t n0 = (size + bs - 1) / bs;
  if (n0 < 2 || (n0 + bf - 1) / bf != n1)
    return fail(GLFSX_E_ARG, "level-1 count %llu does not match size",
                (unsigned long long)n1);
  out->size = size;
  out->block_size = bs;
  if (n1 == 1) {
    memcpy(out->ref, level1, 64);
    return 0;
  }
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  Salts salts;
  if (int e = derive_salts(c, salt, &salts)) return e;
  const uint64_t m = (n1 + bf - 1) / bf;
  if (int e = level_prepare(c->d_lvl_a, n1, m, bs, c->stream)) return e;
  // scatter the gathered refs into zero-padded nodes (index.go:33-38)
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t cnt = std::min(bf, n1 - k * bf);
    HIP_TRY(hipMemcpyAsync(c->d_lvl_a.u8() + k * bs, level1 + k * bf * 64,
                           cnt * 64, hipMemcpyHostToDevice, c->stream));
  }
  uint64_t posts = 0;
  return build_up(c, c->stream, salts, cid_key, bs, c->d_lvl_a.u8(), m,
                  &c->d_lvl_b, out->ref, &posts);
}
}  // namespace

namespace {
// Persistent worker threads of glfsx_create_devices, one per (device,
// index): part k of a call runs on the worker of its device whose index
// counts the earlier parts on the same device.  A worker keeps its thread's
// context (stream, level buffers, scratch) across calls, so a call creates
// no streams or buffers once warm.  Calls are serialised (each takes every
// device it names).
struct PartWorker {
  int dev = 0;
  std::mutex mu;
  std::condition_variable cv;
  std::function<int()> fn;
  bool pending = false, done = false;
  int rc = 0;
  std::string err;
  float ms = -1.f;  // the last part's GPU time (HIP events on its stream)
  hipEvent_t ev[2] = {nullptr, nullptr};
  void loop() {
    set_thread_device(dev);
    for (;;) {
      std::function<int()> f;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return pending; });
        f = std::move(fn);
        pending = false;
      }
      // the part's work runs on this thread's context stream (the calls get
      // a null stream): events around it time the device's share of the call
      Ctx *c = nullptr;
      bool timed = ctx_get(&c) == 0;
      if (timed && !ev[0])
        timed = hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
      if (timed) timed = hipEventRecord(ev[0], c->stream) == hipSuccess;
      const int r = f();
      std::string e = r ? last_error_text() : std::string();
      float t = -1.f;
      if (timed && hipEventRecord(ev[1], c->stream) == hipSuccess &&
          hipEventSynchronize(ev[1]) == hipSuccess)
        (void)hipEventElapsedTime(&t, ev[0], ev[1]);
      {
        std::lock_guard<std::mutex> lk(mu);
        rc = r;
        err = std::move(e);
        ms = t;
        done = true;
      }
      cv.notify_all();
    }
  }
  void submit(std::function<int()> f) {
    std::lock_guard<std::mutex> lk(mu);
    fn = std::move(f);
    done = false;
    pending = true;
    cv.notify_all();
  }
  int wait(std::string *e, float *t) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done; });
    *e = err;
    *t = ms;
    return rc;
  }
};
std::mutex g_parts_mu;  // one glfsx_create_devices call at a time
std::vector<std::pair<std::pair<int, int>, PartWorker *>> g_part_workers;
// per part of the last glfsx_create_devices call: data-block pass GPU ms,
// then the levels above (on devs[0]) as one more entry
std::vector<float> g_parts_ms;

PartWorker *part_worker(int dev, int idx) {
  for (auto &x : g_part_workers)
    if (x.first == std::make_pair(dev, idx)) return x.second;
  auto *pw = new PartWorker();  // lives for the process, like its thread
  pw->dev = dev;
  std::thread([pw] { pw->loop(); }).detach();
  g_part_workers.push_back({{dev, idx}, pw});
  return pw;
}

// Run fns[k] on the worker of (devs[k], its index); the first failure (in
// part order) is returned with its text.
int run_parts(const int *devs, std::vector<std::function<int()>> &fns) {
  std::vector<PartWorker *> ws(fns.size());
  for (size_t k = 0; k < fns.size(); ++k) {
    int idx = 0;
    for (size_t i = 0; i < k; ++i) idx += devs[i] == devs[k];
    ws[k] = part_worker(devs[k], idx);
  }
  for (size_t k = 0; k < fns.size(); ++k) ws[k]->submit(std::move(fns[k]));
  int first = 0;
  std::string msg;
  for (size_t k = 0; k < fns.size(); ++k) {
    std::string e;
    float t = -1.f;
    const int rc = ws[k]->wait(&e, &t);
    g_parts_ms.push_back(t);
    if (rc && !first) {
      first = rc;
      msg = "part " + std::to_string(k) + " (device " + std::to_string(devs[k]) + "): " + e;
    }
  }
  return first ? fail(first, "%s", msg.c_str()) : 0;
}
}  // namespace

namespace {
// Shared setup of the device batch entry points: the argument checks, the
// calling thread's context and the job over the caller's buffers.
int batch_setup(const void *d_ptext, uint64_t total, uint64_t block_size, void *d_ctext,
                void *d_refs, Ctx **c, PostJob *j) {
  if (!d_refs || (total && !d_ptext)) return fail(GLFSX_E_ARG, "null argument");
  if (int e = check_batch_block_size(block_size)) return e;
  *j = block_job(d_ptext, total, block_size, d_ctext, dense_refs(d_refs));
  return ctx_get(c);
}
}  // namespace

int glfsx_post_batch_device(const uint8_t salt[32], const void *d_ptext,
                            uint64_t total, uint64_t block_size, void *d_ctext,
                            void *d_refs, const uint8_t *cid_key,
                            void *stream) {
  if (!salt) return fail(GLFSX_E_ARG, "null argument");
  Ctx *c;
  PostJob j;
  if (int e = batch_setup(d_ptext, total, block_size, d_ctext, d_refs, &c, &j)) return e;
  if (j.n == 0) return 0;
  set_keys(j, salt, cid_key);
  HIP_TRY(launch_post(j, pick_stream(c, stream), false));
  return 0;
}

int glfsx_dek_batch_device(const uint8_t salt[32], const void *d_ptext,
                           uint64_t total, uint64_t block_size, void *d_refs,
                           void *stream) {
  if (!salt) return fail(GLFSX_E_ARG, "null salt");
  Ctx *c;
  PostJob j;
  if (int e = batch_setup(d_ptext, total, block_size, nullptr, d_refs, &c, &j)) return e;
  set_keys(j, salt, nullptr);
  HIP_TRY(launch_keyed_hash(j, 32, pick_stream(c, stream)));
  return 0;
}

int glfsx_cid_batch_device(const void *d_ptext, uint64_t total,
                           uint64_t block_size, void *d_ctext, void *d_refs,
                           const uint8_t *cid_key, void *stream) {
  Ctx *c;
  PostJob j;
  if (int e = batch_setup(d_ptext, total, block_size, d_ctext, d_refs, &c, &j)) return e;
  set_cid_key(j, cid_key);
  HIP_TRY(launch_cid_pass(j, pick_stream(c, stream)));
  return 0;
}

int glfsx_post(const uint8_t salt[32], const void *ptext, uint64_t n,
               void *ctext_out, uint8_t *ref_out, const uint8_t *cid_key) {
  if (!salt || !ref_out || (n && !ptext)) return fail(GLFSX_E_ARG, "null argument");
  if (n > kMaxMsgLen)
    return fail(GLFSX_E_UNSUPPORTED, "message of %llu bytes above the kernels' limit %llu",
                (unsigned long long)n, (unsigned long long)kMaxMsgLen);
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  const uint8_t *p = static_cast<const uint8_t *>(ptext);
  if (n > kMaxMedLen)
    return post_staged_message(c->stream, {c->d_in, c->d_ct, c->d_refs}, salt, cid_key, p, n,
                               ctext_out, ref_out);
  const bool ct = ctext_out && n;
  if (int e = post_host_message(c->dev, {c->h_oin, c->h_oct, c->h_oref}, salt, cid_key, p, n, ct,
                                ref_out))
    return e;
  if (ct) memcpy(ctext_out, c->h_oct.p, n);
  return 0;
}

int glfsx_post_batch(const uint8_t salt[32], const void *ptext, uint64_t total,
                     uint64_t block_size, void *ctext_out, uint8_t *refs_out,
                     const uint8_t *cid_key) {
  if (!salt || !refs_out || (total && !ptext))
    return fail(GLFSX_E_ARG, "null argument");
  if (int e = check_batch_block_size(block_size)) return e;
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  const uint64_t n = (total + block_size - 1) / block_size;
  if (n == 0) return 0;
  // Stage in slabs of whole blocks (<= 256 MiB) to bound device memory.
  const uint64_t slab_blocks =
      std::max<uint64_t>(1, (256ull << 20) / block_size);
  for (uint64_t b0 = 0; b0 < n; b0 += slab_blocks) {
    const uint64_t nb = std::min(slab_blocks, n - b0);
    const uint64_t off = b0 * block_size;
    const uint64_t bytes = std::min<uint64_t>(nb * block_size, total - off);
    if (int e = c->d_in.ensure(bytes + 64)) return e;
    if (int e = c->d_ct.ensure(bytes + 64)) return e;
    if (int e = c->d_refs.ensure(nb * 64)) return e;
    HIP_TRY(hipMemcpyAsync(c->d_in.p, static_cast<const uint8_t *>(ptext) + off,
                           bytes, hipMemcpyHostToDevice, c->stream));
    PostJob j = block_job(c->d_in.p, bytes, block_size, c->d_ct.p, dense_refs(c->d_refs.p));
    set_keys(j, salt, cid_key);
    for (bool fused : {true, false}) {  // again with two launches if the fused one failed
      HIP_TRY(launch_post(j, c->stream, fused));
      HIP_TRY(hipMemcpyAsync(refs_out + 64 * b0, c->d_refs.p, nb * 64,
                             hipMemcpyDeviceToHost, c->stream));
      if (ctext_out)
        HIP_TRY(hipMemcpyAsync(static_cast<uint8_t *>(ctext_out) + off, c->d_ct.p,
                               bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(stream_wait(c->stream));
      if (!fused_errors_take(c->stream)) break;
    }
  }
  return 0;
}

int glfsx_create_device(uint64_t block_size, const uint8_t *salt,
                        const uint8_t *cid_key, const void *d_data,
                        uint64_t size, void *d_ctext, glfsx_root *out,
                        uint64_t *n_posts, void *stream) {
  return with_fused_retry([&] {
    return create_device_impl(block_size, salt, cid_key, d_data, size, d_ctext, out,
                              n_posts, stream);
  });
}

int glfsx_shard_device(uint64_t block_size, const uint8_t *salt,
                       const uint8_t *cid_key, const void *d_range,
                       uint64_t size, uint64_t first_block, uint64_t nb,
                       void *d_ctext, uint8_t *level1_out, void *stream) {
  return with_fused_retry([&] {
    return shard_device_impl(block_size, salt, cid_key, d_range, size, first_block, nb,
                             d_ctext, level1_out, stream);
  });
}

int glfsx_root_from_level1(uint64_t block_size, const uint8_t *salt,
                           const uint8_t *cid_key, const uint8_t *level1,
                           uint64_t n1, uint64_t size, glfsx_root *out) {
  return with_fused_retry([&] {
    return root_from_level1_impl(block_size, salt, cid_key, level1, n1, size, out);
  });
}

int glfsx_create_devices_ms(float *ms, int cap) {
  std::lock_guard<std::mutex> lk(g_parts_mu);
  const int n = int(g_parts_ms.size());
  for (int k = 0; k < std::min(n, cap); ++k) ms[k] = g_parts_ms[k];
  return n;
}

// Create over a blob whose bytes lie on several devices (in one
// process): part k = bytes of blocks [first_k, first_k + nb_k) on devs[k];
// each device posts its data blocks and level-1 nodes concurrently, the
// level-1 refs are gathered on the host and levels >= 2 posted on devs[0].
int glfsx_create_devices(uint64_t block_size, const uint8_t *salt,
                         const uint8_t *cid_key, int nparts, const int *devs,
                         const void *const *d_parts, const uint64_t *part_sizes,
                         void *const *d_ctexts, uint8_t *level1_out,
                         glfsx_root *out, uint64_t *n_posts) {
  if (!out || !devs || !d_parts || !part_sizes || nparts < 1 || nparts > 1024)
    return fail(GLFSX_E_ARG, "bad arguments");
  if (int e = check_block_size(block_size)) return e;
  const int ndev = glfsx_device_count();
  const uint64_t bs = block_size, bf = bs / 64, span = bs * bf;
  uint64_t size = 0;
  for (int k = 0; k < nparts; ++k) {
    if (devs[k] < 0 || devs[k] >= ndev)
      return fail(GLFSX_E_ARG, "device %d out of range (%d devices)", devs[k], ndev);
    if (part_sizes[k] && !d_parts[k]) return fail(GLFSX_E_ARG, "null part %d", k);
    if (k + 1 < nparts && (part_sizes[k] == 0 || part_sizes[k] % span))
      return fail(GLFSX_E_ARG,
                  "part %d: %llu bytes; every part but the last must be a positive "
                  "multiple of block_size * block_size/64 = %llu (whole level-1 nodes)",
                  k, (unsigned long long)part_sizes[k], (unsigned long long)span);
    size += part_sizes[k];
  }
  if (nparts > 1 && part_sizes[nparts - 1] == 0)
    return fail(GLFSX_E_ARG, "the last part is empty");
  std::lock_guard<std::mutex> lk(g_parts_mu);
  g_parts_ms.clear();
  const uint64_t n0 = (size + bs - 1) / bs;
  if (nparts == 1 || n0 <= bf) {  // one part: Create on its device
    std::vector<std::function<int()>> fns{[&] {
      return glfsx_create_device(bs, salt, cid_key, d_parts[0], size,
                                 d_ctexts ? d_ctexts[0] : nullptr, out, n_posts, nullptr);
    }};
    return run_parts(devs, fns);  // level1_out is not written
  }
  const uint64_t n1 = (n0 + bf - 1) / bf;
  std::vector<uint8_t> lvl1(n1 * 64);
  std::vector<std::function<int()>> fns;
  uint64_t first = 0;
  for (int k = 0; k < nparts; ++k) {
    const uint64_t nb = (part_sizes[k] + bs - 1) / bs;
    uint8_t *dst = lvl1.data() + (first / bf) * 64;
    void *ct = d_ctexts ? d_ctexts[k] : nullptr;
    const void *src = d_parts[k];
    fns.push_back([=] {
      return glfsx_shard_device(bs, salt, cid_key, src, size, first, nb, ct, dst, nullptr);
    });
    first += nb;
  }
  if (int e = run_parts(devs, fns)) return e;
  std::vector<std::function<int()>> top{[&] {
    return glfsx_root_from_level1(bs, salt, cid_key, lvl1.data(), n1, size, out);
  }};
  if (int e = run_parts(devs, top)) return e;
  if (level1_out) memcpy(level1_out, lvl1.data(), lvl1.size());
  if (n_posts) {
    uint64_t posts = n0 + n1;
    for (uint64_t r = n1; r > 1;) {
      r = (r + bf - 1) / bf;
      posts += r;
    }
    *n_posts = posts;
  }
  return 0;
}


namespace {
// glfsx_create of a blob of at most one block of <= kMaxMedLen bytes (a
// glfs.PostBlob of a small file, machine.go:64): its Writer would stage the
// bytes, post them as the tail block at Finish and return that block's ref
// as the root (blob.go:136-140, 190-193) -- or, for the empty blob, post
// the empty index node (blob.go:187-189).  The same single Post, without a
// Writer: the thread's pinned one-shot staging and one coalesced one-shot
// post (no writer pools, locks or streams per call).
int create_one_block(Ctx *c, uint64_t bs, const uint8_t *salt, const uint8_t *cid_key,
                     const void *data, uint64_t size, glfsx_post_fn post, void *post_ctx,
                     glfsx_root *out) {
  Salts salts;
  if (int e = derive_salts(c, salt, &salts)) return e;
  out->size = size;
  out->block_size = bs;
  return post_host_message(c->dev, {c->h_oin, c->h_oct, c->h_oref},
                           size ? salts.raw : salts.index, cid_key,
                           static_cast<const uint8_t *>(data), size, post != nullptr, out->ref,
                           post, post_ctx, size ? 0 : 1);
}
}  // namespace

int glfsx_create(uint64_t block_size, uint64_t store_max, const uint8_t *salt,
                 const uint8_t *cid_key, const void *data, uint64_t size,
                 glfsx_post_fn post, void *post_ctx, glfsx_root *out) {
  const uint64_t bs = block_size ? block_size : store_max;  // blob.go:86-89
  if (out && (size == 0 || data) && bs <= store_max && bs >= GLFSX_MIN_BLOCK_SIZE &&
      bs <= kMaxMsgLen && size <= bs && size <= kMaxMedLen) {
    Ctx *c;
    if (int e = ctx_get(&c)) return e;
    return create_one_block(c, bs, salt, cid_key, data, size, post, post_ctx, out);
  }
  int err = 0;
  glfsx_writer *w =
      glfsx_writer_new(block_size, store_max, salt, cid_key, post, post_ctx, &err);
  if (!w) return err;
  int e = glfsx_writer_write(w, data, size);
  if (!e) e = glfsx_writer_finish(w, out);
  glfsx_writer_free(w);
  return e;
}
