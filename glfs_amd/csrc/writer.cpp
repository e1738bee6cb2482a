// writer.cpp -- the Writer (bigblob/blob.go:71-206) and every glfsx_writer_*
// entry point.
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <unistd.h>

#include "writer.h"

using namespace glfsx;
using namespace glfsx::host;

namespace {

const uint8_t *cidk(const glfsx_writer *w) {
  return w->has_cid_key ? w->cid_key : nullptr;
}

// Post one message from host memory (ref.go:98 post + sink), synchronously,
// with the writer's own staging: messages of at most kMaxMedLen bytes as a
// one-shot post (data read in place when it lies 16-B aligned in the pinned
// buffer `pin`), larger ones and device memory (dev_src: written on the
// upload stream) on the writer's hash stream.
int post_one(glfsx_writer *w, int kind, const uint8_t salt[32],
             const uint8_t *data, uint64_t n, uint8_t ref[64],
             bool dev_src = false, const PinBuf *pin = nullptr,
             uint64_t present = ~0ull) {
  OneBuf &o = w->one;
  if (!dev_src && n <= kMaxMedLen)
    return post_host_message(w->dev, {o.h_in, o.h_ct, o.h_ref}, salt, cidk(w), data, n,
                             w->post != nullptr, ref, w->post, w->post_ctx, kind, pin, present);
  if (int e = o.h_ct.ensure(n + 64)) return e;
  if (int e = o.h_ref.ensure(64)) return e;
  if (dev_src)
    if (int e = w->ev_out.ensure()) return e;
  if (int e = post_staged_message(w->ws, {o.d_in, o.d_ct, o.d_ref}, salt, cidk(w), data, n,
                                  o.h_ct.p, o.h_ref.p, dev_src ? hipEvent_t(w->ev_out) : nullptr,
                                  w->s_up))
    return e;
  memcpy(ref, o.h_ref.p, 64);
  return deliver(w->post, w->post_ctx, kind, ref, o.h_ct.p, n);
}

// The index stack's post (writer_book.h; blob.go:165-206): an index node of
// len bytes, its refs in the first `present` of them, or the empty blob's
// node (len 0).
auto node_poster(glfsx_writer *w) {
  return [w](const uint8_t *refs, uint64_t present, uint64_t len, uint8_t out[64]) -> int {
    if (len <= kMaxMedLen)  // the kernel reads the rest as zero
      return post_one(w, 1, w->salts.index, refs, len, out, false, nullptr, present);
    w->node.assign(len, 0);
    memcpy(w->node.data(), refs, present);
    return post_one(w, 1, w->salts.index, w->node.data(), len, out);
  };
}

// The Writer's half of postBuf (blob.go:152-163) for a block the GPU has
// posted: addRef, then the size.
int account_block(glfsx_writer *w, const uint8_t ref[64], uint64_t len) {
  if (int e = w->index.add(ref, node_poster(w))) return e;
  w->size += len;
  return 0;
}

// The same with its Post: deliver -> addRef -> size.
int replay_block(glfsx_writer *w, const uint8_t ref[64], const void *ctext, uint64_t len) {
  if (int e = deliver(w->post, w->post_ctx, 0, ref, ctext, len)) return e;
  return account_block(w, ref, len);
}

// A one-launch split post on the hash stream failed (fused_check): the
// error word cannot tell which batch's launch it was, so every batch still
// in flight is hashed again with two launches per post, in order.
int rehash_inflight(glfsx_writer *w) {
  for (const WLane &L : w->lanes) {
    DevScope d(L.dev);
    HIP_TRY(hipStreamSynchronize(L.ws));
    HIP_TRY(hipStreamSynchronize(L.s_down));
    (void)fused_errors_take(L.ws);
  }
  for (WSlot &x : w->slot) {
    if (!x.busy) continue;
    const WLane &L = w->lanes[x.lane];
    DevScope d(L.dev);
    HIP_TRY(launch_post(x.job, L.ws, false));
    HIP_TRY(hipMemcpyAsync(x.h_refs.p, x.d_refs.p, x.nblk * 64, hipMemcpyDeviceToHost, L.ws));
    if (w->post)
      HIP_TRY(hipMemcpyAsync(x.h_ct.p, x.d_ct.p, x.nblk * w->bs, hipMemcpyDeviceToHost,
                             L.ws));
  }
  for (const WLane &L : w->lanes) {
    DevScope d(L.dev);
    HIP_TRY(stream_wait(L.ws));
  }
  return 0;
}

// Wait for an in-flight batch and replay postBuf (blob.go:152-163) for each
// of its blocks, in order.
int complete(glfsx_writer *w, WSlot &sl) {
  if (!sl.busy) return 0;
  HIP_TRY(hipEventSynchronize(sl.done));
  bool failed;
  {
    const WLane &L = w->lanes[sl.lane];
    DevScope d(L.dev);
    failed = fused_errors_take(L.ws) != 0;
  }
  // the replay's single posts (index nodes: post_one on the writer's hash
  // stream and staging) run on the home device, whichever lane's device the
  // caller (submit) has current
  DevScope home(w->dev);
  if (failed)
    if (int e = rehash_inflight(w)) return e;
  sl.busy = false;
  for (uint64_t b = 0; b < sl.nblk; ++b)
    if (int e = replay_block(w, sl.h_refs.u8() + 64 * b, sl.h_ct.u8() + b * w->bs, w->bs))
      return e;
  return 0;
}

// Enqueue the current slot's complete blocks (H2D, DEK + ChaCha/CID kernels,
// D2H of refs and ctext), finish the oldest batch still in flight if it
// holds the next slot, and switch slots, carrying the partial block over.
int submit(glfsx_writer *w) {
  const uint64_t full = w->fill.full, partial = w->fill.partial;
  if (full == 0) return 0;
  WSlot &sl = w->slot[w->cur];
  const int next = (w->cur + 1) % int(w->slot.size());
  WSlot &nx = w->slot[next];
  const WLane &L = w->lanes[sl.lane];
  DevScope dscope(L.dev);
  const uint64_t nbytes = full * w->bs;
  if (int e = sl.d_in.ensure(nbytes)) return e;
  if (int e = sl.d_ct.ensure(nbytes)) return e;
  if (int e = sl.d_refs.ensure(full * 64)) return e;
  if (w->post)
    if (int e = sl.h_ct.ensure(nbytes + 64)) return e;
  if (int e = sl.h_refs.ensure(full * 64)) return e;
  for (Event *ev : {&sl.up, &sl.hashed, &sl.done})
    if (int e = ev->ensure()) return e;
  if (!sl.on_dev)  // device-written bytes are already in d_in (s_up order)
    HIP_TRY(hipMemcpyAsync(sl.d_in.p, sl.h_in.p, nbytes, hipMemcpyHostToDevice, L.s_up));
  HIP_TRY(hipEventRecord(sl.up, L.s_up));
  HIP_TRY(hipStreamWaitEvent(L.ws, sl.up, 0));
  sl.job = block_job(sl.d_in.u8(), nbytes, w->bs, sl.d_ct.u8(), dense_refs(sl.d_refs.u8()));
  set_keys(sl.job, w->salts.raw, cidk(w));
  HIP_TRY(launch_post(sl.job, L.ws, fused_posts()));
  HIP_TRY(hipEventRecord(sl.hashed, L.ws));
  HIP_TRY(hipStreamWaitEvent(L.s_down, sl.hashed, 0));
  HIP_TRY(hipMemcpyAsync(sl.h_refs.p, sl.d_refs.p, full * 64,
                         hipMemcpyDeviceToHost, L.s_down));
  if (w->post)
    HIP_TRY(hipMemcpyAsync(sl.h_ct.p, sl.d_ct.p, nbytes, hipMemcpyDeviceToHost,
                           L.s_down));
  HIP_TRY(hipEventRecord(sl.done, L.s_down));
  sl.nblk = full;
  sl.seq = ++w->seq;
  sl.busy = true;
  // `nx` is the oldest batch in flight (submitted nslots-1 batches ago):
  // completing it keeps Posts in order
  if (int e = complete(w, nx)) return e;
  if (sl.on_dev) {  // carry the partial block over on the device (one lane)
    if (int e = nx.d_in.ensure(w->fill.cap() + 64)) return e;
    if (partial)
      HIP_TRY(hipMemcpyAsync(nx.d_in.p, sl.d_in.u8() + nbytes, partial,
                             hipMemcpyDeviceToDevice, L.s_up));
    nx.on_dev = true;
  } else {
    if (int e = nx.h_in.grow(std::max<uint64_t>(partial, 1), 0)) return e;
    if (partial) memcpy(nx.h_in.u8(), sl.h_in.u8() + nbytes, partial);
    nx.on_dev = false;
  }
  w->cur = next;
  w->fill.carry();
  return 0;
}

// Move the current slot's staged bytes between host and device staging.
int slot_to_device(glfsx_writer *w) {
  WSlot &sl = w->slot[w->cur];
  if (sl.on_dev) return 0;
  const uint64_t used = w->fill.used();
  if (int e = sl.d_in.ensure(w->fill.cap() + 64)) return e;
  if (used)
    HIP_TRY(hipMemcpyAsync(sl.d_in.p, sl.h_in.p, used, hipMemcpyHostToDevice, w->s_up));
  sl.on_dev = true;
  return 0;
}

int slot_to_host(glfsx_writer *w) {
  WSlot &sl = w->slot[w->cur];
  if (!sl.on_dev) return 0;
  const uint64_t used = w->fill.used();
  if (int e = sl.h_in.grow(std::max<uint64_t>(used, 1), 0)) return e;
  if (used) {
    HIP_TRY(hipMemcpyAsync(sl.h_in.p, sl.d_in.p, used, hipMemcpyDeviceToHost, w->s_up));
    HIP_TRY(hipStreamSynchronize(w->s_up));
  }
  sl.on_dev = false;
  return 0;
}

// Append n device bytes, ordered after everything already on the upload
// stream (blob.go:120-133 block bookkeeping, as glfsx_writer_write).
int write_dev(glfsx_writer *w, const uint8_t *p, uint64_t n) {
  while (n) {
    if (int e = slot_to_device(w)) return e;
    WSlot &sl = w->slot[w->cur];
    const uint64_t take = std::min<uint64_t>(w->fill.room(), n);
    HIP_TRY(hipMemcpyAsync(sl.d_in.u8() + w->fill.used(), p, take, hipMemcpyDeviceToDevice,
                           w->s_up));
    p += take;
    n -= take;
    if (w->fill.add(take))
      if (int e = submit(w)) return e;
  }
  return 0;
}
}  // namespace

glfsx_writer *glfsx_writer_new(uint64_t block_size, uint64_t store_max,
                               const uint8_t *salt, const uint8_t *cid_key,
                               glfsx_post_fn post, void *post_ctx, int *err) {
  int dummy;
  if (!err) err = &dummy;
  uint64_t bs = store_max;  // blob.go:86
  if (block_size > 0) bs = block_size;
  if (bs > store_max) {  // blob.go:90-92
    *err = fail(GLFSX_E_BLOCKSIZE_GT_MAX, "blockSize %llu > maxSize %llu",
                (unsigned long long)bs, (unsigned long long)store_max);
    return nullptr;
  }
  if (int e = check_block_size(bs)) {  // blob.go:93-95
    *err = e;
    return nullptr;
  }
  Ctx *c;
  if (int e = ctx_get(&c)) {
    *err = e;
    return nullptr;
  }
  auto *w = new glfsx_writer();
  w->dev = c->dev;
  w->bs = w->fill.bs = w->index.node_len = bs;
  w->index.bf = bs / 64;  // blob.go:107
  if (int e = derive_salts(c, salt, &w->salts)) {
    delete w;
    *err = e;
    return nullptr;
  }
  if (cid_key) {
    memcpy(w->cid_key, cid_key, 32);
    w->has_cid_key = true;
  }
  w->post = post;
  w->post_ctx = post_ctx;
  uint64_t batch_mib = 64;
  if (const char *e = getenv("GLFSX_BATCH_MIB")) batch_mib = std::max(1ull, strtoull(e, nullptr, 10));
  if (const char *e = getenv("GLFSX_SLOTS")) w->nslots = std::min(kMaxSlots, std::max(2, atoi(e)));
  w->fill.batch_blocks = std::max<uint64_t>(1, (batch_mib << 20) / bs);
  w->slot.resize(w->nslots);
  for (WSlot &x : w->slot) take_slot(x, w->dev, 0);
  w->one = one_pool().take(w->dev);
  w->one.dev = w->dev;
  if (!take_streams(w->home, w->dev)) {
    glfsx_writer_free(w);
    *err = fail(GLFSX_E_DEVICE, "hipStreamCreate failed");
    return nullptr;
  }
  w->ws = w->home.hash;
  w->s_up = w->home.up;
  w->s_down = w->home.down;
  w->lanes.push_back(WLane{w->dev, w->ws, w->s_up, w->s_down});
  *err = 0;
  return w;
}

int glfsx_writer_set_devices(glfsx_writer *w, const int *devs, int ndev) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  if (!devs || ndev < 1 || ndev > 64) return fail(GLFSX_E_ARG, "need 1..64 devices");
  if (w->seq || w->fill.used() || w->size || w->sticky || w->ev_in)
    return fail(GLFSX_E_ARG, "glfsx_writer_set_devices: the writer has already been written to");
  const int n = glfsx_device_count();
  for (int k = 0; k < ndev; ++k)
    if (devs[k] < 0 || devs[k] >= n)
      return fail(GLFSX_E_ARG, "device %d out of range (%d devices)", devs[k], n);
  std::vector<WLane> lanes(ndev);
  for (int k = 0; k < ndev; ++k) {
    lanes[k].dev = devs[k];
    if (devs[k] == w->dev) {  // the home streams
      lanes[k] = WLane{w->dev, w->ws, w->s_up, w->s_down};
      continue;
    }
    // lanes on one device share its streams: a device's copy engines and
    // hardware queues are the resource (GPU_MAX_HW_QUEUES = 4 per process;
    // more streams on one device alias queues and serialise each other:
    // 4 GiB through lanes [0, 0] 40.8 -> 29 GiB/s with separate streams)
    bool shared = false;
    for (int i = 0; i < k && !shared; ++i)
      if (lanes[i].dev == devs[k]) {
        lanes[k] = WLane{devs[k], lanes[i].ws, lanes[i].s_up, lanes[i].s_down};
        shared = true;
      }
    if (shared) continue;
    Streams &s = lanes[k].own;
    if (!take_streams(s, devs[k])) {
      for (int i = 0; i < k; ++i) stream_pool().give(std::move(lanes[i].own));
      return fail(GLFSX_E_DEVICE, "hipStreamCreate on device %d failed", devs[k]);
    }
    lanes[k].ws = s.hash;
    lanes[k].s_up = s.up;
    lanes[k].s_down = s.down;
  }
  for (WLane &L : w->lanes) stream_pool().give(std::move(L.own));
  for (WSlot &x : w->slot) give_slot(x);
  w->lanes = std::move(lanes);
  w->slot = std::vector<WSlot>(size_t(w->nslots) * ndev);
  for (size_t i = 0; i < w->slot.size(); ++i)
    take_slot(w->slot[i], w->lanes[i % ndev].dev, int(i % ndev));
  w->cur = 0;
  return 0;
}

namespace {
// Every writer entry point runs on the writer's device (the calling thread
// may have another one current) and keeps the error text on the writer.
struct WriterCall {
  glfsx_writer *w;
  explicit WriterCall(glfsx_writer *w_) : w(w_) {
    int cur = -1;  // a Write of 32 KiB (io.Copy) costs ~1.7 us: skip the set
    if (hipGetDevice(&cur) != hipSuccess || cur != w->dev) (void)hipSetDevice(w->dev);
  }
  int done(int rc) {
    if (rc) w->err = last_error_text();
    return rc;
  }
  // The writer is dead after its first error: that error again, or 0.
  int dead() { return w->sticky ? done(fail(w->sticky, "%s", w->err.c_str())) : 0; }
  // e is the writer's first error.
  int stick(int e) { return done(w->sticky = e); }
};

// Drain: submit the staged complete blocks and deliver the Posts of every
// batch in flight, oldest first.
int complete_all(glfsx_writer *w) {
  for (;;) {
    WSlot *o = nullptr;
    for (auto &sl : w->slot)
      if (sl.busy && (!o || sl.seq < o->seq)) o = &sl;
    if (!o) return 0;
    if (int e = complete(w, *o)) return e;
  }
}

int drain(glfsx_writer *w) {
  if (int e = submit(w)) return e;
  return complete_all(w);
}

// A few complete blocks (<= kFewBlocks) staged on the host -- with the tail
// at Finish, or without it in a strict Write -- go out as one coalesced
// one-shot post (a request per block, the kernels reading the pinned
// staging in place) instead of a batch through the three-stream pipeline:
// a PostBlob of a few MiB, or a strict Write that completes a block, is one
// launch pair and one wait.  Posts and addRef replay in block order
// (blob.go:152-163), after every older batch's.  Without the tail, the
// partial block's bytes move to the front of the staging.
constexpr uint64_t kFewBlocks = 8;
int post_few(glfsx_writer *w, bool tail, bool *done) {
  *done = false;
  WSlot &sl = w->slot[w->cur];
  FillCursor &f = w->fill;
  if (sl.on_dev || f.full == 0 || f.full > kFewBlocks ||
      w->bs > kMaxMedLen || (w->bs & 15) || !sl.h_in.dp)
    return 0;
  if (int e = complete_all(w)) return e;
  const uint64_t k = f.full + (tail && f.partial ? 1 : 0);
  OneBuf &o = w->one;
  if (w->post)
    if (int e = o.h_ct.ensure(f.used() + 64)) return e;
  if (int e = o.h_ref.ensure(64 * k)) return e;
  std::vector<OneReq> reqs(k);
  std::vector<OneReq *> rp(k);
  for (uint64_t b = 0; b < k; ++b) {
    const uint64_t off = b * w->bs;
    OneDesc &d = reqs[b].d;
    d.src = sl.h_in.dptr() + off;
    d.ctext = w->post ? o.h_ct.dptr() + off : nullptr;
    d.ref = o.h_ref.dptr() + 64 * b;
    d.len = uint32_t(b < f.full ? w->bs : f.partial);
    d.present = d.len;
    set_keys(d, w->salts.raw, cidk(w));
    rp[b] = &reqs[b];
  }
  if (int e = one_post_many(w->dev, rp.data(), k)) return e;
  // refs out first: an index node posted by addRef reuses the single-post
  // staging (its ctext lands on block 0's, already delivered)
  std::vector<uint8_t> refs(o.h_ref.u8(), o.h_ref.u8() + 64 * k);
  for (uint64_t b = 0; b < k; ++b)
    if (int e = replay_block(w, &refs[64 * b], o.h_ct.u8() + b * w->bs, reqs[b].d.len))
      return e;
  if (tail)
    f.partial = 0;
  else if (f.partial)
    memmove(sl.h_in.u8(), sl.h_in.u8() + f.full * w->bs, f.partial);
  f.carry();
  *done = true;
  return 0;
}

// blob.go:120-133 error timing: deliver the Posts of every block completed
// so far before the Write returns.
int drain_strict(glfsx_writer *w) {
  bool few = false;
  if (int e = post_few(w, false, &few)) return e;
  return few ? complete_all(w) : drain(w);
}
}  // namespace

// blob.go:120-133: a block is complete exactly when buffered + incoming
// reaches bs; complete blocks are hashed a batch at a time.
int glfsx_writer_write(glfsx_writer *w, const void *data, size_t n) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  if (n && !data) return call.done(fail(GLFSX_E_ARG, "null data"));
  const uint8_t *p = static_cast<const uint8_t *>(data);
  while (n) {
    if (int e = slot_to_host(w)) return call.stick(e);
    WSlot &sl = w->slot[w->cur];
    const uint64_t used = w->fill.used();
    const uint64_t take = std::min<uint64_t>(w->fill.room(), n);
    if (int e = sl.h_in.grow(used + take, used)) return call.stick(e);
    par_memcpy(sl.h_in.u8() + used, p, take, w->lanes[sl.lane].dev);
    p += take;
    n -= take;
    if (w->fill.add(take))
      if (int e = submit(w)) return call.stick(e);
  }
  if (w->strict)
    if (int e = drain_strict(w)) return call.stick(e);
  return 0;
}

int glfsx_writer_reserve(glfsx_writer *w, void **buf, uint64_t *cap) {
  if (!w || !buf || !cap) return fail(GLFSX_E_ARG, "null argument");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  if (int e = slot_to_host(w)) return call.stick(e);
  WSlot &sl = w->slot[w->cur];
  const uint64_t used = w->fill.used();
  if (int e = sl.h_in.grow(w->fill.cap(), used)) return call.stick(e);
  *buf = sl.h_in.u8() + used;
  *cap = w->fill.room();  // >= 1: a full batch is submitted as soon as it fills
  w->reserved = w->fill.room();
  return 0;
}

int glfsx_writer_commit(glfsx_writer *w, uint64_t n) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  if (n > w->reserved)
    return call.done(fail(GLFSX_E_ARG, "commit of %llu bytes, %llu reserved",
                          (unsigned long long)n, (unsigned long long)w->reserved));
  w->reserved = 0;
  if (w->fill.add(n))
    if (int e = submit(w)) return call.stick(e);
  if (w->strict && n)
    if (int e = drain_strict(w)) return call.stick(e);
  return 0;
}

namespace {
// Reader threads per batch of glfsx_writer_read_at (GLFSX_READ_THREADS;
// capped by the copy pool: the GPU box's share is 16 cores).
unsigned read_threads() {
  static const unsigned v = [] {
    const char *e = getenv("GLFSX_READ_THREADS");
    return e ? std::max(1u, unsigned(strtoul(e, nullptr, 10))) : 16u;
  }();
  return v;
}

int64_t pread_fn(void *ctx, void *buf, uint64_t len, uint64_t off) {
  const int fd = int(reinterpret_cast<intptr_t>(ctx));
  for (;;) {
    const ssize_t r = pread(fd, buf, size_t(std::min<uint64_t>(len, 1ull << 30)), off_t(off));
    if (r >= 0) return r;
    if (errno != EINTR) return -int64_t(errno);
  }
}
}  // namespace

int glfsx_writer_read_at(glfsx_writer *w, glfsx_read_at_fn read_at, void *ctx,
                         uint64_t offset, uint64_t n, uint64_t *got) {
  if (got) *got = 0;
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  if (!read_at) return fail(GLFSX_E_ARG, "null reader");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  if (w->reserved) return call.done(fail(GLFSX_E_ARG, "staging lent out by glfsx_writer_reserve"));
  uint64_t total = 0;
  int rc = 0;
  while (total < n) {
    if (int e = slot_to_host(w)) return call.stick(e);
    WSlot &sl = w->slot[w->cur];  // free: submit completed it before moving on
    const uint64_t used = w->fill.used();
    if (int e = sl.h_in.grow(w->fill.cap(), used)) return call.stick(e);
    const uint64_t want = std::min(w->fill.room(), n - total);
    const int64_t r = par_read_at(read_at, ctx, sl.h_in.u8() + used, want, offset + total,
                                  read_threads(), w->lanes[sl.lane].dev);
    if (r < 0) {
      rc = fail(GLFSX_E_IO, "read of %llu bytes at input offset %llu failed (%lld)",
                (unsigned long long)want, (unsigned long long)(offset + total), (long long)r);
      break;
    }
    total += uint64_t(r);
    if (w->fill.add(uint64_t(r)))
      if (int e = submit(w)) return call.stick(e);
    if (uint64_t(r) < want) break;  // the end of the input
  }
  if (got) *got = total;
  if (w->strict && total)
    if (int e = drain_strict(w)) return call.stick(e);
  return call.done(rc);
}

int glfsx_writer_read_fd(glfsx_writer *w, int fd, uint64_t offset, uint64_t n,
                         uint64_t *got) {
  if (fd < 0) {
    if (got) *got = 0;
    return fail(GLFSX_E_ARG, "bad file descriptor %d", fd);
  }
  return glfsx_writer_read_at(w, pread_fn, reinterpret_cast<void *>(intptr_t(fd)), offset, n,
                              got);
}

int glfsx_writer_copy(glfsx_writer *w, const void *data, uint64_t n, uint64_t piece) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  if (piece == 0) return fail(GLFSX_E_ARG, "piece of 0 bytes");
  const uint8_t *p = static_cast<const uint8_t *>(data);
  for (uint64_t off = 0; off < n; off += piece)
    if (int e = glfsx_writer_write(w, p + off, std::min(piece, n - off))) return e;
  return 0;
}

int glfsx_writer_flush(glfsx_writer *w) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  if (int e = drain(w)) return call.stick(e);
  return 0;
}

int glfsx_writer_write_device(glfsx_writer *w, const void *d_data, size_t n,
                              void *stream) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  if (n && !d_data) return call.done(fail(GLFSX_E_ARG, "null data"));
  if (n == 0) return 0;
  if (w->lanes.size() != 1)
    return call.done(fail(GLFSX_E_UNSUPPORTED, "device input needs a one-device writer"));
  hipStream_t cs = static_cast<hipStream_t>(stream);
  auto go = [&]() -> int {
    if (int e = w->ev_in.ensure()) return e;
    if (int e = w->ev_out.ensure()) return e;
    if (cs) {  // the bytes are ready once the caller's stream gets here
      HIP_TRY(hipEventRecord(w->ev_in, cs));
      HIP_TRY(hipStreamWaitEvent(w->s_up, w->ev_in, 0));
    }
    if (int e = write_dev(w, static_cast<const uint8_t *>(d_data), n)) return e;
    // the caller may reuse d_data once its stream passes this point
    HIP_TRY(hipEventRecord(w->ev_out, w->s_up));
    if (cs)
      HIP_TRY(hipStreamWaitEvent(cs, w->ev_out, 0));
    else
      HIP_TRY(hipEventSynchronize(w->ev_out));
    if (w->strict)
      if (int e = drain(w)) return e;
    return 0;
  };
  if (int e = go()) return call.stick(e);
  return 0;
}

int glfsx_writer_write_ctext_blocks(glfsx_writer *w, const void *const *blocks,
                                    uint64_t nblocks, uint64_t total, uint64_t block_size,
                                    const uint8_t *refs) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  if (total == 0) return 0;
  if (!blocks || !refs) return call.done(fail(GLFSX_E_ARG, "null argument"));
  if (w->lanes.size() != 1)
    return call.done(fail(GLFSX_E_UNSUPPORTED, "device input needs a one-device writer"));
  if (block_size == 0 || block_size % 64)
    return call.done(fail(GLFSX_E_UNSUPPORTED, "decrypt needs block_size %% 64 == 0"));
  const uint64_t nb = (total + block_size - 1) / block_size;
  if (nblocks != nb)
    return call.done(fail(GLFSX_E_ARG, "%llu blocks given, %llu bytes need %llu",
                          (unsigned long long)nblocks, (unsigned long long)total,
                          (unsigned long long)nb));
  auto go = [&]() -> int {
    if (int e = w->ev_in.ensure()) return e;
    if (int e = w->ev_out.ensure()) return e;
    if (w->cx.dev < 0) {
      w->cx = ctext_pool().take(w->dev);
      w->cx.dev = w->dev;
    }
    CtextBuf &X = w->cx;
    for (Event &ev : X.ev)
      if (int e = ev.ensure()) return e;
    const uint64_t slab = std::max<uint64_t>(1, (64ull << 20) / block_size);
    for (PinBuf &hb : X.h)
      if (int e = hb.ensure(slab * block_size + 64 * slab)) return e;
    if (int e = X.d_ctx.ensure(slab * block_size + 64)) return e;
    if (int e = X.d_ptx.ensure(slab * block_size + 64)) return e;
    if (int e = X.d_rfx.ensure(64 * slab)) return e;
    // Three stages overlap: the copy threads gather slab i + 1 from the
    // store's memory into host buffer (i + 1) & 1 while this thread uploads
    // slab i, decrypts it into the Writer's staging and hands it on (the
    // Writer's own pipeline hashes it and brings the ctext back); buffer
    // (i + 1) & 1 is gathered into once slab i - 1's upload from it is done.
    // Uploads, decrypts and the Writer's copies are in order on s_up (the
    // device temporaries are reused in stream order).  A -DGLFSX_CONCAT_TRACE=1
    // build (tools/build_variant.sh) prints each slab's host timeline to
    // stderr.
    const int dev = w->lanes[0].dev;
    const uint64_t ns = (nb + slab - 1) / slab;
    std::atomic<int> left[2];
    left[0].store(0);
    left[1].store(0);
    struct Settle {  // no gather may still write a buffer, or read the
      std::atomic<int> *l;  // caller's blocks, once this call returns
      ~Settle() {
        gather_wait(&l[0]);
        gather_wait(&l[1]);
      }
    } settle{left};
#if GLFSX_CONCAT_TRACE
    constexpr bool trace = true;
#else
    constexpr bool trace = false;
#endif
    const auto tz = std::chrono::steady_clock::now();
    auto us = [&] {
      return double(std::chrono::duration_cast<std::chrono::nanoseconds>(
                        std::chrono::steady_clock::now() - tz).count()) * 1e-3;
    };
    std::vector<double> tr;
    auto start = [&](uint64_t i) {
      const uint64_t b0 = i * slab, k = std::min(slab, nb - b0);
      const uint64_t bytes = std::min<uint64_t>(k * block_size, total - b0 * block_size);
      gather_start(&left[i & 1], X.h[i & 1].u8(), blocks + b0, k, block_size,
                   bytes - (k - 1) * block_size, dev);
    };
    start(0);
    for (uint64_t i = 0; i < ns; ++i) {
      const uint64_t b0 = i * slab, k = std::min(slab, nb - b0);
      const uint64_t bytes = std::min<uint64_t>(k * block_size, total - b0 * block_size);
      PinBuf &hb = X.h[i & 1];
      const double t_in = trace ? us() : 0;
      gather_wait(&left[i & 1]);
      const double t_gathered = trace ? us() : 0;
      memcpy(hb.u8() + bytes, refs + 64 * b0, 64 * k);
      HIP_TRY(hipMemcpyAsync(X.d_ctx.p, hb.p, bytes, hipMemcpyHostToDevice, w->s_up));
      HIP_TRY(hipMemcpyAsync(X.d_rfx.p, hb.u8() + bytes, 64 * k, hipMemcpyHostToDevice,
                             w->s_up));
      HIP_TRY(hipEventRecord(X.ev[i & 1], w->s_up));
      double t_next = t_gathered;
      if (i + 1 < ns) {
        if (i >= 1) HIP_TRY(hipEventSynchronize(X.ev[(i + 1) & 1]));
        t_next = trace ? us() : 0;
        start(i + 1);
      }
      HIP_TRY(launch_decrypt(X.d_ctx.u8(), X.d_ptx.u8(), k, block_size,
                             bytes - (k - 1) * block_size, X.d_rfx.u8(), w->s_up));
      if (int e = write_dev(w, X.d_ptx.u8(), bytes)) return e;
      if (trace) tr.insert(tr.end(), {t_in, t_gathered, t_next, us()});
    }
    if (trace) {
      for (size_t x = 0; x + 3 < tr.size(); x += 4)
        fprintf(stderr,
                "concat slab %zu: wait-gather %.1f..%.1f us, next gather from %.1f, "
                "handed on %.1f\n",
                x / 4, tr[x], tr[x + 1], tr[x + 2], tr[x + 3]);
    }
    HIP_TRY(hipStreamSynchronize(w->s_up));
    if (w->strict)
      if (int e = drain(w)) return e;
    return 0;
  };
  if (int e = go()) return call.stick(e);
  return 0;
}

int glfsx_writer_write_ctext(glfsx_writer *w, const void *ctext, uint64_t total,
                             uint64_t block_size, const uint8_t *refs) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  if (total == 0 || !ctext || block_size == 0 || block_size % 64) {
    // (the same checks and errors; nothing to split into blocks)
    const void *one = ctext;
    return glfsx_writer_write_ctext_blocks(w, ctext ? &one : nullptr, 0, total, block_size,
                                           refs);
  }
  const uint64_t nb = (total + block_size - 1) / block_size;
  std::vector<const void *> blocks(nb);
  for (uint64_t j = 0; j < nb; ++j)
    blocks[j] = static_cast<const uint8_t *>(ctext) + j * block_size;
  return glfsx_writer_write_ctext_blocks(w, blocks.data(), nb, total, block_size, refs);
}

int glfsx_writer_set_strict(glfsx_writer *w, int strict) {
  if (!w) return fail(GLFSX_E_ARG, "null writer");
  w->strict = strict != 0;
  return 0;
}

const char *glfsx_writer_error(const glfsx_writer *w) {
  return w ? w->err.c_str() : "null writer";
}

int glfsx_writer_finish(glfsx_writer *w, glfsx_root *out) {
  if (!w || !out) return fail(GLFSX_E_ARG, "null argument");
  WriterCall call(w);
  if (int e = call.dead()) return e;
  bool few = false;
  if (int e = post_few(w, true, &few)) return call.stick(e);
  if (!few)
    if (int e = drain(w)) return call.stick(e);
  if (const uint64_t tail = w->fill.partial) {  // blob.go:136-140: the tail block, never padded
    uint8_t ref[64];
    const WSlot &sl = w->slot[w->cur];
    if (int e = post_one(w, 0, w->salts.raw, sl.on_dev ? sl.d_in.u8() : sl.h_in.u8(), tail,
                         ref, sl.on_dev, &sl.h_in))  // (post_one delivers the Post)
      return call.stick(e);
    if (int e = account_block(w, ref, tail)) return call.stick(e);
    w->fill.partial = 0;
  }
  uint8_t root[64];
  int e = w->index.finish(root, node_poster(w));
  if (e == IndexStack::kShouldNotHappen) e = fail(GLFSX_E_ARG, "should not happen");
  if (e) return call.stick(e);
  memcpy(out->ref, root, 64);
  out->size = w->size;
  out->block_size = w->bs;
  return 0;
}

void glfsx_writer_free(glfsx_writer *w) {
  if (!w) return;
  (void)hipSetDevice(w->dev);
  // a writer that never submitted a batch nor took device input, and did
  // not fail, has nothing in flight (its single posts waited for themselves)
  if (w->seq || w->ev_in || w->sticky) {
    for (hipStream_t st : {w->s_up, w->ws, w->s_down})
      if (st) (void)hipStreamSynchronize(st);
    for (const WLane &L : w->lanes)
      if (L.own) {
        DevScope d(L.dev);
        for (hipStream_t st : {L.s_up, L.ws, L.s_down}) (void)hipStreamSynchronize(st);
      }
  }
  // a pool destroys what it does not keep; what stays in *w is moved from
  for (auto &sl : w->slot) give_slot(sl);
  for (WLane &L : w->lanes) stream_pool().give(std::move(L.own));
  one_pool().give(std::move(w->one));
  stream_pool().give(std::move(w->home));
  ctext_pool().give(std::move(w->cx));  // (its streams are drained above: ev_in is set)
  delete w;
}

