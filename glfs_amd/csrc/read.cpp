// read.cpp -- the read side: batched decrypt and verified read ("open") from
// device or host memory.
#include <cstdio>

#include "host.h"
#include "ragged_groups.h"

using namespace glfsx;
using namespace glfsx::host;

namespace {

// What a slab of the host pipeline runs: a plain decrypt (open == nullptr),
// or the verified read with these keys (ptext nullable then).
struct SlabOpen {
  const uint8_t *salt, *cid_key;  // as open_keys takes them
  uint32_t *status_out;           // nullable
  uint64_t n_bad = 0, first_bad = 0;
  uint32_t first_status = 0;
};

// Batched getF from host memory: slabs of whole blocks through two slots and
// three streams (upload k+1 / decrypt k / download k-1 overlap).  With `open`
// each slab's status words come down behind its plaintext.
int slab_pipeline(Ctx *c, const void *ctext, uint64_t total, uint64_t block_size,
                  const uint8_t *refs, void *ptext, SlabOpen *open) {
  const uint64_t n = (total + block_size - 1) / block_size;
  const uint64_t slab_blocks = std::max<uint64_t>(1, (64ull << 20) / block_size);
  struct Slot {
    DevBuf d_in, d_out, d_refs, d_status;
    PinBuf h_in, h_out;
    Event up, done;
    uint64_t b0 = 0, nb = 0, bytes = 0, st_off = 0;
    bool busy = false;
  };
  // (never deleted, like the thread's contexts: see ~Ctx)
  static thread_local Slot *const slots = new Slot[2];
  static thread_local hipStream_t s_up = nullptr, s_dn = nullptr;
  if (!s_up) {
    HIP_TRY(hipStreamCreateWithFlags(&s_up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s_dn, hipStreamNonBlocking));
  }
  auto finish = [&](Slot &sl) -> int {
    if (!sl.busy) return 0;
    sl.busy = false;
    HIP_TRY(hipEventSynchronize(sl.done));
    if (ptext)
      par_memcpy(static_cast<uint8_t *>(ptext) + sl.b0 * block_size, sl.h_out.u8(), sl.bytes);
    if (open) {
      const uint32_t *st = reinterpret_cast<const uint32_t *>(sl.h_out.u8() + sl.st_off);
      if (open->status_out) memcpy(open->status_out + sl.b0, st, 4 * sl.nb);
      for (uint64_t i = 0; i < sl.nb; ++i)
        if (st[i] && open->n_bad++ == 0) {
          open->first_bad = sl.b0 + i;
          open->first_status = st[i];
        }
    }
    return 0;
  };
  // a failure leaves no slot marked busy for the thread's next call
  auto bail = [&](int e) {
    for (int i = 0; i < 2; ++i) {
      if (slots[i].busy) (void)hipEventSynchronize(slots[i].done);
      slots[i].busy = false;
    }
    return e;
  };
  int k = 0;
  for (uint64_t b0 = 0; b0 < n; b0 += slab_blocks, k ^= 1) {
    Slot &sl = slots[k];
    if (int e = finish(sl)) return bail(e);
    sl.b0 = b0;
    sl.nb = std::min(slab_blocks, n - b0);
    sl.bytes = std::min<uint64_t>(sl.nb * block_size, total - b0 * block_size);
    sl.st_off = ptext ? (sl.bytes + 15) & ~15ull : 0;
    if (int e = sl.d_in.ensure(sl.bytes + 64)) return bail(e);
    if (ptext)
      if (int e = sl.d_out.ensure(sl.bytes + 64)) return bail(e);
    if (int e = sl.d_refs.ensure(64 * sl.nb)) return bail(e);
    if (open)
      if (int e = sl.d_status.ensure(4 * sl.nb)) return bail(e);
    if (int e = sl.h_in.ensure(sl.bytes + 64 * sl.nb)) return bail(e);
    if (int e = sl.h_out.ensure(sl.st_off + (open ? 4 * sl.nb : 0) + 16)) return bail(e);
    if (int e = sl.up.ensure()) return bail(e);
    if (int e = sl.done.ensure()) return bail(e);
    par_memcpy(sl.h_in.u8(), static_cast<const uint8_t *>(ctext) + b0 * block_size, sl.bytes);
    memcpy(sl.h_in.u8() + sl.bytes, refs + 64 * b0, 64 * sl.nb);
    HIP_TRY(hipMemcpyAsync(sl.d_in.p, sl.h_in.p, sl.bytes, hipMemcpyHostToDevice, s_up));
    HIP_TRY(hipMemcpyAsync(sl.d_refs.p, sl.h_in.u8() + sl.bytes, 64 * sl.nb,
                           hipMemcpyHostToDevice, s_up));
    HIP_TRY(hipEventRecord(sl.up, s_up));
    HIP_TRY(hipStreamWaitEvent(c->stream, sl.up, 0));
    if (open) {
      OpenJob job = open_job(sl.d_in.p, ptext ? sl.d_out.p : nullptr, sl.bytes, block_size,
                             sl.d_refs.p, static_cast<uint32_t *>(sl.d_status.p));
      open_keys(job, open->salt, open->cid_key);
      HIP_TRY(launch_open(job, c->stream));
    } else {
      HIP_TRY(launch_decrypt(sl.d_in.u8(), sl.d_out.u8(), sl.nb, block_size,
                             sl.bytes - (sl.nb - 1) * block_size, sl.d_refs.u8(), c->stream));
    }
    HIP_TRY(hipEventRecord(sl.up, c->stream));
    HIP_TRY(hipStreamWaitEvent(s_dn, sl.up, 0));
    if (ptext)
      HIP_TRY(hipMemcpyAsync(sl.h_out.p, sl.d_out.p, sl.bytes, hipMemcpyDeviceToHost, s_dn));
    if (open)
      HIP_TRY(hipMemcpyAsync(sl.h_out.u8() + sl.st_off, sl.d_status.p, 4 * sl.nb,
                             hipMemcpyDeviceToHost, s_dn));
    HIP_TRY(hipEventRecord(sl.done, s_dn));
    sl.busy = true;
  }
  for (int i = 0; i < 2; ++i, k ^= 1)
    if (int e = finish(slots[k])) return bail(e);
  return 0;
}

int open_check_args(const void *ctext, const void *refs, const void *status, bool need_status,
                    uint64_t block_size) {
  if (!ctext || !refs || (need_status && !status)) return fail(GLFSX_E_ARG, "null argument");
  if ((reinterpret_cast<uintptr_t>(refs) | reinterpret_cast<uintptr_t>(status)) & 3)
    return fail(GLFSX_E_ARG, "refs and status must be 4-byte aligned");
  if (block_size == 0 || block_size % 64 || block_size > kMaxMsgLen)
    return fail(GLFSX_E_UNSUPPORTED,
                "open needs block_size %% 64 == 0 and at most %llu, got %llu",
                (unsigned long long)kMaxMsgLen, (unsigned long long)block_size);
  return 0;
}

}  // namespace

extern "C" {

int glfsx_decrypt_batch_device(const void *d_ctext, uint64_t total,
                               uint64_t block_size, const void *d_refs,
                               void *d_ptext, void *stream) {
  if (total == 0) return 0;
  if (!d_ctext || !d_refs || !d_ptext) return fail(GLFSX_E_ARG, "null argument");
  if (block_size == 0 || block_size % 64)
    return fail(GLFSX_E_UNSUPPORTED, "decrypt needs block_size %% 64 == 0");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  const uint64_t n = (total + block_size - 1) / block_size;
  HIP_TRY(launch_decrypt(static_cast<const uint8_t *>(d_ctext),
                         static_cast<uint8_t *>(d_ptext), n, block_size,
                         total - (n - 1) * block_size,
                         static_cast<const uint8_t *>(d_refs), pick_stream(c, stream)));
  return 0;
}

int glfsx_decrypt_batch(const void *ctext, uint64_t total, uint64_t block_size,
                        const uint8_t *refs, void *ptext) {
  if (total == 0) return 0;
  if (!ctext || !refs || !ptext) return fail(GLFSX_E_ARG, "null argument");
  if (block_size == 0 || block_size % 64)
    return fail(GLFSX_E_UNSUPPORTED, "decrypt needs block_size %% 64 == 0");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  return slab_pipeline(c, ctext, total, block_size, refs, ptext, nullptr);
}

int glfsx_open_batch_device(const uint8_t *salt, const uint8_t *cid_key,
                            const void *d_ctext, uint64_t total, uint64_t block_size,
                            const void *d_refs, void *d_ptext, uint32_t *d_status,
                            void *stream) {
  if (total == 0) return 0;
  if (int e = open_check_args(d_ctext, d_refs, d_status, true, block_size)) return e;
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  OpenJob job = open_job(d_ctext, d_ptext, total, block_size, d_refs, d_status);
  open_keys(job, salt, cid_key);
  HIP_TRY(launch_open(job, pick_stream(c, stream)));
  return 0;
}

int glfsx_open_batch(const uint8_t *salt, const uint8_t *cid_key, const void *ctext,
                     uint64_t total, uint64_t block_size, const uint8_t *refs,
                     void *ptext, uint32_t *status_out, uint64_t *n_bad) {
  if (n_bad) *n_bad = 0;
  if (total == 0) return 0;
  if (int e = open_check_args(ctext, refs, status_out, false, block_size)) return e;
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  SlabOpen op{salt, cid_key, status_out};
  if (int e = slab_pipeline(c, ctext, total, block_size, refs, ptext, &op)) return e;
  if (n_bad) *n_bad = op.n_bad;
  if (op.n_bad == 0) return 0;
  return corrupt_fail("block", op.first_bad, (total + block_size - 1) / block_size,
                      op.first_status, op.n_bad);
}

int glfsx_set_open_route(int route) { return set_open_route(route); }

int glfsx_open(const uint8_t *salt, const uint8_t *cid_key, const uint8_t ref[64],
               const void *ctext, uint64_t n, void *ptext, uint32_t *status_out) {
  if (!ref || (n && !ctext)) return fail(GLFSX_E_ARG, "null argument");
  if (n > kMaxMsgLen)
    return fail(GLFSX_E_UNSUPPORTED, "message of %llu bytes above the kernels' limit %llu",
                (unsigned long long)n, (unsigned long long)kMaxMsgLen);
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  uint32_t status = 0;
  // route 1 (tests, measurements): every size through device staging
  const int route = set_open_route(-1);
  if (n <= kMaxOneLen && route != 1) {
    if (int e = open_host_message(c->dev, {c->h_oin, c->h_oct, c->h_oref}, salt, cid_key, ref,
                                  static_cast<const uint8_t *>(ctext), n, ptext, &status))
      return e;
  } else {
    // one upload, launch_open over one block, plaintext and status behind it,
    // one wait; the ref and the status word share d_refs
    const uint64_t bs = std::max<uint64_t>(64, (n + 63) & ~63ull);
    if (int e = c->d_in.ensure(bs + 64)) return e;
    if (ptext)
      if (int e = c->d_ct.ensure(bs + 64)) return e;
    if (int e = c->d_refs.ensure(128)) return e;
    if (n) HIP_TRY(hipMemcpyAsync(c->d_in.p, ctext, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_refs.p, ref, 64, hipMemcpyHostToDevice, c->stream));
    OpenJob job = open_job(c->d_in.p, ptext ? c->d_ct.p : nullptr, n, bs, c->d_refs.p,
                           reinterpret_cast<uint32_t *>(c->d_refs.u8() + 64));
    open_keys(job, salt, cid_key);
    HIP_TRY(launch_open(job, c->stream));
    if (ptext && n)
      HIP_TRY(hipMemcpyAsync(ptext, c->d_ct.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&status, job.status, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(stream_wait(c->stream));
  }
  if (status_out) *status_out = status;
  if (!status) return 0;
  char hex[65];
  for (int i = 0; i < 32; ++i) snprintf(hex + 2 * i, 3, "%02x", ref[i]);
  return fail(GLFSX_E_CORRUPT, "blob %s %s", hex, failed_checks(status));
}

int glfsx_open_ragged_device(const uint8_t *salt, const uint8_t *cid_key,
                             const void *d_ctext, const uint64_t *d_offsets,
                             const uint64_t *d_lengths, uint64_t n, uint64_t max_len,
                             const void *d_refs, void *d_ptext, uint32_t *d_status,
                             void *stream) {
  if (!d_ctext || !d_refs || !d_status) return fail(GLFSX_E_ARG, "null argument");
  if ((reinterpret_cast<uintptr_t>(d_refs) | reinterpret_cast<uintptr_t>(d_status)) & 3)
    return fail(GLFSX_E_ARG, "refs and status must be 4-byte aligned");
  if (max_len > kMaxRaggedLen)
    return fail(GLFSX_E_UNSUPPORTED, "max_len %llu above the ragged open's %llu",
                (unsigned long long)max_len, (unsigned long long)kMaxRaggedLen);
  if (n == 0) return 0;
  if (!d_offsets || !d_lengths) return fail(GLFSX_E_ARG, "null argument");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  OpenRaggedJob job =
      open_ragged_job(d_ctext, d_ptext, d_offsets, d_lengths, n, max_len, d_refs, d_status);
  open_keys(job, salt, cid_key);
  HIP_TRY(launch_open_ragged(job, pick_stream(c, stream)));
  return 0;
}

int glfsx_open_blobs(const uint8_t *salt, const uint8_t *cid_key, const void *ctext,
                     const uint64_t *offsets, const uint64_t *lengths, uint64_t n,
                     const uint8_t *refs, void *ptext, uint32_t *status_out,
                     uint64_t *n_bad) {
  if (n_bad) *n_bad = 0;
  if (n == 0) return 0;
  if (!ctext || !refs || !offsets || !lengths) return fail(GLFSX_E_ARG, "null argument");
  uint64_t max_len = 0;
  for (uint64_t i = 0; i < n; ++i) max_len = std::max(max_len, lengths[i]);
  if (max_len > kMaxRaggedLen)
    return fail(GLFSX_E_UNSUPPORTED, "a message of %llu bytes is above the ragged open's %llu",
                (unsigned long long)max_len, (unsigned long long)kMaxRaggedLen);
  std::vector<RaggedGroup> groups;
  std::vector<uint64_t> soff;
  ragged_groups(lengths, n, kRaggedGroupBytes, &groups, &soff);
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  const uint8_t *src = static_cast<const uint8_t *>(ctext);
  uint8_t *dst = static_cast<uint8_t *>(ptext);
  // The groups one after the other through the thread's first pooled slot:
  // gathered into its pinned staging by the copy threads, opened in place on
  // the device, the plaintext scattered back from the pinned staging.
  Ctx::BlobSlot &g = c->bslot[0];
  uint64_t bad = 0, first_bad = 0;
  uint32_t first_status = 0;
  auto run = [&](const RaggedGroup &grp) -> int {
    const uint64_t m = grp.i1 - grp.i0;
    if (int e = g.h_in.ensure(grp.bytes + 64)) return e;
    if (int e = g.d_in.ensure(grp.bytes + 64)) return e;
    if (int e = g.h_meta.ensure(20 * m)) return e;  // offsets, lengths, then status
    if (int e = g.d_meta.ensure(20 * m)) return e;
    if (int e = g.h_refs.ensure(64 * m)) return e;
    if (int e = g.d_refs.ensure(64 * m)) return e;
    uint64_t *lo = reinterpret_cast<uint64_t *>(g.h_meta.p), *ll = lo + m;
    memcpy(lo, &soff[grp.i0], 8 * m);
    memcpy(ll, lengths + grp.i0, 8 * m);
    // gather, copying each run of messages contiguous on both sides at once
    ragged_runs(offsets + grp.i0, lo, ll, m, [&](uint64_t s, uint64_t d, uint64_t len) {
      par_memcpy(g.h_in.u8() + d, src + s, len);
    });
    memcpy(g.h_refs.p, refs + 64 * grp.i0, 64 * m);
    if (grp.bytes)
      HIP_TRY(hipMemcpyAsync(g.d_in.p, g.h_in.p, grp.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(g.d_meta.p, g.h_meta.p, 16 * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(g.d_refs.p, g.h_refs.p, 64 * m, hipMemcpyHostToDevice, c->stream));
    const uint64_t *d_lo = reinterpret_cast<const uint64_t *>(g.d_meta.p);
    OpenRaggedJob job =  // in place: staged messages are disjoint
        open_ragged_job(g.d_in.p, ptext ? g.d_in.p : nullptr, d_lo, d_lo + m, m, max_len,
                        g.d_refs.p, reinterpret_cast<uint32_t *>(g.d_meta.u8() + 16 * m));
    open_keys(job, salt, cid_key);
    HIP_TRY(launch_open_ragged(job, c->stream));
    if (ptext && grp.bytes)
      HIP_TRY(hipMemcpyAsync(g.h_in.p, g.d_in.p, grp.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(g.h_meta.u8() + 16 * m, job.status, 4 * m, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(stream_wait(c->stream));
    const uint32_t *st = reinterpret_cast<const uint32_t *>(g.h_meta.u8() + 16 * m);
    if (status_out) memcpy(status_out + grp.i0, st, 4 * m);
    for (uint64_t j = 0; j < m; ++j)
      if (st[j] && bad++ == 0) {
        first_bad = grp.i0 + j;
        first_status = st[j];
      }
    if (ptext)  // scatter, by the same runs
      ragged_runs(offsets + grp.i0, lo, ll, m, [&](uint64_t s, uint64_t d, uint64_t len) {
        par_memcpy(dst + s, g.h_in.u8() + d, len);
      });
    return 0;
  };
  for (const RaggedGroup &grp : groups)
    if (int e = run(grp)) {
      (void)hipStreamSynchronize(c->stream);  // nothing may still use the staging
      return e;
    }
  if (n_bad) *n_bad = bad;
  if (bad == 0) return 0;
  return corrupt_fail("message", first_bad, n, first_status, bad);
}

}  // extern "C"
