// read.cpp -- the read side: batched decrypt and verified read ("open") from
// device or host memory.
#include "host.h"

using namespace glfsx;
using namespace glfsx::host;

namespace {

// What a slab of the host pipeline runs: a plain decrypt (open == nullptr),
// or the verified read with these keys (ptext nullable then).
struct SlabOpen {
  OpenJob keys;          // salt, cid_key, salted, cid_keyed
  uint32_t *status_out;  // nullable
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
    const uint64_t last_len = sl.bytes - (sl.nb - 1) * block_size;
    if (open) {
      OpenJob job = open->keys;
      job.ctext = sl.d_in.u8();
      job.ptext = ptext ? sl.d_out.u8() : nullptr;
      job.n = sl.nb;
      job.bs = block_size;
      job.last_len = last_len;
      job.refs = sl.d_refs.u8();
      job.status = static_cast<uint32_t *>(sl.d_status.p);
      HIP_TRY(launch_open(job, c->stream));
    } else {
      HIP_TRY(launch_decrypt(sl.d_in.u8(), sl.d_out.u8(), sl.nb, block_size, last_len,
                             sl.d_refs.u8(), c->stream));
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

void open_keys(OpenJob &j, const uint8_t *salt, const uint8_t *cid_key) {
  j.salted = salt != nullptr;
  if (salt) words_from_key(j.salt, salt);
  set_cid_key(j, cid_key);
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
  OpenJob job{};
  open_keys(job, salt, cid_key);
  job.ctext = static_cast<const uint8_t *>(d_ctext);
  job.ptext = static_cast<uint8_t *>(d_ptext);
  job.n = (total + block_size - 1) / block_size;
  job.bs = block_size;
  job.last_len = total - (job.n - 1) * block_size;
  job.refs = static_cast<const uint8_t *>(d_refs);
  job.status = d_status;
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
  SlabOpen op{};
  open_keys(op.keys, salt, cid_key);
  op.status_out = status_out;
  if (int e = slab_pipeline(c, ctext, total, block_size, refs, ptext, &op)) return e;
  if (n_bad) *n_bad = op.n_bad;
  if (op.n_bad == 0) return 0;
  return fail(GLFSX_E_CORRUPT, "block %llu of %llu failed its %s check%s (%llu bad in all)",
              (unsigned long long)op.first_bad,
              (unsigned long long)((total + block_size - 1) / block_size),
              op.first_status == 3 ? "CID and DEK" : op.first_status == 1 ? "CID" : "DEK",
              op.first_status == 3 ? "s" : "", (unsigned long long)op.n_bad);
}

int glfsx_set_open_route(int route) { return set_open_route(route); }

}  // extern "C"
