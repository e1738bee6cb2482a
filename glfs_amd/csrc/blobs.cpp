// blobs.cpp -- many blobs in one call (post_blobs) and a tree with its
// blobs (post_tree), from host or device memory.
#include "host.h"
#include "ragged_groups.h"

using namespace glfsx;
using namespace glfsx::host;

int glfsx_post_blobs_device(uint64_t block_size, const uint8_t *salt,
                            const uint8_t *cid_key, const void *d_data,
                            const uint64_t *d_offsets, const uint64_t *d_lengths,
                            uint64_t n, uint64_t max_len, void *d_ctext,
                            void *d_roots, void *stream) {
  if (n == 0) return 0;
  if (!d_data || !d_offsets || !d_lengths || !d_roots)
    return fail(GLFSX_E_ARG, "null argument");
  if (int e = check_block_size(block_size)) return e;
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  hipStream_t s = pick_stream(c, stream);
  Salts salts;
  if (int e = derive_salts(c, salt, &salts)) return e;
  // blobs of <= min(16 KiB, block_size): one lane each (k_small skips the
  // others; a blob longer than its block size has several blocks)
  const uint64_t small_max = small_max_for(block_size);
  SmallJob j = small_job(d_data, d_ctext, d_offsets, d_lengths, n, max_len, small_max, d_roots);
  set_keys(j, salts, cid_key);
  HIP_TRY(launch_post_small(j, s));
  if (max_len <= small_max) return 0;
  // larger single-block blobs (the caller said some may exceed 16 KiB), up
  // to 16 MiB: the ragged post, whatever their number and mix of lengths
  // (the root is post(rawSalt, blob), blob.go:190-193)
  const uint64_t rag_max = std::min(block_size, kMaxRaggedLen);
  if (rag_max > small_max) {  // (not at block sizes of 16 KiB and less)
    RaggedJob rj = ragged_job(d_data, d_ctext, d_offsets, d_lengths, n, small_max,
                              std::min(max_len, rag_max), d_roots);
    set_keys(rj, salts.raw, cid_key);
    HIP_TRY(launch_post_ragged(rj, s));
  }
  if (max_len <= rag_max) return 0;
  // what is left: find them, then a whole Create each (several blocks) or
  // one post (a single block above 16 MiB)
  std::vector<uint64_t> offs(n), lens(n);
  HIP_TRY(hipMemcpyAsync(offs.data(), d_offsets, 8 * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(lens.data(), d_lengths, 8 * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  for (uint64_t i = 0; i < n; ++i) {
    if (lens[i] <= rag_max) continue;  // posted above
    const uint8_t *src = static_cast<const uint8_t *>(d_data) + offs[i];
    uint8_t *ct = d_ctext ? static_cast<uint8_t *>(d_ctext) + offs[i] : nullptr;
    uint8_t *ref = static_cast<uint8_t *>(d_roots) + 64 * i;
    if (lens[i] <= block_size) {
      PostJob pj = single_job(src, lens[i], ct, ref);
      set_keys(pj, salts.raw, cid_key);
      HIP_TRY(launch_post(pj, s, fused_posts()));
    } else {
      glfsx_root r;
      if (int e = glfsx_create_device(block_size, salt, cid_key, src, lens[i], ct, &r,
                                      nullptr, s))
        return e;
      HIP_TRY(hipMemcpyAsync(ref, r.ref, 64, hipMemcpyHostToDevice, s));
      HIP_TRY(stream_wait(s));  // r lives on this frame
    }
  }
  return 0;
}

int glfsx_post_ragged_device(const uint8_t salt[32], const uint8_t *cid_key,
                             const void *d_data, const uint64_t *d_offsets,
                             const uint64_t *d_lengths, uint64_t n, uint64_t max_len,
                             void *d_ctext, void *d_refs, void *stream) {
  if (n == 0) return 0;
  if (!salt || !d_data || !d_offsets || !d_lengths || !d_refs)
    return fail(GLFSX_E_ARG, "null argument");
  if (max_len > kMaxRaggedLen)
    return fail(GLFSX_E_UNSUPPORTED, "max_len %llu above the ragged post's %llu",
                (unsigned long long)max_len, (unsigned long long)kMaxRaggedLen);
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  hipStream_t s = pick_stream(c, stream);
  RaggedJob rj = ragged_job(d_data, d_ctext, d_offsets, d_lengths, n, kRaggedAll, max_len, d_refs);
  set_keys(rj, salt, cid_key);
  HIP_TRY(launch_post_ragged(rj, s));
  return 0;
}

namespace {
// A store sink that keeps every Post (large blobs of glfsx_post_blobs are
// created first and their Posts replayed in call order).
struct CapturedPost {
  int kind;
  uint8_t ref[64];
  std::vector<uint8_t> ctext;
};
int capture_post(void *ctx, int kind, const uint8_t *ref, const void *ctext,
                 uint64_t len) {
  auto *v = static_cast<std::vector<CapturedPost> *>(ctx);
  v->emplace_back();
  CapturedPost &p = v->back();
  p.kind = kind;
  memcpy(p.ref, ref, 64);
  p.ctext.assign(static_cast<const uint8_t *>(ctext),
                 static_cast<const uint8_t *>(ctext) + len);
  return 0;
}
int replay(const std::vector<CapturedPost> &posts, glfsx_post_fn post, void *post_ctx) {
  for (const CapturedPost &p : posts)
    if (int e = deliver(post, post_ctx, p.kind, p.ref, p.ctext.data(), p.ctext.size())) return e;
  return 0;
}

// glfsx_post_blobs' single-block blobs of at most med_max bytes, pipelined
// from host memory: the blobs are taken in index order in groups whose bytes
// fit a 64 MiB slot; each group's bytes are packed into pinned staging (runs
// of blobs contiguous in `data` copied at once, by the copy pool; a blob
// above small_max starts on a 64-B boundary of the slot), uploaded on one
// stream, hashed on the context's stream -- one lane per blob of at most
// small_max bytes (launch_post_small), the longer ones by the ragged post
// (launch_post_ragged) over the same slot -- and their roots and ctext
// downloaded on a third, while the next group is packed -- three slots in
// flight, so the host copy, both PCIe directions and the kernels overlap.  A
// group's Posts are delivered when its slot is reused or at the end, in blob
// order, the larger blobs' captured Posts in their places: exactly n
// sequential PostBlob calls' order.
constexpr uint64_t kGroupBytes = 64ull << 20;

// Where a blob of len bytes goes in a slot filled up to o.
inline uint64_t slot_offset(uint64_t o, uint64_t len, uint64_t small_max) {
  return len > small_max ? (o + 63) & ~uint64_t(63) : o;
}

int complete_group(Ctx::BlobSlot &g, const uint64_t *lengths, uint64_t med_max,
                   const std::vector<std::vector<CapturedPost>> &big, glfsx_post_fn post,
                   void *post_ctx, uint8_t *roots_out) {
  if (!g.busy) return 0;
  HIP_TRY(hipEventSynchronize(g.done));
  g.busy = false;
  for (uint64_t i = g.i0; i < g.i1; ++i) {
    if (lengths[i] <= med_max) {
      const uint8_t *ref = g.h_refs.u8() + 64 * (i - g.i0);
      memcpy(roots_out + 64 * i, ref, 64);
      // a single-block blob's single Post: a data block, or the empty blob's
      // index node (blob.go:187-189)
      if (int e = deliver(post, post_ctx, lengths[i] ? 0 : 1, roots_out + 64 * i,
                          g.h_ct.u8() + g.loff[i - g.i0], lengths[i]))
        return e;
    } else if (int e = replay(big[i], post, post_ctx)) {
      return e;
    }
  }
  return 0;
}

int post_small_groups(Ctx *c, uint64_t bs, const uint8_t *salt, const uint8_t *cid_key,
                      const uint8_t *data, const uint64_t *offsets, const uint64_t *lengths,
                      uint64_t n, uint64_t small_max, uint64_t med_max,
                      const std::vector<std::vector<CapturedPost>> &big, glfsx_post_fn post,
                      void *post_ctx, uint8_t *roots_out) {
  Salts salts;
  if (int e = derive_salts(c, salt, &salts)) return e;
  if (!c->s_up) HIP_TRY(hipStreamCreateWithFlags(&c->s_up, hipStreamNonBlocking));
  if (!c->s_down) HIP_TRY(hipStreamCreateWithFlags(&c->s_down, hipStreamNonBlocking));
  for (auto &g : c->bslot)
    for (Event *ev : {&g.done, &g.up, &g.hashed})
      if (int e = ev->ensure()) return e;
  // on any failure, nothing may still be writing the slots' pinned staging
  auto drain = [&] {
    for (hipStream_t st : {c->s_up, c->stream, c->s_down}) (void)hipStreamSynchronize(st);
    for (auto &g : c->bslot) g.busy = false;
  };
  int k = 0;
  uint64_t i = 0;
  while (i < n) {
    Ctx::BlobSlot &g = c->bslot[k];
    k = (k + 1) % 3;
    if (int e = complete_group(g, lengths, med_max, big, post, post_ctx, roots_out)) {
      drain();
      return e;
    }
    // the group: blobs [i, i1) whose packed bytes fit kGroupBytes (a single
    // blob always fits: they are <= kMaxMedLen)
    uint64_t i1 = i, bytes = 0, max_len = 0, max_med = 0;
    while (i1 < n) {
      const uint64_t len = lengths[i1] <= med_max ? lengths[i1] : 0;
      const uint64_t end = slot_offset(bytes, len, small_max) + len;
      if (i1 > i && end > kGroupBytes) break;
      bytes = end;
      if (len <= small_max) max_len = std::max(max_len, len);
      else max_med = std::max(max_med, len);
      ++i1;
    }
    const uint64_t m = i1 - i;
    auto run = [&]() -> int {
      if (int e = g.h_in.ensure(bytes + 64)) return e;
      if (int e = g.d_in.ensure(bytes + 64)) return e;
      if (int e = g.d_ct.ensure(bytes + 64)) return e;
      if (post)
        if (int e = g.h_ct.ensure(bytes + 64)) return e;
      if (int e = g.h_meta.ensure(16 * m)) return e;
      if (int e = g.d_meta.ensure(16 * m)) return e;
      if (int e = g.h_refs.ensure(64 * m)) return e;
      if (int e = g.d_refs.ensure(64 * m)) return e;
      g.loff.assign(m, 0);
      uint64_t *lo = reinterpret_cast<uint64_t *>(g.h_meta.p), *ll = lo + m;
      // pack, copying each run of blobs that are contiguous in `data` at once
      uint64_t o = 0;
      for (uint64_t j = 0; j < m; ++j) {
        const uint64_t len = lengths[i + j];
        const bool here = len <= med_max;
        if (here) o = slot_offset(o, len, small_max);
        lo[j] = here ? o : 0;
        ll[j] = here ? len : kRaggedAbsent;  // skipped by both posts
        g.loff[j] = lo[j];
        if (here) o += len;
      }
      ragged_runs(offsets + i, lo, ll, m, [&](uint64_t src, uint64_t dst, uint64_t len) {
        par_memcpy(g.h_in.u8() + dst, data + src, len);
      });
      if (bytes) HIP_TRY(hipMemcpyAsync(g.d_in.p, g.h_in.p, bytes, hipMemcpyHostToDevice, c->s_up));
      HIP_TRY(hipMemcpyAsync(g.d_meta.p, g.h_meta.p, 16 * m, hipMemcpyHostToDevice, c->s_up));
      HIP_TRY(hipEventRecord(g.up, c->s_up));
      HIP_TRY(hipStreamWaitEvent(c->stream, g.up, 0));
      const uint64_t *d_lo = reinterpret_cast<const uint64_t *>(g.d_meta.p);
      SmallJob j = small_job(g.d_in.p, g.d_ct.p, d_lo, d_lo + m, m, max_len, small_max, g.d_refs.p);
      set_keys(j, salts, cid_key);
      HIP_TRY(launch_post_small(j, c->stream));
      if (max_med) {  // blobs above small_max (k_small skipped them)
        RaggedJob rj = ragged_job(g.d_in.p, g.d_ct.p, d_lo, d_lo + m, m, small_max, max_med,
                                  g.d_refs.p);
        set_keys(rj, salts.raw, cid_key);
        HIP_TRY(launch_post_ragged(rj, c->stream));
      }
      HIP_TRY(hipEventRecord(g.hashed, c->stream));
      HIP_TRY(hipStreamWaitEvent(c->s_down, g.hashed, 0));
      HIP_TRY(hipMemcpyAsync(g.h_refs.p, g.d_refs.p, 64 * m, hipMemcpyDeviceToHost, c->s_down));
      if (post && bytes)
        HIP_TRY(hipMemcpyAsync(g.h_ct.p, g.d_ct.p, bytes, hipMemcpyDeviceToHost, c->s_down));
      HIP_TRY(hipEventRecord(g.done, c->s_down));
      return 0;
    };
    if (int e = run()) {
      drain();
      return e;
    }
    g.i0 = i;
    g.i1 = i1;
    g.busy = true;
    i = i1;
  }
  // the rest, oldest first
  for (int r = 0; r < 3; ++r) {
    Ctx::BlobSlot &g = c->bslot[(k + r) % 3];
    if (int e = complete_group(g, lengths, med_max, big, post, post_ctx, roots_out)) {
      drain();
      return e;
    }
  }
  return 0;
}
}  // namespace

int glfsx_post_blobs(uint64_t block_size, uint64_t store_max, const uint8_t *salt,
                     const uint8_t *cid_key, const void *data,
                     const uint64_t *offsets, const uint64_t *lengths, uint64_t n,
                     glfsx_post_fn post, void *post_ctx, uint8_t *roots_out) {
  if (n == 0) return 0;
  if (!data || !offsets || !lengths || !roots_out)
    return fail(GLFSX_E_ARG, "null argument");
  const uint64_t bs = block_size ? block_size : store_max;  // blob.go:86-89
  if (bs > store_max)
    return fail(GLFSX_E_BLOCKSIZE_GT_MAX, "blockSize %llu > maxSize %llu",
                (unsigned long long)bs, (unsigned long long)store_max);
  if (int e = check_block_size(bs)) return e;
  // single-block blobs of up to kMaxMedLen go through the pipelined device
  // batches (post_small_groups: their root is the block's ref,
  // blob.go:190-193); larger ones are Created one by one through the Writer,
  // their Posts captured and delivered in call order with the others'.
  std::vector<std::vector<CapturedPost>> big(n);
  uint64_t n_grouped = 0;
  const uint64_t small_max = small_max_for(bs);  // one block, <= 16 KiB
  const uint64_t med_max = std::min(bs, kMaxMedLen);
  for (uint64_t i = 0; i < n; ++i) {
    if (lengths[i] <= med_max) {
      ++n_grouped;
    } else {
      glfsx_root r;
      if (int e = glfsx_create(bs, store_max, salt, cid_key,
                               static_cast<const uint8_t *>(data) + offsets[i],
                               lengths[i], capture_post, &big[i], &r))
        return e;
      memcpy(roots_out + 64 * i, r.ref, 64);
    }
  }
  if (n_grouped) {
    Ctx *c;
    if (int e = ctx_get(&c)) return e;
    if (int e = post_small_groups(c, bs, salt, cid_key, static_cast<const uint8_t *>(data),
                                  offsets, lengths, n, small_max, med_max, big, post,
                                  post_ctx, roots_out))
      return e;
  } else {
    for (uint64_t i = 0; i < n; ++i)
      if (int e = replay(big[i], post, post_ctx)) return e;
  }
  return 0;
}

// BASELINE config 4 in one call, device-resident: tree.go:250-320's
// PostTreeMap over n entries whose blobs are glfs.PostBlob'd (machine.go:64)
// -- blob roots (glfsx_post_blobs_device), the tree's JSON lines
// (glfsx_tree_encode_device) and the tree blob's Create
// (glfsx_create_device) -- in one call, every launch queued before the host
// waits:
//   A: the blobs' DEK pass;
//   B (beside it): the lines' layout (lengths, then a one-workgroup prefix
//      that stores the total in a pinned word the host reads) and the lines
//      without their hex digits, at raised wave priority (a hex field is
//      fixed width, so the layout does not depend on the roots' values);
//   A: the blobs' CID pass once the static lines are in, writing each
//      root's hex digits into its line;
//   A: the tree blob's blocks and index levels (glfsx_create_device's
//      closed form) once the host has read the total.
// Same bytes and roots as the three calls in sequence
// (tests/test_gpu_tree_read.py).  Blobs above 16 KiB, a tree block size that
// is not a multiple of 64, or no line buffer take the three calls in
// sequence.
namespace {
int post_tree_device_impl(uint64_t n, uint64_t blob_bs, const uint8_t *blob_salt,
                          const uint8_t *tree_salt, const uint8_t *cid_key,
                          const void *d_data, const uint64_t *d_offsets,
                          const uint64_t *d_lengths, uint64_t max_len, void *d_ctext,
                          void *d_roots, const uint8_t *d_names,
                          const uint64_t *d_name_offs, const uint32_t *d_modes,
                          const uint8_t *d_types, const uint64_t *d_type_offs,
                          const uint64_t *d_block_sizes, uint64_t tree_bs, void *d_lines,
                          uint64_t lines_cap, void *d_tree_ctext, glfsx_root *tree_root,
                          uint64_t *lines_len, void *stream) {
  if (!tree_root || !lines_len) return fail(GLFSX_E_ARG, "null argument");
  if (int e = check_block_size(blob_bs)) return e;
  if (int e = check_block_size(tree_bs)) return e;
  if (n == 0 || max_len > small_max_for(blob_bs) || tree_bs % 64 || !d_lines) {
    if (int e = glfsx_post_blobs_device(blob_bs, blob_salt, cid_key, d_data, d_offsets,
                                        d_lengths, n, max_len, d_ctext, d_roots, stream))
      return e;
    if (int e = glfsx_tree_encode_device(n, d_names, d_name_offs, d_modes, d_types,
                                         d_type_offs, static_cast<const uint8_t *>(d_roots),
                                         d_lengths, d_block_sizes, d_lines, lines_cap,
                                         nullptr, lines_len, stream))
      return e;
    return glfsx_create_device(tree_bs, tree_salt, cid_key, d_lines, *lines_len,
                               d_tree_ctext, tree_root, nullptr, stream);
  }
  if (!d_data || !d_offsets || !d_lengths || !d_roots || !d_name_offs || !d_modes ||
      !d_type_offs || !d_block_sizes)
    return fail(GLFSX_E_ARG, "null argument");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  hipStream_t A = pick_stream(c, stream);
  if (!c->stream2) HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  hipStream_t B = c->stream2;
  const uint64_t wgs = (n + kTreeWG - 1) / kTreeWG;
  for (Event &ev : c->events)
    if (int e = ev.ensure()) return e;
  hipEvent_t ev_before = c->events[0], ev_layout = c->events[1], ev_static = c->events[2];
  Salts bsalts, tsalts;
  if (int e = derive_salts(c, blob_salt, &bsalts)) return e;
  if (int e = derive_salts(c, tree_salt, &tsalts)) return e;
  const uint64_t words = n + wgs + 1;
  if (int e = c->d_tree.ensure(8 * (words + n))) return e;
  if (int e = c->h_tree.ensure(8 * (wgs + 1))) return e;
  TreeJob tj = tree_job(n, d_names, d_name_offs, d_modes, d_types, d_type_offs, d_roots,
                        d_lengths, d_block_sizes, c->d_tree.p, words, d_lines, lines_cap);
  tj.hex_pos = tj.scratch + words;  // where each root's digits go
  tj.prio = 1;                      // beside the DEK pass: raised issue priority
  // the prefix stores the exclusive prefixes and the total in the pinned
  // words the host reads (a copy kernel behind it on B would wait for a CU
  // beside the DEK pass -- 1.1 ms in the round-4 trace)
  tj.prefix_host = reinterpret_cast<uint64_t *>(c->h_tree.dptr());
  // B's work comes after everything already on A
  HIP_TRY(hipEventRecord(ev_before, A));
  HIP_TRY(hipStreamWaitEvent(B, ev_before, 0));
  SmallJob sj = small_job(d_data, d_ctext, d_offsets, d_lengths, n, max_len,
                          small_max_for(blob_bs), d_roots);
  set_keys(sj, bsalts, cid_key);
  sj.passes = 1;  // the DEK pass: the critical path, queued first
  HIP_TRY(launch_post_small(sj, A));
  HIP_TRY(launch_tree_layout(tj, B));
  HIP_TRY(hipEventRecord(ev_layout, B));
  HIP_TRY(launch_tree_static(tj, B));
  HIP_TRY(hipEventRecord(ev_static, B));
  sj.passes = 2;  // the CID pass, writing the digits once the static parts are in
  sj.hex_out = static_cast<uint8_t *>(d_lines);
  sj.hex_pos = tj.hex_pos;
  sj.cid_wait = ev_static;
  HIP_TRY(launch_post_small(sj, A));
  // the layout (beside the DEK pass) gives the tree blob's size
  HIP_TRY(hipEventSynchronize(ev_layout));
  const uint64_t total = static_cast<const uint64_t *>(c->h_tree.p)[wgs];
  if (total > lines_cap) {
    HIP_TRY(hipStreamSynchronize(A));
    *lines_len = total;
    return fail(GLFSX_E_ARG, "tree lines need %llu bytes, buffer holds %llu",
                (unsigned long long)total, (unsigned long long)lines_cap);
  }
  // the tree blob, on A after the CID pass (its lines are complete then)
  const uint64_t nblk = (total + tree_bs - 1) / tree_bs;
  const uint64_t n1 = (nblk + tree_bs / 64 - 1) / (tree_bs / 64);
  if (int e = level_prepare(c->d_lvl_a, nblk, n1, tree_bs, A)) return e;
  uint8_t *lvl = c->d_lvl_a.u8();
  PostJob j = block_job(d_lines, total, tree_bs, d_tree_ctext, dense_refs(lvl));  // ref t at byte 64t
  set_keys(j, tsalts.raw, cid_key);
  HIP_TRY(launch_post(j, A, fused_posts()));
  *lines_len = total;
  tree_root->size = total;
  tree_root->block_size = tree_bs;
  if (nblk <= 1) {  // one block: its ref is the root (blob.go:190-193)
    if (int e = c->h_root.ensure(64)) return e;
    HIP_TRY(hipMemcpyAsync(c->h_root.p, lvl, 64, hipMemcpyDeviceToHost, A));
    HIP_TRY(stream_wait(A));  // (B is drained: A waited for its static lines)
    if (int e = fused_check(A)) return e;
    memcpy(tree_root->ref, c->h_root.p, 64);
    return 0;
  }
  uint64_t posts = 0;
  return build_up(c, A, tsalts, cid_key, tree_bs, lvl, n1, &c->d_lvl_b, tree_root->ref, &posts);
}
}  // namespace

int glfsx_post_tree_device(uint64_t n, uint64_t blob_bs, const uint8_t *blob_salt,
                           const uint8_t *tree_salt, const uint8_t *cid_key,
                           const void *d_data, const uint64_t *d_offsets,
                           const uint64_t *d_lengths, uint64_t max_len, void *d_ctext,
                           void *d_roots, const uint8_t *d_names,
                           const uint64_t *d_name_offs, const uint32_t *d_modes,
                           const uint8_t *d_types, const uint64_t *d_type_offs,
                           const uint64_t *d_block_sizes, uint64_t tree_bs, void *d_lines,
                           uint64_t lines_cap, void *d_tree_ctext, glfsx_root *tree_root,
                           uint64_t *lines_len, void *stream) {
  return with_fused_retry([&] {
    return post_tree_device_impl(n, blob_bs, blob_salt, tree_salt, cid_key, d_data, d_offsets,
                                 d_lengths, max_len, d_ctext, d_roots, d_names, d_name_offs,
                                 d_modes, d_types, d_type_offs, d_block_sizes, tree_bs, d_lines,
                                 lines_cap, d_tree_ctext, tree_root, lines_len, stream);
  });
}

int glfsx_tree_encode_device(uint64_t n, const uint8_t *d_names,
                             const uint64_t *d_name_offs, const uint32_t *d_modes,
                             const uint8_t *d_types, const uint64_t *d_type_offs,
                             const uint8_t *d_roots, const uint64_t *d_sizes,
                             const uint64_t *d_block_sizes, void *d_out,
                             uint64_t out_cap, uint64_t *d_line_ends,
                             uint64_t *out_len, void *stream) {
  if (!out_len) return fail(GLFSX_E_ARG, "null out_len");
  *out_len = 0;
  if (n == 0) return 0;
  if (!d_name_offs || !d_modes || !d_type_offs || !d_roots || !d_sizes ||
      !d_block_sizes)
    return fail(GLFSX_E_ARG, "null argument");
  Ctx *c;
  if (int e = ctx_get(&c)) return e;
  hipStream_t s = pick_stream(c, stream);
  const uint64_t words = n + (n + kTreeWG - 1) / kTreeWG + 1;
  if (int e = c->d_tree.ensure(8 * words)) return e;
  if (int e = c->h_small.ensure(64)) return e;
  TreeJob j = tree_job(n, d_names, d_name_offs, d_modes, d_types, d_type_offs, d_roots, d_sizes,
                       d_block_sizes, c->d_tree.p, words, d_out, d_out ? out_cap : 0);
  j.line_ends = d_line_ends;
  HIP_TRY(launch_tree_encode(j, s));
  HIP_TRY(hipMemcpyAsync(c->h_small.p, j.total, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  memcpy(out_len, c->h_small.p, 8);
  if (d_out && *out_len > out_cap)
    return fail(GLFSX_E_ARG, "tree lines need %llu bytes, buffer holds %llu",
                (unsigned long long)*out_len, (unsigned long long)out_cap);
  return 0;
}

int glfsx_tree_decode_device(const void *d_data, uint64_t len, uint8_t *d_names,
                             uint64_t names_cap, uint64_t *d_name_offs, uint32_t *d_modes,
                             uint8_t *d_types, uint64_t types_cap, uint64_t *d_type_offs,
                             uint8_t *d_roots, uint64_t *d_sizes, uint64_t *d_block_sizes,
                             uint32_t *d_status, uint64_t n_cap, uint64_t counts[5],
                             void *stream) {
  Ctx *c;
  if (int e = ctx_get(&c)) return e;  // before any argument is looked at
  if (!counts || (len && !d_data)) return fail(GLFSX_E_ARG, "null argument");
  for (int k = 0; k < 5; ++k) counts[k] = 0;
  if (len > (1ull << 40)) return fail(GLFSX_E_UNSUPPORTED, "tree bytes above 2^40");
  hipStream_t s = pick_stream(c, stream);
  if (len == 0) {  // no lines: the two offset arrays hold their one word
    if (d_name_offs) HIP_TRY(hipMemsetAsync(d_name_offs, 0, 8, s));
    if (d_type_offs) HIP_TRY(hipMemsetAsync(d_type_offs, 0, 8, s));
    HIP_TRY(stream_wait(s));
    return 0;
  }
  // every line has a byte, so len bounds n; at least one word of index
  const uint64_t cap = std::max<uint64_t>(1, std::min(n_cap, len));
  if (tree_decode_wgs(cap) > 0x7FFFFFFFull)
    return fail(GLFSX_E_UNSUPPORTED, "n_cap above the kernels' grid limit");
  TreeDecodeJob j{};
  j.data = static_cast<const uint8_t *>(d_data);
  j.len = len;
  j.n_cap = cap;
  if (int e = c->d_tree.ensure(8 * tree_decode_words(j.data, len, cap))) return e;
  if (int e = c->h_small.ensure(64)) return e;
  j.scratch = reinterpret_cast<uint64_t *>(c->d_tree.p);
  j.names = d_names;
  j.names_cap = names_cap;
  j.name_offs = d_name_offs;
  j.modes = d_modes;
  j.types = d_types;
  j.types_cap = types_cap;
  j.type_offs = d_type_offs;
  j.roots = d_roots;
  j.sizes = d_sizes;
  j.block_sizes = d_block_sizes;
  j.status = d_status;
  if (n_cap == 0) {  // no room for a line: counts only (the index still has a word)
    j.names = j.types = j.roots = nullptr;
    j.name_offs = j.type_offs = j.sizes = j.block_sizes = nullptr;
    j.modes = j.status = nullptr;
  }
  HIP_TRY(launch_tree_decode(j, s));
  HIP_TRY(hipMemcpyAsync(c->h_small.p, j.scratch, 40, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  memcpy(counts, c->h_small.p, 40);
  const bool per_line = d_name_offs || d_modes || d_type_offs || d_roots || d_sizes ||
                        d_block_sizes || d_status;
  if (counts[0] > cap) {  // the index could not hold the lines: nothing was parsed
    counts[1] = counts[2] = counts[3] = 0;
    return fail(GLFSX_E_ARG, "%llu tree lines, n_cap holds %llu", (unsigned long long)counts[0],
                (unsigned long long)cap);
  }
  if (per_line && counts[0] > n_cap)
    return fail(GLFSX_E_ARG, "%llu tree lines, n_cap holds %llu", (unsigned long long)counts[0],
                (unsigned long long)n_cap);
  if ((d_names && counts[1] > names_cap) || (d_types && counts[2] > types_cap))
    return fail(GLFSX_E_ARG, "decoded names / types need %llu / %llu bytes, buffers hold %llu / %llu",
                (unsigned long long)counts[1], (unsigned long long)counts[2],
                (unsigned long long)names_cap, (unsigned long long)types_cap);
  if (n_cap == 0) {  // a tail alone: the offset arrays' one word
    if (d_name_offs) HIP_TRY(hipMemsetAsync(d_name_offs, 0, 8, s));
    if (d_type_offs) HIP_TRY(hipMemsetAsync(d_type_offs, 0, 8, s));
    HIP_TRY(stream_wait(s));
  }
  return 0;
}

namespace {
// One side as the kernels take it; what must be there for n entries: the
// names always, the ref columns with `refs`, the modes with `modes`.
int tree_cols(const glfsx_tree_cols *c, bool refs, bool modes, TreeCols *out) {
  if (!c) return fail(GLFSX_E_ARG, "null column set");
  if (c->n && (!c->name_offs ||
               (refs && (!c->type_offs || !c->roots || !c->sizes || !c->block_sizes)) ||
               (modes && !c->modes)))
    return fail(GLFSX_E_ARG, "null column");
  *out = TreeCols{c->n,     c->names, c->name_offs,   c->modes, c->types, c->type_offs,
                  c->roots, c->sizes, c->block_sizes, c->status};
  return 0;
}
}  // namespace

int glfsx_tree_join_device(const glfsx_tree_cols *a, const glfsx_tree_cols *b,
                           int64_t *d_a_match, int64_t *d_b_match, uint8_t *d_a_class,
                           void *stream) {
  Ctx *c;
  if (int e = ctx_get(&c)) return e;  // before any argument is looked at
  TreeJoinJob j{};
  if (int e = tree_cols(a, d_a_class != nullptr, false, &j.a)) return e;
  if (int e = tree_cols(b, d_a_class != nullptr, false, &j.b)) return e;
  if ((j.a.n + j.b.n + kTreeWG - 1) / kTreeWG > 0x7FFFFFFFull)
    return fail(GLFSX_E_UNSUPPORTED, "entries above the kernel's grid limit");
  j.a_match = d_a_match;
  j.b_match = d_b_match;
  j.a_class = d_a_class;
  HIP_TRY(launch_tree_join(j, pick_stream(c, stream)));
  return 0;
}

int glfsx_tree_select_device(const glfsx_tree_cols *a, const glfsx_tree_cols *b,
                             const int64_t *d_sel, uint64_t k, uint8_t *d_names,
                             uint64_t names_cap, uint64_t *d_name_offs, uint32_t *d_modes,
                             uint8_t *d_types, uint64_t types_cap, uint64_t *d_type_offs,
                             uint8_t *d_roots, uint64_t *d_sizes, uint64_t *d_block_sizes,
                             uint32_t *d_status, uint64_t k_cap, uint64_t counts[2],
                             void *stream) {
  Ctx *c;
  if (int e = ctx_get(&c)) return e;  // before any argument is looked at
  if (!counts || (k && !d_sel)) return fail(GLFSX_E_ARG, "null argument");
  counts[0] = counts[1] = 0;
  TreeSelectJob j{};
  if (int e = tree_cols(a, true, d_modes != nullptr, &j.a)) return e;
  if (int e = tree_cols(b, true, d_modes != nullptr, &j.b)) return e;
  if ((k + kTreeWG - 1) / kTreeWG > 0x7FFFFFFFull)
    return fail(GLFSX_E_UNSUPPORTED, "k above the kernels' grid limit");
  hipStream_t s = pick_stream(c, stream);
  if (k == 0) {  // no entries: the two offset arrays hold their one word
    if (d_name_offs) HIP_TRY(hipMemsetAsync(d_name_offs, 0, 8, s));
    if (d_type_offs) HIP_TRY(hipMemsetAsync(d_type_offs, 0, 8, s));
    HIP_TRY(stream_wait(s));
    return 0;
  }
  const bool per_entry = d_name_offs || d_modes || d_type_offs || d_roots || d_sizes ||
                         d_block_sizes || d_status;
  if (int e = c->d_tree.ensure(8 * tree_select_words(k))) return e;
  if (int e = c->h_small.ensure(64)) return e;
  j.sel = d_sel;
  j.k = k;
  j.scratch = reinterpret_cast<uint64_t *>(c->d_tree.p);
  j.write = (per_entry || d_names || d_types) && !(per_entry && k > k_cap);
  j.names = d_names;
  j.names_cap = names_cap;
  j.name_offs = d_name_offs;
  j.modes = d_modes;
  j.types = d_types;
  j.types_cap = types_cap;
  j.type_offs = d_type_offs;
  j.roots = d_roots;
  j.sizes = d_sizes;
  j.block_sizes = d_block_sizes;
  j.status = d_status;
  HIP_TRY(hipMemsetAsync(j.scratch, 0, 24, s));  // the two totals and the bad-sel flag
  HIP_TRY(launch_tree_select(j, s));
  HIP_TRY(hipMemcpyAsync(c->h_small.p, j.scratch, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  uint64_t res[3];
  memcpy(res, c->h_small.p, 24);
  counts[0] = res[0];
  counts[1] = res[1];
  if (res[2]) return fail(GLFSX_E_ARG, "a sel value names no entry of either side");
  if (per_entry && k > k_cap)
    return fail(GLFSX_E_ARG, "%llu entries selected, k_cap holds %llu", (unsigned long long)k,
                (unsigned long long)k_cap);
  if ((d_names && res[0] > names_cap) || (d_types && res[1] > types_cap))
    return fail(GLFSX_E_ARG, "selected names / types need %llu / %llu bytes, buffers hold %llu / %llu",
                (unsigned long long)res[0], (unsigned long long)res[1],
                (unsigned long long)names_cap, (unsigned long long)types_cap);
  return 0;
}

