// launch_plan.h -- which kernel a launch of post_kernels.hip runs and with
// what shape, as pure functions of the job's sizes, the low bits of its
// addresses and the tuning values: no HIP call, builds with the host compiler
// alone, CPU-tested (tests/c/stream_scratch_test.cpp, launch_plan_sweep.cpp).
// A launch is a LaunchRec, which its family's one launch site runs and logs:
// the bulk passes (k_pass, k_quad, k_pass_dc, k_open) in the pass log, the
// small-blob, decrypt, ragged and one-shot kernels in the aux log.  Rationale
// and measurements: DESIGN.md.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "launch_log.h"
#include "one_classes.h"

#if defined(__HIPCC__)
#define PLAN_HD __host__ __device__ __forceinline__
#else
#define PLAN_HD inline
#endif

namespace glfsx {

constexpr uint32_t kMaxSplitLog2 = 8;  // the last workgroup merges <= 256 CVs
constexpr uint64_t kDcMinWgs = 1024;   // see pass_plan

// The tuning values, read once per call: a launch of fewer than split_target
// workgroups spreads each message over more (0: never); one of at most
// latency_wgs (default 512 = 2 waves per SIMD) is latency-bound.
struct Knobs {
  uint32_t split_target, latency_wgs;
};

// The launchable set: what the dispatchers of post_kernels.hip instantiate.
constexpr int kPassGs[] = {1, 2, 4, 8, 16, 32, 64};  // k_pass<G, CHACHA, ALIGNED, A>
constexpr int kQuadQpws[] = {64, 256};                // k_quad<QPW>
constexpr int kDcGs[] = {1, 2, 4};                    // k_pass_dc<G>
constexpr int kOpenGs[] = {1, 2, 4, 8};               // k_open<G, ALIGNED, 2>
constexpr int kSmallGs[] = {1, 2, 4, 8, 16};          // k_small, k_small_q (the aux log)
template <class T, size_t N>
constexpr bool among(const T (&set)[N], uint32_t x) {
  for (size_t i = 0; i < N; ++i)
    if (uint32_t(set[i]) == x) return true;
  return false;
}
// k_pass: unaligned only in form 2; form 1 only the aligned CID pass, G >= 4.
constexpr bool pass_form_ok(uint32_t g, bool chacha, bool aligned, uint32_t form) {
  return form == 2 || (aligned && (form == 0 || (form == 1 && chacha && g >= 4)));
}
// The ragged passes (RagKind below: the post's two, the open's three modes):
// k_rag_chunk<kind == 1, A>, k_rag_open_chunk<kind - 2, A>, the merge levels.
enum RagKind : uint32_t {
  kRagPostDek = 0, kRagPostCid = 1, kRagOpen0 = 2, kRagOpen1 = 3, kRagOpen2 = 4
};
constexpr int kRagPostKinds[] = {kRagPostDek, kRagPostCid};
constexpr int kRagOpenKinds[] = {kRagOpen2, kRagOpen1, kRagOpen0};
constexpr int kRagForms[] = {0, 2};
constexpr uint32_t kRagMaxGrid = 1u << 20;
constexpr bool rag_chacha(uint32_t kind) { return kind == kRagPostCid || kind >= kRagOpen1; }
// The one-shot classes: k_one<QUADS>, k_one_open<QUADS, SALTED>, each by value
// or over an array; QUADS 16 up to kOneQuads16Max bytes.  The medium pair: 64.
constexpr int kOneQuads[] = {16, 64};
constexpr uint64_t kOneQuads16Max = 16 * 1024;
constexpr bool aux_launchable(const LaunchRec &r) {
  if (r.family >= kLaunchRagChunk && r.family <= kLaunchRagMergeB)
    return (among(kRagPostKinds, r.g) || among(kRagOpenKinds, r.g)) &&
           r.chacha == rag_chacha(r.g) && !r.aligned &&
           (r.family == kLaunchRagChunk ? among(kRagForms, r.form) : r.form == 0);
  if (!r.aligned || r.form || r.fine_div > 1) return false;
  if (r.family == kLaunchMed) return r.g == 64 && r.chacha;
  if (r.family == kLaunchOne) return among(kOneQuads, r.g) && r.chacha;
  return r.family == kLaunchOneOpen && among(kOneQuads, r.g);
}
constexpr bool launchable(const LaunchRec &r) {
  const bool both = r.chacha == 1 && r.form == 2;  // k_pass_dc, k_open: both passes, form 2
  if (r.chacha > 1 || r.aligned > 1) return false;
  if (r.family >= kLaunchRagChunk) return aux_launchable(r);
  if (r.family == kLaunchPass)
    return among(kPassGs, r.g) && pass_form_ok(r.g, r.chacha, r.aligned, r.form);
  if (r.family == kLaunchQuad)
    return among(kQuadQpws, r.g) && !r.chacha && r.aligned && r.form == 0;
  if (r.family == kLaunchPassDc) return among(kDcGs, r.g) && both && r.aligned;
  return r.family == kLaunchOpen && among(kOpenGs, r.g) && both;
}

// ARX form: latency-bound launches run form 0, the compiler-scheduled ARX,
// which then issues faster than the asm forms (tools/arx.hip); others `bulk`.
inline uint32_t arx_form(uint64_t wgs, uint32_t latency_wgs, uint32_t bulk = 2) {
  return wgs <= latency_wgs ? 0u : bulk;
}

inline uint64_t chunks_of(uint64_t len) { return len ? (len + 1023) >> 10 : 1; }

// Chunks per lane (g) and log2 workgroups per message (sl) of a launch over
// n messages of at most maxlen bytes.
struct PassPlan {
  int g;
  uint32_t sl;
};
inline PassPlan pass_plan(uint64_t n, uint64_t maxlen, uint32_t split_target,
                          uint32_t latency_wgs) {
  const uint64_t C = chunks_of(maxlen);
  int g = 1;
  while (256ull * g < C && g < 64) g *= 2;
  // messages above 256 lanes x 64 chunks (16 MiB) always span several
  // workgroups
  uint32_t sl = 0;
  while ((256ull * g << sl) < C) ++sl;
  // few messages: halve the chunks per lane and double the workgroups per
  // message until the launch fills the chip (256 CUs x 8 workgroups)
  const uint64_t target = split_target;
  const int g0 = g;
  const uint32_t sl0 = sl;
  while (g > 1 && sl < kMaxSplitLog2 && (n << sl) < target) {
    g /= 2;
    ++sl;
  }
  // ... but a one-launch split post (k_pass_dc: more than latency_wgs * 5/8
  // workgroups, G <= 4) of fewer than ~1024 workgroups runs its DEK and CID
  // items in about one round each and loses to the two-pass latency form:
  // take the plan with the most workgroups that stays in that form
  // (scripts/r4_plan_sweep.py)
  const uint64_t lat = uint64_t(latency_wgs) * 5 / 8;
  if (sl > 0 && g <= 4 && (n << sl) > lat && (n << sl) < kDcMinWgs) {
    int bg = 0;
    uint32_t bsl = 0;
    for (int gg = g0, s = int(sl0); gg >= 1 && s <= int(kMaxSplitLog2); gg /= 2, ++s)
      if ((n << s) <= lat) {
        bg = gg;
        bsl = uint32_t(s);
      }
    if (bg && bsl > 0) {
      g = bg;
      sl = bsl;
    }
  }
  return {g, sl};
}

// k_pass under plan p.  Above the latency bound the aligned CID pass with no
// split and G >= 4 (the headline's) runs form 1 (quarter-round order),
// everything else form 2 (step-interleaved).
inline LaunchRec pass_rec(PassPlan p, bool chacha, bool aligned, uint64_t n, uint32_t latency_wgs) {
  const uint32_t grid = uint32_t(n << p.sl);
  const uint32_t form =
      aligned ? arx_form(grid, latency_wgs, chacha && p.g >= 4 && p.sl == 0 ? 1 : 2) : 2u;
  return {kLaunchPass, uint32_t(p.g), chacha, aligned, form, p.sl, grid, 0, 0, uint32_t(n)};
}

// BLAKE3-only pass in quad layout (k_quad): latency-bound launches of at
// most 16384 chunks, messages of at most 64 x 256 KiB.  Messages of up to
// 64 x 64 KiB (4 MiB: index nodes at 1-4 MiB blocks) use 64 quads per
// workgroup, larger ones 256 (the last workgroup merges <= 64 CVs, one per
// quad of its own).  refs4: ref address, offset and stride multiples of 4.
inline int quad_qpw(uint64_t maxlen) { return maxlen <= (64ull << 16) ? 64 : 256; }
inline bool quad_ok(uint64_t n, uint64_t maxlen, bool aligned, bool refs4, uint32_t sl,
                    uint32_t latency_wgs) {
  return aligned && refs4 && (n << sl) <= latency_wgs && n * chunks_of(maxlen) <= 16384 &&
         maxlen <= (64ull * 256) << 10;
}
inline LaunchRec quad_rec(uint64_t n, uint64_t maxlen) {
  const int qpw = quad_qpw(maxlen);
  const uint64_t span = uint64_t(qpw) << 10;
  const uint64_t W = maxlen > span ? (maxlen + span - 1) / span : 1;
  uint32_t sl = 0;
  while ((1ull << sl) < W) ++sl;
  return {kLaunchQuad, uint32_t(qpw), 0, 1, 0, sl, uint32_t(n << sl), 0, 0, uint32_t(n)};
}
// A BLAKE3-only pass (DEK, or CID of ctext in memory): k_quad where it may.
inline LaunchRec hash_rec(PassPlan p, uint64_t n, uint64_t maxlen, bool aligned, bool refs4,
                          uint32_t latency_wgs) {
  if (quad_ok(n, maxlen, aligned, refs4, p.sl, latency_wgs)) return quad_rec(n, maxlen);
  return pass_rec(p, false, aligned, n, latency_wgs);
}

// k_pass_dc's work lists (message j on list j % kLists).  Items of list x:
// the DEK items of its m messages (2^sl each), then the CID items: coarse
// (2^sl per message) for the first m - F, fine (2^(sl+1), half the chunks per
// lane, for a shorter run-down) for the last F = ceil(m / fine_div).
constexpr uint32_t kLists = 8;  // one per XCD
constexpr uint32_t kDcFineDiv = 4;
PLAN_HD uint32_t dc_list_msgs(uint32_t n, uint32_t x) {
  return n > x ? (n - x + kLists - 1u) / kLists : 0u;
}
PLAN_HD uint32_t dc_list_fine(uint32_t m, uint32_t fine_div) {
  return fine_div ? (m + fine_div - 1u) / fine_div : 0u;
}
PLAN_HD uint32_t dc_list_items(uint32_t m, uint32_t f, uint32_t sl) {
  return (2u * m + f) << sl;
}

// One post, as the selection sees it.  *_lo: the low four bits of the
// addresses (ctext_lo 0 without ctext).  fuse: launch_post's `fused`.
struct PostShape {
  uint64_t n, msg_len, last_len, stride;
  uint32_t src_lo, ctext_lo, refs_lo;
  bool has_ctext;
  uint64_t out_bf, out_stride;
  bool fuse;
  uint64_t maxlen() const { return n > 1 && msg_len > last_len ? msg_len : last_len; }
  bool aligned() const { return ((src_lo | ctext_lo | stride) & 15) == 0; }
  bool refs4(uint32_t out_off) const { return ((refs_lo | out_off | out_stride) & 3) == 0; }
};
// The one plan of a post: both passes and the fused form follow it.
inline PassPlan plan_of(const PostShape &j, Knobs k) {
  return pass_plan(j.n, j.maxlen(), k.split_target, k.latency_wgs);
}

// The DEK pass (launch_keyed_hash), digests at out_off of each slot.
inline LaunchRec dek_rec(const PostShape &j, PassPlan p, uint32_t out_off, Knobs k) {
  return hash_rec(p, j.n, j.maxlen(), j.aligned(), j.refs4(out_off), k.latency_wgs);
}

// The CID side: one k_pass<G, true, ...>, or -- latency-bound launches, where
// that pass runs ChaCha20 and BLAKE3 in series on one wave per SIMD -- a
// keystream launch (launch_decrypt at block size ks_bs) and a BLAKE3 pass over
// the ctext.  Needs the ctext in memory, dense DEKs, contiguous messages.
struct CidRoute {
  bool keystream;
  uint64_t ks_bs;
  LaunchRec pass;
};
inline CidRoute cid_route(const PostShape &j, PassPlan p, Knobs k) {
  const bool dense = j.out_bf >= j.n, contiguous = j.n == 1 || j.stride == j.msg_len;
  if ((j.n << p.sl) <= k.latency_wgs && j.has_ctext && dense && contiguous &&
      (j.n == 1 || j.msg_len % 64 == 0)) {
    const uint64_t one = j.last_len > 4096 ? (j.last_len + 4095) & ~4095ull : 4096;
    const bool aligned = ((j.ctext_lo | j.stride) & 15) == 0;
    return {true, j.n > 1 ? j.msg_len : one,
            hash_rec(p, j.n, j.maxlen(), aligned, j.refs4(0), k.latency_wgs)};
  }
  return {false, 0, pass_rec(p, true, j.aligned(), j.n, k.latency_wgs)};
}

// A whole post: one k_pass_dc launch (its record in `dek`) for split-mode
// posts of more than 5/8 latency_wgs workgroups whose two passes would each be
// a k_pass<G <= 4, CHACHA, true, 2> launch; else the DEK pass and the CID side.
struct PostRoute {
  bool fused;
  LaunchRec dek;
  CidRoute cid;
};
inline PostRoute post_route(const PostShape &j, Knobs k) {
  const PassPlan p = plan_of(j, k);
  const uint64_t maxlen = j.maxlen(), wgs = j.n << p.sl;
  if (!j.fuse || j.n < 2 || !j.aligned() || !j.refs4(0) || p.sl == 0 || maxlen == 0 ||
      wgs * 8 <= uint64_t(k.latency_wgs) * 5 || !among(kDcGs, uint32_t(p.g)) ||
      quad_ok(j.n, maxlen, true, true, p.sl, k.latency_wgs))
    return {false, dek_rec(j, p, 32, k), cid_route(j, p, k)};
  const uint32_t fine_div = (p.g > 1 && p.sl < kMaxSplitLog2) ? kDcFineDiv : 0u;
  uint64_t items = 0;
  for (uint32_t x = 0; x < kLists; ++x) {
    const uint32_t m = dc_list_msgs(uint32_t(j.n), x);
    items += dc_list_items(m, dc_list_fine(m, fine_div), p.sl);
  }
  return {true, {kLaunchPassDc, uint32_t(p.g), 1, 1, 2, p.sl, uint32_t(items), fine_div,
                 uint32_t(items), uint32_t(j.n)}, {}};
}

// The verified read.  route: 0 auto, 1 always composed, 2 fused wherever
// k_open is able (salted, blocks of at most 256 lanes x 8 chunks).  Auto
// fuses only where k_open measured no slower (DESIGN.md "k_open -- the
// verified read"): from 1024 blocks of at least 256 KiB and 1 GiB in all.
inline bool open_rec(uint64_t n, uint64_t bs, bool salted, bool aligned, int route, LaunchRec *r) {
  const bool able = salted && bs <= (2ull << 20);
  const bool wins = n >= 1024 && bs >= (256ull << 10) && n * bs >= (1ull << 30);
  if (!able || route == 1 || (route == 0 && !wins)) return false;
  const uint64_t C = (bs + 1023) >> 10;
  const uint32_t g = C <= 256 ? 1 : C <= 512 ? 2 : C <= 1024 ? 4 : 8;
  *r = {kLaunchOpen, g, 1, aligned, 2, 0, uint32_t(n), 0, 0, uint32_t(n)};
  return true;
}

// ---- The families outside the pass log ----
// The small-blob kernels (k_small, k_small_q), the read-side decrypt
// (k_decrypt_lines, k_decrypt), the levels of a ragged pass and the one-shot
// classes append to a second log, the aux log (glfsx_debug_aux_log), at their
// launch sites: small_rec, lines_rec, decrypt_rec, rag_pass_recs and one_rec
// below; tests/test_gpu_small_decrypt_matrix.py has a row per instantiation.

struct GridForm {
  uint32_t grid, form;
};
inline uint32_t capped_grid(uint64_t wgs, uint32_t slots) {
  return uint32_t(slots && slots < wgs ? slots : wgs);
}

// One pass of a ragged call (RagKind): the post's DEK or CID pass, or the open
// in mode 0 (the CID alone), 1 (and the plaintext) or 2 (and the DEK check).
// Its chunk level: a workgroup per tile of 256 chunks, at most 2^20;
// latency-bound launches in form 0.  Called by rag_pass_recs alone.
inline GridForm rag_chunk_plan(uint64_t total, uint32_t latency_wgs) {
  const uint64_t tiles = (total + 255) >> 8;
  return {capped_grid(tiles, kRagMaxGrid), arx_form(tiles, latency_wgs)};
}
// Its launches, from the plan's totals (tot: chunks, merge groups, messages
// of more than 256 chunks): the chunk level, then the merge levels that have
// work, a workgroup per group (A) or message (B), at most 2^20.
struct RagPlan {
  uint32_t n;
  LaunchRec rec[3];
};
inline RagPlan rag_pass_recs(const uint64_t tot[3], uint32_t kind, uint32_t latency_wgs) {
  const GridForm c = rag_chunk_plan(tot[0], latency_wgs);
  const uint32_t chacha = rag_chacha(kind);
  RagPlan p{1, {{kLaunchRagChunk, kind, chacha, 0, c.form, 0, c.grid, 0, log_word(tot[0]), 0}}};
  for (uint32_t level = 1; level <= 2; ++level)
    if (tot[level])
      p.rec[p.n++] = {kLaunchRagChunk + level, kind, chacha, 0, 0, 0,
                      capped_grid(tot[level], kRagMaxGrid), 0, log_word(tot[level]), 0};
  return p;
}

// One launch over the n requests of one-shot class c, none longer than
// max_len: k_one or k_one_open with 16 quads of four lanes up to
// kOneQuads16Max bytes and 64 above, or the medium pair (k_med_dek, then
// k_med_cid, on the same grid: a workgroup per 64 KiB span).  One request
// goes by value (fine_div 1), more through the descriptor array.  False: a
// length the class does not take.  r->grid 0: nothing to launch.
inline bool one_rec(OneClass c, uint32_t n, uint64_t max_len, LaunchRec *r) {
  *r = LaunchRec{};
  if (n == 0) return true;
  const bool med = c == kOneMed;
  if (max_len > (med ? kMaxMedLen : kMaxOneLen) || (med && max_len <= kMaxOneLen)) return false;
  const uint32_t quads = max_len <= kOneQuads16Max ? 16 : 64;
  const uint32_t wmax = med ? uint32_t((max_len + 65535) >> 16) : 1u;
  *r = {med ? kLaunchMed : c == kOneSmall ? kLaunchOne : kLaunchOneOpen, quads,
        c != kOneOpen, 1, 0, 0, n * wmax, n == 1, uint32_t(max_len), n};
  return true;
}
// Its workgroup, the kernels' __launch_bounds__: four lanes per quad, and as
// many again for the salted open's second tree.
constexpr uint32_t one_block(const LaunchRec &r) {
  return r.g * (r.family == kLaunchOneOpen && r.chacha ? 8 : 4);
}

// One pass over n small blobs of at most max_len bytes.  g: chunks per blob
// (0: too long).  Few blobs: k_small, a lane per blob, form 0.  Else per-wave
// items (k_small_q): n_coarse items of 64 blobs, the rest -- at least the last
// 1/kSmallFineDiv of the blobs when G > 1 -- as fine items of 64 / G; four
// items per workgroup, at most the resident workgroups (capped_grid).
constexpr uint32_t kSmallFineDiv = 8;
struct SmallPlan {
  int g;
  bool queue;  // k_small_q
  uint32_t form;
  uint64_t n_coarse, items, wgs;
};
inline SmallPlan small_plan(uint64_t n, uint64_t max_len, bool chacha, uint32_t latency_wgs) {
  const uint64_t C = chunks_of(max_len);
  SmallPlan p{};
  while (p.g < 16 && uint64_t(p.g) < C) p.g = p.g ? 2 * p.g : 1;
  if (uint64_t(p.g) < C) p.g = 0;
  p.wgs = (n + 255) / 256;
  p.queue = uint32_t(p.wgs) > latency_wgs;
  if (!p.queue || !p.g) return p;
  p.form = chacha ? 1 : 2;
  const uint64_t fine = p.g > 1 ? n / kSmallFineDiv : 0, bpi = 64 / p.g;
  p.n_coarse = (n - fine) >> 6;  // whole coarse items; the rest goes fine
  p.items = p.n_coarse + (n - (p.n_coarse << 6) + bpi - 1) / bpi;
  p.wgs = (p.items + 3) / 4;
  return p;
}
// The aux-log record of a small-blob launch: grid as launched (k_small_q:
// after capped_grid), n_coarse, items and n saturated.
inline LaunchRec small_rec(const SmallPlan &p, bool chacha, uint32_t grid, uint64_t n) {
  return {p.queue ? kLaunchSmallQ : kLaunchSmall, uint32_t(p.g), chacha, 0, p.form, 0, grid,
          log_word(p.n_coarse), log_word(p.items), log_word(n)};
}

// launch_decrypt over n blocks of bs bytes (the last last_len).  Whole 4 KiB
// units go through the line kernel when bs is a multiple of 4096 and both
// buffers are 16-byte aligned; upb_shift: log2 units per block (64: not a
// power of two).  A wave takes runs of 2^run_shift units (inside one block)
// while that leaves >= 65536 runs (<= 16384 workgroups of 4 waves).
// k_decrypt takes the keystream blocks from first_kb on.
struct DecryptPlan {
  uint64_t units;  // 0: no k_decrypt_lines launch
  uint32_t upb_shift, run_shift;
  GridForm lines;
  uint64_t first_kb;
  uint32_t grid;  // of k_decrypt; 0: no launch
};
inline DecryptPlan decrypt_plan(uint64_t n, uint64_t bs, uint64_t last_len, bool aligned,
                                uint32_t latency_wgs) {
  const uint64_t total = (n - 1) * bs + last_len, kbs = (total + 63) >> 6;
  DecryptPlan p{};
  if (bs % 4096 == 0 && aligned) p.units = total >> 12;
  if (p.units) {
    const uint64_t upb = bs >> 12;
    p.upb_shift = (upb & (upb - 1)) == 0 ? uint32_t(__builtin_ctzll(upb)) : 64u;
    if (p.upb_shift < 64)
      while (p.run_shift < p.upb_shift && (p.units >> (p.run_shift + 1)) >= 65536) ++p.run_shift;
    const uint64_t runs = (p.units + (1ull << p.run_shift) - 1) >> p.run_shift;
    const uint32_t grid = capped_grid((runs + 3) / 4, 16384);
    p.lines = {grid, arx_form(grid, latency_wgs)};
  }
  p.first_kb = p.units << 6;
  if (p.first_kb < kbs) p.grid = capped_grid((kbs - p.first_kb + 255) / 256, 65536);
  return p;
}
// The aux-log records of launch_decrypt's two launches over n blocks.
inline LaunchRec lines_rec(const DecryptPlan &p, uint64_t n) {
  return {kLaunchDecryptLines, 0, 1, 1, p.lines.form, p.run_shift, p.lines.grid, p.upb_shift,
          log_word(p.units), log_word(n)};
}
inline LaunchRec decrypt_rec(const DecryptPlan &p, bool aligned, uint64_t n) {
  return {kLaunchDecrypt, 0, 1, aligned, 0, 0, p.grid, 0, log_word(p.first_kb), log_word(n)};
}

}  // namespace glfsx
#undef PLAN_HD
