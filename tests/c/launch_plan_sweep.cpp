// The kernel selection of glfs_amd/csrc/launch_plan.h, stand-alone: built by
// tests/test_gpu_pass_matrix.py with the host compiler under
// -fsanitize=address,undefined.  No HIP, nothing but the pure functions.
//
//   launch_plan_sweep                 sweeps shapes, alignments and knob values
//       and prints one line "K family g chacha aligned form" per distinct
//       instantiation returned.  Fails unless every record returned is
//       launchable and every launchable instantiation was returned.  Then the
//       families of the aux log: small_plan over every n in 1..5000 and every
//       G ("S family G CHACHA form" lines; the set must be kSmallGs x the
//       dispatcher's forms; k_small_q's item arithmetic covers every blob
//       once) and decrypt_plan ("D family form" lines; units and keystream
//       blocks cover the bytes once, no run straddles a block).  Then
//       rag_pass_recs over chunk totals 0 .. 2^21 + 1 around every multiple
//       of 256 and around 2^20 tiles (merge totals none, one and above 2^20
//       with each; either side of 256 and 2^20 with the totals up to 4097 and
//       above 2^21), the five pass kinds and four latency bounds ("R family
//       kind form" lines), and one_rec over every class, n and length on
//       either side of 16 KiB, 64 KiB and 4 MiB ("O family QUADS salted
//       by_value" lines): grids in closed form, refused lengths refused, and
//       the reachable set equal to the launchable one.
//   launch_plan_sweep --aux FIXTURE   the same replay for the ragged passes
//       and the one-shot classes (scripts/record_launches.py --aux).
//   launch_plan_sweep FIXTURE      feeds every call recorded in FIXTURE
//       (scripts/record_launches.py, run at the commit before the selection
//       moved here) to the pure functions and requires the recorded records.
//
// The replay models how the host runtime forms its jobs (records(): Create's
// levels with bf = bs / 64, single_job with stride 0, the staged host post
// always aligned and free to fuse, the composed open), so it checks
// launch_plan.h together with that model: when create.cpp, blobs.cpp or
// read.cpp form a job differently, update records() with them and record
// again (the script's second run on the GPU is the check without a model).
//
// A fixture line: entry n bs last src_off ct_off refs_off ctmode flag
// latency_wgs split_target open_route nrec, then nrec records of ten words.
// entry: 1 glfsx_dek_batch_device, 2 glfsx_cid_batch_device, 3
// glfsx_post_batch_device, 4 glfsx_post_batch, 5 glfsx_create_device, 6
// glfsx_open_batch_device.  ctmode: 0 no ctext (open: no ptext), 1 out of
// place, 2 in place.  flag: CID keyed (open: salted).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "launch_plan.h"

using namespace glfsx;

struct Case {
  uint64_t entry, n, bs, last, src_off, ct_off, refs_off, ctmode, flag, lat, split, route;
};

static PostShape blocks(const Case &c, uint64_t n, uint64_t last, uint32_t src_lo, uint32_t ct_lo,
                        bool ctext, uint32_t refs_lo, uint64_t bf, uint64_t stride, bool fuse) {
  return {n, c.bs, last, c.bs, src_lo, ctext ? ct_lo : 0u, refs_lo, ctext, bf, stride, fuse};
}

static LaunchRec dek(const PostShape &j, uint32_t out_off, Knobs k) {
  return dek_rec(j, plan_of(j, k), out_off, k);
}

static void post(const PostShape &j, Knobs k, std::vector<LaunchRec> *out) {
  const PostRoute r = post_route(j, k);
  out->push_back(r.dek);
  if (!r.fused) out->push_back(r.cid.pass);
}

// The bulk launches of one call of the C ABI, as the host runtime makes them
// (create.cpp, read.cpp: block_job, single_job, dense_refs, node_refs).
static std::vector<LaunchRec> records(const Case &c) {
  const Knobs k{uint32_t(c.split), uint32_t(c.lat)};
  const uint32_t src = uint32_t(c.src_off) & 15, ct = uint32_t(c.ct_off) & 15,
                 refs = uint32_t(c.refs_off) & 15;
  const bool ctext = c.ctmode != 0;
  std::vector<LaunchRec> out;
  switch (c.entry) {
    case 1:
      out.push_back(dek(blocks(c, c.n, c.last, src, 0, false, refs, ~0ull, 0, false), 32, k));
      break;
    case 2: {
      const PostShape j = blocks(c, c.n, c.last, src, ct, ctext, refs, ~0ull, 0, false);
      out.push_back(cid_route(j, plan_of(j, k), k).pass);
      break;
    }
    case 3:
      post(blocks(c, c.n, c.last, src, ct, ctext, refs, ~0ull, 0, false), k, &out);
      break;
    case 4:  // staged: aligned device buffers, always a ctext, may fuse
      post(blocks(c, c.n, c.last, 0, 0, true, 0, ~0ull, 0, true), k, &out);
      break;
    case 5: {
      if (c.n <= 1) {  // single_job: one message, stride 0
        PostShape j{1, c.last, c.last, 0, src, ctext ? ct : 0u, 0, ctext, ~0ull, 0, true};
        post(j, k, &out);
        break;
      }
      const uint64_t bf = c.bs / 64;
      post(blocks(c, c.n, c.last, src, ct, ctext, 0, bf, c.bs, true), k, &out);
      for (uint64_t nodes = (c.n + bf - 1) / bf;; nodes = (nodes + bf - 1) / bf) {
        const bool root = nodes == 1;
        post(blocks(c, nodes, c.bs, 0, 0, true, 0, root ? ~0ull : bf, root ? 0 : c.bs, true), k,
             &out);
        if (root) break;
      }
      break;
    }
    case 6: {
      const bool aligned = ((src | (ctext ? ct : 0u) | c.bs) & 15) == 0;
      LaunchRec r;
      if (open_rec(c.n, c.bs, c.flag != 0, aligned, int(c.route), &r)) {
        out.push_back(r);
        break;
      }
      // composed: the CID of the ctext, then (salted) the DEK of the plaintext
      // (the caller's, or aligned scratch); digests in aligned scratch
      out.push_back(dek(blocks(c, c.n, c.last, src, 0, false, 0, ~0ull, 0, false), 0, k));
      if (c.flag)
        out.push_back(
            dek(blocks(c, c.n, c.last, ctext ? ct : 0u, 0, false, 0, ~0ull, 0, false), 32, k));
      break;
    }
  }
  return out;
}

static int g_failed = 0;
static void fail(const char *what, const Case &c) {
  fprintf(stderr, "%s: entry %" PRIu64 " n %" PRIu64 " bs %" PRIu64 " last %" PRIu64
          " lat %" PRIu64 " split %" PRIu64 "\n", what, c.entry, c.n, c.bs, c.last, c.lat, c.split);
  ++g_failed;
}

using Kernel = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>;
static Kernel kernel_of(const LaunchRec &r) {
  return Kernel{r.family, r.g, r.chacha, r.aligned, r.form};
}

static void sweep_small();
static void sweep_decrypt();
static void sweep_ragged();
static void sweep_one();

static int sweep() {
  std::set<Kernel> seen;
  const uint64_t KiB = 1024, MiB = 1024 * KiB;
  const uint64_t sizes[] = {64,       4 * KiB,  64 * KiB,      256 * KiB, 512 * KiB, MiB,
                            2 * MiB,  4 * MiB,  4 * MiB + 64,  8 * MiB,   16 * MiB,  32 * MiB,
                            64 * MiB, MiB - 16, 2 * MiB - 1};
  const uint64_t ns[] = {1, 2, 3, 18, 65, 300, 1024, 5000};
  const uint64_t lats[] = {0, 512, 1u << 31}, splits[] = {0, 4, 16, 36, 2048};
  for (uint64_t entry = 1; entry <= 6; ++entry)
    for (uint64_t bs : sizes)
      for (uint64_t n : ns)
        for (uint64_t lat : lats)
          for (uint64_t split : splits)
            for (uint64_t off = 0; off < 2; ++off)
              for (uint64_t ctmode = 0; ctmode < 2; ++ctmode) {
                if (entry == 6 && bs % 64) continue;
                if (entry == 5 && (bs % 64 || bs < 4 * KiB)) continue;
                const Case c{entry, n, bs, bs / 2 + 1, off, 0, 0, ctmode, 1,
                             lat,   split, entry == 6 ? 2 * off : 0};
                for (const LaunchRec &r : records(c)) {
                  if (!launchable(r)) fail("not launchable", c);
                  if (r.grid == 0 || r.n == 0) fail("empty launch", c);
                  seen.insert(kernel_of(r));
                }
              }
  // every member of the launchable set was returned
  size_t launchable_n = 0;
  for (uint32_t family = 0; family <= 5; ++family)
    for (uint32_t g = 0; g <= 512; ++g)
      for (uint32_t chacha = 0; chacha <= 2; ++chacha)
        for (uint32_t aligned = 0; aligned <= 2; ++aligned)
          for (uint32_t form = 0; form <= 3; ++form) {
            const LaunchRec r{family, g, chacha, aligned, form, 0, 1, 0, 0, 1};
            if (!launchable(r)) continue;
            ++launchable_n;
            if (!seen.count(kernel_of(r))) {
              fprintf(stderr, "launchable but never chosen: %u %u %u %u %u\n", family, g, chacha,
                      aligned, form);
              ++g_failed;
            }
          }
  if (launchable_n != seen.size()) ++g_failed;
  for (const Kernel &k : seen)
    printf("K %u %u %u %u %u\n", std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k),
           std::get<4>(k));
  sweep_small();
  sweep_decrypt();
  sweep_ragged();
  sweep_one();
  return g_failed;
}

// ---- the families of the aux log: small blobs and the read-side decrypt ----

static void fail_small(const char *what, uint64_t n, uint64_t max_len, bool chacha, uint64_t lat) {
  fprintf(stderr, "small: %s: n %" PRIu64 " max_len %" PRIu64 " chacha %d lat %" PRIu64 "\n", what,
          n, max_len, int(chacha), lat);
  ++g_failed;
}

// k_small_q's own item arithmetic (small_kernels.h, the first lines of the
// kernel's body: BPI, fine0, items, and the first blob it hands small_fine),
// restated here: with the functions shared through launch_plan.h the compiler
// emitted other code for all ten k_small_q (same registers).  Keep the two in
// step.  The kernel knows only SArgs::n and SArgs::n_coarse.
static uint32_t small_bpi(int g) { return g > 1 ? 64u / uint32_t(g) : 64u; }  // BPI
static uint64_t small_fine0(uint64_t n_coarse) { return n_coarse << 6; }      // fine0
static uint64_t small_items(uint64_t n, uint64_t n_coarse, uint32_t bpi) {    // items
  const uint64_t fine0 = small_fine0(n_coarse);
  return n_coarse + (n > fine0 ? (n - fine0 + bpi - 1) / bpi : 0);
}
static uint64_t small_fine_first(uint64_t item, uint64_t n_coarse, uint32_t bpi) {
  return small_fine0(n_coarse) + (item - n_coarse) * bpi;  // small_fine's b0
}

// k_small_q's walk over its items (the `while (item < items)` loop,
// small_blob's `i >= a.n` and small_fine's `valid`): every blob in exactly
// one item, no item empty, the plan's item count the kernel's own.
static void check_small_items(const SmallPlan &p, uint64_t n, uint64_t max_len, bool chacha) {
  const uint32_t bpi = small_bpi(p.g);
  const uint64_t items = small_items(n, p.n_coarse, bpi), fine0 = small_fine0(p.n_coarse);
  if (items != p.items) fail_small("items differ from the kernel's", n, max_len, chacha, 0);
  if (p.wgs != (items + 3) / 4) fail_small("workgroups", n, max_len, chacha, 0);
  if (fine0 > n) fail_small("coarse items past the end", n, max_len, chacha, 0);
  if (p.g > 1 && n - fine0 < n / kSmallFineDiv) fail_small("too few fine", n, max_len, chacha, 0);
  if (p.g == 1 && n - fine0 >= 64) fail_small("G = 1 leaves a whole item", n, max_len, chacha, 0);
  std::vector<uint8_t> hit(n, 0);
  for (uint64_t item = 0; item < items; ++item) {
    // the kernel's branch: a lane per blob of (item << 6 | lane), or a fine item
    const bool coarse = p.g == 1 || item < p.n_coarse;
    const uint64_t b0 = coarse ? item << 6 : small_fine_first(item, p.n_coarse, bpi);
    const uint64_t b1 = b0 + (coarse ? 64 : bpi);
    if (b0 >= n) fail_small("empty item", n, max_len, chacha, 0);
    for (uint64_t b = b0; b < b1 && b < n; ++b) ++hit[b];
  }
  for (uint64_t b = 0; b < n; ++b)
    if (hit[b] != 1) {
      fail_small("a blob in no item or in two", n, max_len, chacha, 0);
      break;
    }
}

using SmallKernel = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>;  // family G CHACHA form

static void sweep_small() {
  std::set<SmallKernel> seen, want;
  // the dispatcher (launch_small_pass): k_small<G, CHACHA, 0>, k_small_q<G, CHACHA, CHACHA ? 1 : 2>
  for (int g : kSmallGs)
    for (uint32_t chacha = 0; chacha < 2; ++chacha) {
      want.insert({kLaunchSmall, uint32_t(g), chacha, 0u});
      want.insert({kLaunchSmallQ, uint32_t(g), chacha, chacha ? 1u : 2u});
    }
  const uint64_t lats[] = {0, 512, 1u << 31};
  std::vector<uint64_t> ns;
  for (uint64_t n = 1; n <= 5000; ++n) ns.push_back(n);
  for (uint64_t n : {65536ull, 131072ull, 131073ull, 400000ull, 1ull << 20}) ns.push_back(n);
  for (int g : kSmallGs)
    for (uint64_t max_len : {uint64_t(g) << 10, (uint64_t(g) << 10) - 1, (uint64_t(g) << 9) + 1})
      for (uint32_t chacha = 0; chacha < 2; ++chacha)
        for (uint64_t lat : lats)
          for (uint64_t n : ns) {
            const SmallPlan p = small_plan(n, max_len, chacha, uint32_t(lat));
            if (p.g != g) fail_small("G", n, max_len, chacha, lat);
            if (p.queue != ((n + 255) / 256 > lat)) fail_small("queue", n, max_len, chacha, lat);
            if (p.wgs == 0 || p.wgs > UINT32_MAX) fail_small("grid", n, max_len, chacha, lat);
            const LaunchRec r = small_rec(p, chacha, capped_grid(p.wgs, 1280), n);
            if (r.grid == 0 || r.grid > 1280 || r.n != n || r.fine_div != p.n_coarse ||
                r.items != p.items)
              fail_small("record", n, max_len, chacha, lat);
            seen.insert({r.family, r.g, r.chacha, r.form});
            if (p.queue)
              check_small_items(p, n, max_len, chacha);
            else if (p.items || p.n_coarse || p.form)
              fail_small("k_small with items", n, max_len, chacha, lat);
          }
  if (small_plan(1, 0, false, 0).g != 1 || small_plan(1, 16385, false, 0).g != 0) ++g_failed;
  // the work-queue row of the GPU matrix: 400 000 blobs of 64 bytes
  if (small_plan(400000, 64, true, 512).items != 6250) ++g_failed;
  if (seen != want) {
    fprintf(stderr, "small: reached %zu instantiations, the dispatcher has %zu\n", seen.size(),
            want.size());
    ++g_failed;
  }
  for (const SmallKernel &k : seen)
    printf("S %u %u %u %u\n", std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k));
}

static void fail_decrypt(const char *what, uint64_t n, uint64_t bs, uint64_t last, bool aligned) {
  fprintf(stderr, "decrypt: %s: n %" PRIu64 " bs %" PRIu64 " last %" PRIu64 " aligned %d\n", what,
          n, bs, last, int(aligned));
  ++g_failed;
}

// decrypt_plan against the kernels' own walk (read_kernels.h): k_decrypt_lines
// takes run r = units [r << run_shift, min(+ 2^run_shift, units)), the DEK of
// block j = u0 >> upb_shift (or u0 / upb) for the whole run and the counter
// (u - j * upb) << 6; k_decrypt the keystream blocks [first_kb, total_kb).
static void check_decrypt(uint64_t n, uint64_t bs, uint64_t last, bool aligned, uint64_t lat) {
  const DecryptPlan p = decrypt_plan(n, bs, last, aligned, uint32_t(lat));
  const uint64_t total = (n - 1) * bs + last, kbs = (total + 63) >> 6;
  const bool lines = bs % 4096 == 0 && aligned && total >= 4096;
  if ((p.units != 0) != lines) fail_decrypt("line kernel", n, bs, last, aligned);
  // units and keystream blocks cover [0, total) exactly once
  if (p.units << 12 != p.first_kb << 6 || (p.units << 12) > total || p.first_kb > kbs)
    fail_decrypt("cover", n, bs, last, aligned);
  if ((p.grid != 0) != (p.first_kb < kbs)) fail_decrypt("k_decrypt launch", n, bs, last, aligned);
  if (lines && total - (p.units << 12) >= 4096) fail_decrypt("a unit left", n, bs, last, aligned);
  if (!p.units) {
    if (p.lines.grid || p.run_shift || p.upb_shift) fail_decrypt("no units", n, bs, last, aligned);
    return;
  }
  const uint64_t upb = bs >> 12;
  const bool pow2 = (upb & (upb - 1)) == 0;
  if (pow2 ? (1ull << p.upb_shift) != upb : p.upb_shift != 64)
    fail_decrypt("upb_shift", n, bs, last, aligned);
  if (p.upb_shift < 64 ? p.run_shift > p.upb_shift : p.run_shift != 0)
    fail_decrypt("a run straddles a block", n, bs, last, aligned);
  const uint64_t runs = (p.units + (1ull << p.run_shift) - 1) >> p.run_shift;
  if (p.lines.grid == 0 || p.lines.grid > 16384 || p.lines.grid > (runs + 3) / 4)
    fail_decrypt("grid", n, bs, last, aligned);
  if (p.run_shift && (p.units >> p.run_shift) < 65536) fail_decrypt("runs", n, bs, last, aligned);
  if (p.lines.form != (p.lines.grid <= lat ? 0u : 2u)) fail_decrypt("form", n, bs, last, aligned);
  if (p.units > (1u << 18)) return;
  uint64_t next = 0;  // the units in run order are 0, 1, 2, ...
  for (uint64_t run = 0; run < runs; ++run) {
    const uint64_t u0 = run << p.run_shift;
    const uint64_t u1 = u0 + (1ull << p.run_shift) < p.units ? u0 + (1ull << p.run_shift) : p.units;
    const uint64_t j = p.upb_shift < 64 ? u0 >> p.upb_shift : u0 / upb;
    if (u0 >= u1 || j >= n) fail_decrypt("empty run", n, bs, last, aligned);
    for (uint64_t u = u0; u < u1; ++u, ++next) {
      const uint64_t ctr = (u - j * upb) << 6;  // the unit's first counter in block j
      if (u != next || u / upb != j || j * bs + (ctr << 6) != u << 12 || ctr + 64 > (bs >> 6))
        fail_decrypt("unit", n, bs, last, aligned);
    }
  }
  if (next != p.units) fail_decrypt("units walked", n, bs, last, aligned);
}

using DecryptKernel = std::tuple<uint32_t, uint32_t>;  // family form

static void sweep_decrypt() {
  std::set<DecryptKernel> seen;
  const uint64_t KiB = 1024, MiB = 1024 * KiB;
  const uint64_t sizes[] = {64, 128, 4096, 4160, 8192, 12288, 20480, 65536, MiB, 2 * MiB, 3 * MiB};
  const uint64_t ns[] = {1, 2, 3, 6, 7, 33, 261, 513, 4096, 4097, 43691};
  const uint64_t lats[] = {0, 512, 1u << 31};
  for (uint64_t bs : sizes)
    for (uint64_t n : ns)
      for (uint64_t last : {uint64_t(1), uint64_t(5), uint64_t(63), uint64_t(64), uint64_t(65),
                            uint64_t(100), uint64_t(4095), uint64_t(4096), uint64_t(4097),
                            uint64_t(12365), bs / 2, bs - 1, bs})
        for (int aligned = 0; aligned < 2; ++aligned)
          for (uint64_t lat : lats) {
            if (last == 0 || last > bs) continue;
            check_decrypt(n, bs, last, aligned != 0, lat);
            const DecryptPlan p = decrypt_plan(n, bs, last, aligned != 0, uint32_t(lat));
            if (p.units) {
              const LaunchRec r = lines_rec(p, n);
              if (r.split_log2 != p.run_shift || r.fine_div != p.upb_shift || r.items != p.units ||
                  r.grid != p.lines.grid)
                fail_decrypt("record", n, bs, last, aligned != 0);
              seen.insert({r.family, r.form});
            }
            if (p.grid) {
              const LaunchRec r = decrypt_rec(p, aligned != 0, n);
              if (r.items != p.first_kb || r.grid != p.grid || r.aligned != uint32_t(aligned))
                fail_decrypt("record", n, bs, last, aligned != 0);
              seen.insert({r.family, r.form});
            }
          }
  // the rows of the GPU matrix that loop: units, run_shift, upb_shift, grid
  const struct {
    uint64_t n, bs, last, units;
    uint32_t run_shift, upb_shift;
  } big[] = {{261, MiB, 12365, 66563, 0, 8}, {513, MiB, 12365, 131075, 1, 8},
             {43691, 12288, 100, 131070, 0, 64}};
  for (const auto &b : big) {
    const DecryptPlan p = decrypt_plan(b.n, b.bs, b.last, true, 512);
    if (p.units != b.units || p.run_shift != b.run_shift || p.upb_shift != b.upb_shift ||
        p.lines.grid != 16384 || (p.units >> p.run_shift) <= 4ull * p.lines.grid || p.grid != 1)
      fail_decrypt("a looping row", b.n, b.bs, b.last, true);
  }
  if (log_word(UINT32_MAX - 1ull) != UINT32_MAX - 1 || log_word(UINT32_MAX) != UINT32_MAX ||
      log_word(1ull << 32) != UINT32_MAX || log_word(~0ull) != UINT32_MAX)
    ++g_failed;
  const std::set<DecryptKernel> want = {
      {kLaunchDecryptLines, 0u}, {kLaunchDecryptLines, 2u}, {kLaunchDecrypt, 0u}};
  if (seen != want) {
    fprintf(stderr, "decrypt: reached %zu kernels of 3\n", seen.size());
    ++g_failed;
  }
  for (const DecryptKernel &k : seen) printf("D %u %u\n", std::get<0>(k), std::get<1>(k));
}

static int replay(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  size_t lines = 0;
  for (;;) {
    Case c;
    uint64_t nrec;
    const int got = fscanf(f, "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64
                           "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64 "%" SCNu64
                           "%" SCNu64, &c.entry, &c.n, &c.bs, &c.last, &c.src_off, &c.ct_off,
                           &c.refs_off, &c.ctmode, &c.flag, &c.lat, &c.split, &c.route, &nrec);
    if (got == EOF) break;
    if (got != 13 || nrec > 64) {
      fprintf(stderr, "%s: malformed line %zu\n", path, lines + 1);
      fclose(f);
      return 1;
    }
    std::vector<LaunchRec> want(nrec);
    for (LaunchRec &r : want) {
      uint32_t *w = &r.family;
      for (size_t i = 0; i < kLaunchRecWords; ++i)
        if (fscanf(f, "%" SCNu32, &w[i]) != 1) {
          fprintf(stderr, "%s: short record on line %zu\n", path, lines + 1);
          fclose(f);
          return 1;
        }
    }
    const std::vector<LaunchRec> have = records(c);
    if (have.size() != want.size() ||
        memcmp(have.data(), want.data(), have.size() * sizeof(LaunchRec)) != 0) {
      fail("differs from the recorded launches", c);
      for (const LaunchRec &r : have)
        fprintf(stderr, "  now %u %u %u %u %u %u %u %u %u %u\n", r.family, r.g, r.chacha, r.aligned,
                r.form, r.split_log2, r.grid, r.fine_div, r.items, r.n);
    }
    ++lines;
  }
  fclose(f);
  printf("replayed %zu\n", lines);
  return g_failed || lines == 0;
}

// ---- the ragged passes and the one-shot classes ----

static void fail_aux(const char *what, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  fprintf(stderr, "aux: %s: %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", what, a, b, c, d);
  ++g_failed;
}

using AuxKernel = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>;
// "R family kind form" and "O family QUADS salted by_value": the records as
// far as they choose a kernel.
static AuxKernel aux_kernel_of(const LaunchRec &r) {
  if (r.family <= kLaunchRagMergeB) return AuxKernel{r.family, r.g, r.form, 0};
  return AuxKernel{r.family, r.g, r.family == kLaunchOneOpen ? r.chacha : 0u, r.fine_div};
}

// Every record of the ten-word grid that aux_launchable accepts, as kernels.
static std::set<AuxKernel> aux_launchable_set(uint32_t first, uint32_t last) {
  std::set<AuxKernel> out;
  for (uint32_t family = first; family <= last; ++family)
    for (uint32_t g = 0; g <= 65; ++g)
      for (uint32_t chacha = 0; chacha <= 2; ++chacha)
        for (uint32_t aligned = 0; aligned <= 1; ++aligned)
          for (uint32_t form = 0; form <= 3; ++form)
            for (uint32_t by_value = 0; by_value <= 2; ++by_value) {
              const LaunchRec r{family, g, chacha, aligned, form, 0, 1, by_value, 0, 1};
              if (launchable(r)) out.insert(aux_kernel_of(r));
            }
  return out;
}

static void sweep_ragged() {
  std::set<AuxKernel> seen;
  // 0 .. 2^21 + 1 around every multiple of 256 chunks (m - 1, m, m + 1)
  std::vector<uint64_t> totals = {0, 1, 2};
  for (uint64_t m = 256; m <= (1ull << 21); m += 256)
    for (uint64_t d : {uint64_t(0), uint64_t(1), ~uint64_t(0)}) totals.push_back(m + d);
  // 2^20 tiles of 256 chunks, either side, and a count above 32 bits
  for (uint64_t t : {(1ull << 28) - 256, (1ull << 28) - 255, 1ull << 28, (1ull << 28) + 1,
                     (1ull << 32) + 5})
    totals.push_back(t);
  // merge totals: every value either side of 2^20 for the totals up to 4096
  // chunks and the ones above 2^21; none, one and above 2^20 for every total
  const std::vector<uint64_t> all_levels = {0, 1, 255, 256, (1 << 20) - 1, 1 << 20,
                                            (1 << 20) + 1, (1 << 21) + 1};
  const std::vector<uint64_t> few_levels = {0, 1, (1 << 20) + 1};
  const uint32_t lats[] = {0, 1, 512, 1u << 20};
  for (uint32_t kind = kRagPostDek; kind <= kRagOpen2; ++kind)
    for (uint32_t lat : lats)
      for (uint64_t chunks : totals) {
        const bool full = chunks <= 4097 || chunks > (1ull << 21) + 1;
        const std::vector<uint64_t> &levels = full ? all_levels : few_levels;
        for (uint64_t a : levels)
          for (uint64_t b : levels) {
            const uint64_t tot[3] = {chunks, a, b};
            const RagPlan p = rag_pass_recs(tot, kind, lat);
            if (p.n != 1u + (a != 0) + (b != 0)) fail_aux("levels", chunks, a, b, kind);
            uint32_t last = 0;
            for (uint32_t i = 0; i < p.n; ++i) {
              const LaunchRec &r = p.rec[i];
              const uint32_t level = r.family - kLaunchRagChunk;
              if (level > 2 || r.family <= last || !tot[level] != !r.grid)
                fail_aux("order", chunks, a, b, kind);
              last = r.family;
              // the closed forms: a workgroup per tile of 256 chunks, per
              // merge group, per large message; 2^20 at most
              const uint64_t wgs = level ? tot[level] : (chunks + 255) >> 8;
              if (r.grid != (wgs < (1u << 20) ? wgs : 1u << 20)) fail_aux("grid", chunks, a, b, kind);
              if (r.form != (level == 0 && wgs > lat ? 2u : 0u)) fail_aux("form", chunks, a, b, lat);
              if (r.g != kind || r.chacha != (kind == kRagPostCid || kind >= kRagOpen1) ||
                  r.items != log_word(tot[level]) || r.aligned || r.split_log2 || r.fine_div || r.n)
                fail_aux("record", chunks, a, b, kind);
              if (chunks && !launchable(r)) fail_aux("not launchable", chunks, a, b, kind);
              if (r.grid) seen.insert(aux_kernel_of(r));
            }
          }
      }
  if (seen != aux_launchable_set(kLaunchRagChunk, kLaunchRagMergeB)) {
    fprintf(stderr, "ragged: the reachable and the launchable set differ\n");
    ++g_failed;
  }
  for (const AuxKernel &k : seen)
    printf("R %u %u %u\n", std::get<0>(k), std::get<1>(k), std::get<2>(k));
}

static void sweep_one() {
  std::set<AuxKernel> seen;
  const uint64_t MiB = 1 << 20;
  const uint64_t lens[] = {0, 1, 16383, 16384, 16385, 65535, 65536, 65537, 4 * MiB, 4 * MiB + 1};
  for (int c = 0; c < kOneClasses; ++c)
    for (uint32_t n : {0u, 1u, 2u, 1024u})
      for (uint64_t len : lens) {
        LaunchRec r;
        const bool ok = one_rec(OneClass(c), n, len, &r);
        const bool med = c == kOneMed;
        // what the ladders refused: above the class's limit; at or below
        // kMaxOneLen for the medium class; nothing when there is no request
        const bool want = n == 0 || (med ? len > kMaxOneLen && len <= kMaxMedLen : len <= kMaxOneLen);
        if (ok != want) fail_aux("refusal", c, n, len, ok);
        if (!ok || n == 0) {
          if (r.grid || r.family) fail_aux("a record without a launch", c, n, len, ok);
          continue;
        }
        const uint32_t family = med ? kLaunchMed : c == kOneSmall ? kLaunchOne : kLaunchOneOpen;
        const uint32_t quads = len <= 16384 ? 16 : 64, wmax = med ? uint32_t((len + 65535) >> 16) : 1;
        const uint32_t salted = c == kOneOpenSalted, trees = salted ? 2 : 1;
        if (r.family != family || r.g != quads || r.chacha != (c == kOneOpen ? 0u : 1u) ||
            r.aligned != 1 || r.form || r.split_log2 || r.grid != n * wmax ||
            r.fine_div != (n == 1) || r.items != len || r.n != n)
          fail_aux("record", c, n, len, r.grid);
        if (one_block(r) != quads * 4 * trees) fail_aux("block", c, n, len, one_block(r));
        if (!launchable(r)) fail_aux("not launchable", c, n, len, 0);
        seen.insert(aux_kernel_of(r));
      }
  if (seen != aux_launchable_set(kLaunchOne, kLaunchOneOpen)) {
    fprintf(stderr, "one-shot: the reachable and the launchable set differ\n");
    ++g_failed;
  }
  for (const AuxKernel &k : seen)
    printf("O %u %u %u %u\n", std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k));
}

// launch_plan_sweep --aux FIXTURE: the rows of scripts/record_launches.py
// --aux (recorded from the launchers as they were before rag_pass_recs and
// one_rec) against those two functions.
//   R chunks groups large kind latency_wgs nrec <records>
//   O class n max_len nrec <records>
static int replay_aux(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  size_t lines = 0;
  char tag[4];
  while (fscanf(f, "%3s", tag) == 1) {
    uint64_t in[5] = {0, 0, 0, 0, 0}, nrec = 0;
    const int nin = tag[0] == 'R' ? 5 : 3;
    bool ok = (tag[0] == 'R' || tag[0] == 'O') && tag[1] == 0;
    for (int i = 0; ok && i < nin; ++i) ok = fscanf(f, "%" SCNu64, &in[i]) == 1;
    ok = ok && fscanf(f, "%" SCNu64, &nrec) == 1 && nrec <= 3;
    std::vector<LaunchRec> want(ok ? nrec : 0);
    for (LaunchRec &r : want) {
      uint32_t *w = &r.family;
      for (size_t i = 0; ok && i < kLaunchRecWords; ++i) ok = fscanf(f, "%" SCNu32, &w[i]) == 1;
    }
    if (!ok) {
      fprintf(stderr, "%s: malformed line %zu\n", path, lines + 1);
      fclose(f);
      return 1;
    }
    std::vector<LaunchRec> have;
    if (tag[0] == 'R') {
      const RagPlan p = rag_pass_recs(in, uint32_t(in[3]), uint32_t(in[4]));
      have.assign(p.rec, p.rec + p.n);
    } else {
      LaunchRec r;
      if (!one_rec(OneClass(in[0]), uint32_t(in[1]), in[2], &r)) fail_aux("refused", in[0], in[1], in[2], 0);
      if (r.grid) have.push_back(r);
    }
    if (have.size() != want.size() ||
        memcmp(have.data(), want.data(), have.size() * sizeof(LaunchRec)) != 0) {
      fail_aux("differs from the recorded launches", lines + 1, in[0], in[1], in[2]);
      for (const LaunchRec &r : have)
        fprintf(stderr, "  now %u %u %u %u %u %u %u %u %u %u\n", r.family, r.g, r.chacha, r.aligned,
                r.form, r.split_log2, r.grid, r.fine_div, r.items, r.n);
    }
    ++lines;
  }
  fclose(f);
  printf("replayed %zu\n", lines);
  return g_failed || lines == 0;
}

int main(int argc, char **argv) {
  const int bad = argc > 2 && !strcmp(argv[1], "--aux") ? replay_aux(argv[2])
                  : argc > 1                             ? replay(argv[1])
                                                         : sweep();
  if (bad) {
    fprintf(stderr, "launch_plan_sweep: failed\n");
    return 1;
  }
  printf("launch_plan_sweep: ok\n");
  return 0;
}
