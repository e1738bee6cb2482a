// The kernel selection of glfs_amd/csrc/launch_plan.h, stand-alone: built by
// tests/test_gpu_pass_matrix.py with the host compiler under
// -fsanitize=address,undefined.  No HIP, nothing but the pure functions.
//
//   launch_plan_sweep                 sweeps shapes, alignments and knob values
//       and prints one line "K family g chacha aligned form" per distinct
//       instantiation returned.  Fails unless every record returned is
//       launchable and every launchable instantiation was returned.
//   launch_plan_sweep FIXTURE         feeds every call recorded in FIXTURE
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
  return g_failed;
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

int main(int argc, char **argv) {
  const int bad = argc > 1 ? replay(argv[1]) : sweep();
  if (bad) {
    fprintf(stderr, "launch_plan_sweep: failed\n");
    return 1;
  }
  printf("launch_plan_sweep: ok\n");
  return 0;
}
