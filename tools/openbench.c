/* Per-call latency of the verified read of ONE block (scripts/one_open_lat.py):
 * one plain C thread calling the C-ABI, per size
 *   open       glfsx_open, route 0 (k_one_open up to 64 KiB, staged above)
 *   staged     glfsx_open, route 1 (every size through device staging)
 *   batch1     glfsx_open_batch with one block of the same bytes (what a
 *              caller had before glfsx_open: the slab pipeline)
 *   xor        glfsx_chacha20_xor (the unchecked getF)
 *   post       glfsx_post of the same plaintext (k_one / k_med / staged)
 * `reps` interleaved repetitions of `calls` timed calls each in one process,
 * after a warm-up of every variant.  Every timed open must return status 0
 * and the right plaintext.  Measurement harness only -- not part of the
 * library.  The library comes in by path (dlopen), so the program also runs
 * under a profiler as it is.
 *
 *   openbench LIB [reps [calls [size ...]]]
 * prints one JSON object: {"reps":..,"calls":..,"results":[{"size":..,
 * "variant":..,"p50_us":..,"p90_us":..,"n":..}, ...]}.  Exit status 0, or 1
 * with a message on stderr. */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../include/glfsx.h"

typedef int (*open_fn)(const uint8_t *, const uint8_t *, const uint8_t *, const void *, uint64_t,
                       void *, uint32_t *);
typedef int (*batch_fn)(const uint8_t *, const uint8_t *, const void *, uint64_t, uint64_t,
                        const uint8_t *, void *, uint32_t *, uint64_t *);
typedef int (*xor_fn)(const uint8_t *, const void *, void *, uint64_t);
typedef int (*post_fn)(const uint8_t *, const void *, uint64_t, void *, uint8_t *,
                       const uint8_t *);
typedef int (*route_fn)(int);
typedef const char *(*err_fn)(void);

static open_fn open_p;
static batch_fn batch_p;
static xor_fn xor_p;
static post_fn post_p;
static route_fn route_p;
static err_fn err_p;

enum { V_OPEN, V_STAGED, V_BATCH1, V_XOR, V_POST, V_COUNT };
static const char *const kNames[V_COUNT] = {"open", "staged", "batch1", "xor", "post"};

static double now(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

static int cmp(const void *a, const void *b) {
  const double x = *(const double *)a, y = *(const double *)b;
  return x < y ? -1 : x > y;
}

typedef struct {
  uint64_t n;
  uint8_t *pt, *ct, *out, *ct2;
  uint8_t ref[64], ref2[64];
} msg;

static const uint8_t kSalt[32] = {1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,
                                  17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32};

/* One call of variant v on m; 0, or a message on stderr and 1. */
static int call(int v, msg *m) {
  uint32_t st = 0x5a5a5a5au;
  int rc = 0;
  switch (v) {
    case V_OPEN:
    case V_STAGED:
      rc = open_p(kSalt, NULL, m->ref, m->ct, m->n, m->out, &st);
      if (!rc && (st != 0 || memcmp(m->out, m->pt, m->n) != 0)) rc = -100;
      break;
    case V_BATCH1:
      if (m->n == 0) return 0; /* total == 0 is a no-op there */
      rc = batch_p(kSalt, NULL, m->ct, m->n, (m->n + 63) & ~(uint64_t)63, m->ref, m->out, &st,
                   NULL);
      if (!rc && (st != 0 || memcmp(m->out, m->pt, m->n) != 0)) rc = -100;
      break;
    case V_XOR:
      rc = xor_p(m->ref + 32, m->ct, m->out, m->n);
      break;
    case V_POST:
      rc = post_p(kSalt, m->pt, m->n, m->ct2, m->ref2, NULL);
      if (!rc && memcmp(m->ref2, m->ref, 64) != 0) rc = -100;
      break;
  }
  if (rc) {
    fprintf(stderr, "openbench: %s at %llu bytes failed: %d (%s)\n", kNames[v],
            (unsigned long long)m->n, rc, rc == -100 ? "wrong result" : err_p());
    return 1;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: openbench LIB [reps [calls [size ...]]]\n");
    return 1;
  }
  void *h = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
  if (!h) {
    fprintf(stderr, "openbench: %s\n", dlerror());
    return 1;
  }
  open_p = (open_fn)dlsym(h, "glfsx_open");
  batch_p = (batch_fn)dlsym(h, "glfsx_open_batch");
  xor_p = (xor_fn)dlsym(h, "glfsx_chacha20_xor");
  post_p = (post_fn)dlsym(h, "glfsx_post");
  route_p = (route_fn)dlsym(h, "glfsx_set_open_route");
  err_p = (err_fn)dlsym(h, "glfsx_last_error");
  if (!open_p || !batch_p || !xor_p || !post_p || !route_p || !err_p) {
    fprintf(stderr, "openbench: the library lacks an entry point\n");
    return 1;
  }
  const int reps = argc > 2 ? atoi(argv[2]) : 3;
  const int calls = argc > 3 ? atoi(argv[3]) : 200;
  static const uint64_t kDefault[] = {0, 1024, 4096, 16384, 65536, 1u << 20, 2u << 20};
  uint64_t sizes[32];
  int ns = 0;
  for (int i = 4; i < argc && ns < 32; i++) sizes[ns++] = strtoull(argv[i], NULL, 10);
  if (ns == 0)
    for (; ns < (int)(sizeof kDefault / sizeof *kDefault); ns++) sizes[ns] = kDefault[ns];
  if (reps < 1 || calls < 1) return 1;

  msg *ms = (msg *)calloc(ns, sizeof *ms);
  double *lat = (double *)calloc((size_t)ns * V_COUNT * reps * calls, sizeof *lat);
  for (int s = 0; s < ns; s++) {
    msg *m = &ms[s];
    m->n = sizes[s];
    m->pt = (uint8_t *)malloc(m->n + 64);
    m->ct = (uint8_t *)malloc(m->n + 64);
    m->ct2 = (uint8_t *)malloc(m->n + 64);
    m->out = (uint8_t *)malloc(m->n + 64);
    for (uint64_t i = 0; i < m->n; i++) m->pt[i] = (uint8_t)(i * 131 + 7 * s + (i >> 9));
    if (post_p(kSalt, m->pt, m->n, m->ct, m->ref, NULL)) {
      fprintf(stderr, "openbench: glfsx_post: %s\n", err_p());
      return 1;
    }
  }
  /* warm-up: every variant at every size (contexts, staging, code objects) */
  for (int s = 0; s < ns; s++)
    for (int v = 0; v < V_COUNT; v++) {
      route_p(v == V_STAGED ? 1 : 0);
      for (int i = 0; i < 20; i++)
        if (call(v, &ms[s])) return 1;
    }
  for (int r = 0; r < reps; r++)
    for (int s = 0; s < ns; s++)
      for (int v = 0; v < V_COUNT; v++) {
        route_p(v == V_STAGED ? 1 : 0);
        double *l = lat + (((size_t)s * V_COUNT + v) * reps + r) * calls;
        for (int i = 0; i < calls; i++) {
          const double t = now();
          if (call(v, &ms[s])) return 1;
          l[i] = now() - t;
        }
      }
  route_p(0);
  printf("{\"reps\": %d, \"calls\": %d, \"results\": [", reps, calls);
  for (int s = 0; s < ns; s++)
    for (int v = 0; v < V_COUNT; v++) {
      const size_t n = (size_t)reps * calls;
      double *l = lat + ((size_t)s * V_COUNT + v) * n;
      qsort(l, n, sizeof *l, cmp);
      printf("%s\n {\"size\": %llu, \"variant\": \"%s\", \"p50_us\": %.2f, \"p90_us\": %.2f, "
             "\"n\": %zu}",
             s + v ? "," : "", (unsigned long long)sizes[s], kNames[v], l[n / 2] * 1e6,
             l[n * 9 / 10] * 1e6, n);
    }
  printf("\n]}\n");
  return 0;
}
