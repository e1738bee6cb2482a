// copy_pool.cpp -- host copies into pinned staging over persistent copy
// threads, one pool per NUMA node.
#include <cctype>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <pthread.h>
#include <sched.h>
#include <thread>

#include "host.h"

namespace glfsx {
namespace host {
namespace {

// Host copy into pinned staging; large copies are split over a persistent
// pool of copy threads (the Writer's memcpy into w.buf, blob.go:121-126, is
// its host-side cost: one core copies ≈25 GB/s, a 1 MiB PostBlob spent ≈40
// µs here).  Pieces of >= 256 KiB; the caller copies one piece itself and
// spins until the pool has done the rest.  Workers are started on first use
// (up to 15: the GPU box's share is 16 cores) and live for the process.
struct CopyTask {
  uint8_t *dst;
  const uint8_t *src;
  size_t n;
  std::atomic<int> *left;
  // read_at != nullptr: read n bytes at input offset `off` into dst instead
  // (glfsx_writer_read_at); *got = bytes read, or a negative status
  glfsx_read_at_fn read_at = nullptr;
  void *rctx = nullptr;
  uint64_t off = 0;
  int64_t *got = nullptr;
  // blocks != nullptr: gather nblk blocks (bsz bytes each, the last lastn)
  // into dst back to back instead (gather_start)
  const void *const *blocks = nullptr;
  uint64_t nblk = 0, bsz = 0, lastn = 0;
};
void gather_blocks(uint8_t *dst, const void *const *blocks, uint64_t k, uint64_t bs,
                   uint64_t last) {
  for (uint64_t i = 0; i < k; ++i)
    memcpy(dst + i * bs, blocks[i], i + 1 == k ? last : bs);
}

// Read n bytes at offset off through fn, repeating short reads; stops early
// only at the end of the input (fn returns 0) or on an error (< 0).
int64_t read_full(glfsx_read_at_fn fn, void *ctx, uint8_t *dst, uint64_t n, uint64_t off) {
  uint64_t done = 0;
  while (done < n) {
    const int64_t r = fn(ctx, dst + done, n - done, off + done);
    if (r < 0) return r;
    if (r == 0) break;
    done += uint64_t(r);
  }
  return int64_t(done);
}
struct CopyPool {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<CopyTask> q;
  unsigned workers = 0;
  void run() {
    for (;;) {
      CopyTask t;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !q.empty(); });
        t = q.back();
        q.pop_back();
      }
      if (t.blocks)
        gather_blocks(t.dst, t.blocks, t.nblk, t.bsz, t.lastn);
      else if (t.read_at)
        *t.got = read_full(t.read_at, t.rctx, t.dst, t.n, t.off);
      else
        memcpy(t.dst, t.src, t.n);
      t.left->fetch_sub(1, std::memory_order_release);
    }
  }
};
// The NUMA node device `dev` hangs off (sysfs of its PCI function), or -1.
int device_numa_node(int dev) {
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, int(sizeof bdf) - 1, dev) != hipSuccess) return -1;
  for (char *q = bdf; *q; ++q) *q = char(tolower(*q));
  int node = -1;
  if (FILE *f = fopen((std::string("/sys/bus/pci/devices/") + bdf + "/numa_node").c_str(), "r")) {
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
  }
  return node;
}

// The CPUs of NUMA node `node` within this process's affinity; false if
// unknown or none.
bool node_cpus(int node, cpu_set_t *set) {
  if (node < 0) return false;
  char path[96];
  snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
  FILE *f = fopen(path, "r");
  if (!f) return false;
  cpu_set_t mine;
  CPU_ZERO(set);
  if (sched_getaffinity(0, sizeof mine, &mine) != 0) {
    fclose(f);
    return false;
  }
  int lo = 0, hi = 0;
  char sep = 0;
  while (fscanf(f, "%d", &lo) == 1) {  // "0-63,128-191"
    hi = lo;
    if (fscanf(f, "%c", &sep) == 1 && sep == '-') {
      if (fscanf(f, "%d", &hi) != 1) break;
      if (fscanf(f, "%c", &sep) != 1) sep = 0;
    }
    for (int c = lo; c <= hi && c < CPU_SETSIZE; ++c)
      if (CPU_ISSET(c, &mine)) CPU_SET(c, set);
    if (sep != ',') break;
  }
  fclose(f);
  return CPU_COUNT(set) > 0;
}

// One copy pool per NUMA node, used for the staging of a device on that
// node: its threads run on the node's CPUs (GLFSX_NUMA=0: one unbound pool
// for every device), so their copies and reads land in pinned staging the
// device's DMA engines read -- a file read from the device's node ran 27-29
// -> 35-38 GiB/s on a two-socket box (bench file_feed).
// A process driving GPUs on both sockets (glfsx_create_devices, a Writer
// over several lanes) gets a pool on each (one process-wide pool
// bound to the first device's node served the other socket's GPUs from the
// wrong node).
bool numa_binding() {
  static const bool on = [] {
    const char *e = getenv("GLFSX_NUMA");
    return !e || atoi(e) != 0;
  }();
  return on;
}

CopyPool &copy_pool(int dev = -1) {
  static std::mutex mu;
  static std::vector<std::pair<int, CopyPool *>> pools;  // (node, pool), process lifetime
  static std::vector<int> dev_node;                      // device -> node (-2: unknown yet)
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::lock_guard<std::mutex> lk(mu);
  int node = -1;
  if (numa_binding()) {
    if (size_t(dev) >= dev_node.size()) dev_node.resize(dev + 1, -2);
    if (dev_node[dev] == -2) dev_node[dev] = device_numa_node(dev);
    node = dev_node[dev];
  }
  for (auto &p : pools)
    if (p.first == node) return *p.second;
  auto *cp = new CopyPool();
  const unsigned hw = std::thread::hardware_concurrency();
  cp->workers = std::min(15u, hw > 1 ? hw - 1 : 0u);
  cpu_set_t cpus;
  const bool bind = node_cpus(node, &cpus);
  for (unsigned i = 0; i < cp->workers; ++i)
    std::thread([cp, bind, cpus] {
      if (bind) (void)pthread_setaffinity_np(pthread_self(), sizeof cpus, &cpus);
      cp->run();
    }).detach();
  pools.push_back({node, cp});
  return *cp;
}

}  // namespace

// dev: the device whose staging dst is (-1: the current device), which
// picks the copy pool of its NUMA node.
void par_memcpy(uint8_t *dst, const uint8_t *src, size_t n, int dev) {
  constexpr size_t kPiece = 256u << 10;
  if (n < 2 * kPiece) {
    memcpy(dst, src, n);
    return;
  }
  CopyPool &P = copy_pool(dev);
  const size_t parts = std::min<size_t>(P.workers + 1, n / kPiece);
  if (parts <= 1) {
    memcpy(dst, src, n);
    return;
  }
  const size_t per = (n / parts + 4095) & ~size_t(4095);
  std::atomic<int> left{0};
  {
    std::lock_guard<std::mutex> lk(P.mu);
    for (size_t o = per; o < n; o += per) {
      left.fetch_add(1, std::memory_order_relaxed);
      P.q.push_back({dst + o, src + o, std::min(per, n - o), &left});
    }
  }
  P.cv.notify_all();
  memcpy(dst, src, std::min(per, n));
  while (left.load(std::memory_order_acquire) > 0) sched_yield();
}

// k blocks (bs bytes each, the last `last`) from scattered addresses into
// dst back to back, asynchronously (Concat's slabs, straight from the
// store's memory into pinned staging): every part goes to the copy pool and *left counts the parts not yet copied; the caller goes
// on (uploads, decrypts and hashes the previous slab) and waits with
// gather_wait before it reads dst.  Blocks are copied in runs of consecutive
// blocks per task, or -- fewer blocks than threads -- in pieces of >= 1 MiB.
void gather_start(std::atomic<int> *left, uint8_t *dst, const void *const *blocks,
                  uint64_t k, uint64_t bs, uint64_t last, int dev) {
  if (k == 0) return;
  CopyPool &P = copy_pool(dev);
  const uint64_t total = (k - 1) * bs + last;
  if (P.workers == 0) {
    gather_blocks(dst, blocks, k, bs, last);
    return;
  }
  const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>(P.workers, total >> 20));
  {
    std::lock_guard<std::mutex> lk(P.mu);
    if (k >= parts) {
      const uint64_t per = (k + parts - 1) / parts;
      for (uint64_t b = 0; b < k; b += per) {
        const uint64_t m = std::min(per, k - b);
        CopyTask t{};
        t.dst = dst + b * bs;
        t.left = left;
        t.blocks = blocks + b;
        t.nblk = m;
        t.bsz = bs;
        t.lastn = b + m == k ? last : bs;
        left->fetch_add(1, std::memory_order_relaxed);
        P.q.push_back(t);
      }
    } else {
      const uint64_t pieces = (parts + k - 1) / k;
      for (uint64_t i = 0; i < k; ++i) {
        const uint64_t n = i + 1 == k ? last : bs;
        const uint64_t per = std::max<uint64_t>(1, ((n / pieces) + 4095) & ~uint64_t(4095));
        for (uint64_t o = 0; o < n; o += per) {
          left->fetch_add(1, std::memory_order_relaxed);
          P.q.push_back({dst + i * bs + o, static_cast<const uint8_t *>(blocks[i]) + o,
                         size_t(std::min(per, n - o)), left});
        }
      }
    }
  }
  P.cv.notify_all();
}

void gather_wait(std::atomic<int> *left) {
  while (left->load(std::memory_order_acquire) > 0) sched_yield();
}

// Read n bytes of input at offset off into dst with the copy pool's threads
// (pieces of >= 4 MiB, the caller reading the first): an io.ReaderAt / a
// file read by several threads at once, as a page-cache copy is one core's
// memcpy.  Returns the bytes of the contiguous prefix read (< n only at the
// end of the input) or the first piece's error (negative).
int64_t par_read_at(glfsx_read_at_fn fn, void *ctx, uint8_t *dst, uint64_t n, uint64_t off,
                    unsigned max_threads, int dev) {
  constexpr uint64_t kPiece = 4ull << 20;
  CopyPool &P = copy_pool(dev);
  const uint64_t parts = std::max<uint64_t>(
      1, std::min<uint64_t>({uint64_t(P.workers) + 1, uint64_t(max_threads), n / kPiece}));
  if (parts <= 1) return read_full(fn, ctx, dst, n, off);
  const uint64_t per = (n / parts + 4095) & ~uint64_t(4095);
  std::vector<int64_t> got((n + per - 1) / per, 0);
  std::atomic<int> left{0};
  {
    std::lock_guard<std::mutex> lk(P.mu);
    for (uint64_t o = per, k = 1; o < n; o += per, ++k) {
      left.fetch_add(1, std::memory_order_relaxed);
      CopyTask t{dst + o, nullptr, size_t(std::min(per, n - o)), &left};
      t.read_at = fn;
      t.rctx = ctx;
      t.off = off + o;
      t.got = &got[k];
      P.q.push_back(t);
    }
  }
  P.cv.notify_all();
  got[0] = read_full(fn, ctx, dst, std::min(per, n), off);
  while (left.load(std::memory_order_acquire) > 0) sched_yield();
  uint64_t total = 0;
  for (uint64_t k = 0; k < got.size(); ++k) {
    if (got[k] < 0) return got[k];
    total += uint64_t(got[k]);
    if (uint64_t(got[k]) < std::min(per, n - k * per)) break;  // end of input
  }
  return int64_t(total);
}

}  // namespace host
}  // namespace glfsx
