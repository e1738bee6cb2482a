// writer.h -- the Writer's state and the pooled resources it is built from
// (writer.cpp).
#pragma once
#include "host.h"
#include "writer_book.h"

namespace glfsx {
namespace host __attribute__((visibility("hidden"))) {  // (per namespace body)

// ------------------------------------------------------------------ Writer
// bigblob/blob.go:71-83.  Complete blocks are staged in pinned batches and
// hashed on the GPU; Post calls and index bookkeeping then replay the
// reference's exact order (postBuf -> addRef -> maybe post index node).
//
// Two batch slots make the host round trip a pipeline: while batch k's H2D
// copy, kernels and D2H copies run on the writer's stream, the caller's
// Write()s fill batch k+1; batch k is completed (Posts delivered) when batch
// k+1 is submitted or at Finish.
struct WSlot {
  PinBuf h_in;   // complete blocks (+ the block being filled while current)
  PinBuf h_ct, h_refs;
  DevBuf d_in, d_ct, d_refs;
  Event up, hashed, done;
  uint64_t nblk = 0;  // blocks in flight
  uint64_t seq = 0;   // submission order
  PostJob job{};      // the batch's post (repeated if its fused launch failed)
  int lane = 0;       // writer lane (device + streams) the batch runs on
  bool busy = false;
  bool on_dev = false;  // the staged bytes [0, used) live in d_in, not h_in
                        // (written by glfsx_writer_write_device)
  int dev = -1;       // device of d_* (pool key)
};

// Staging of single synchronous posts (index nodes, a writer's tail block).
struct OneBuf {
  DevBuf d_in, d_ct, d_ref;
  PinBuf h_in, h_ct, h_ref;  // h_in: one-shot posts of pageable bytes
  int dev = -1;
};
// Concat's staging (glfsx_writer_write_ctext_blocks): two pinned slabs the
// copy threads gather into, the device copy of a slab, its plaintext and its
// refs.  Pooled per device like the slots: a Concat is one Writer, and
// allocating and pinning ~130 MiB for each one cost more than the hashing.
struct CtextBuf {
  PinBuf h[2];
  Event ev[2];
  DevBuf d_ctx, d_ptx, d_rfx;
  int dev = -1;
};
// A device's upload, hash and download streams.  Destroyed with their device
// current, drained, and after their split-mode scratch is dropped.
struct Streams {
  int dev = -1;
  hipStream_t up = nullptr, hash = nullptr, down = nullptr;
  Streams() = default;
  Streams(Streams &&o) noexcept { *this = std::move(o); }
  Streams &operator=(Streams &&o) noexcept {
    if (this != &o) {
      reset();
      dev = std::exchange(o.dev, -1);
      up = std::exchange(o.up, nullptr);
      hash = std::exchange(o.hash, nullptr);
      down = std::exchange(o.down, nullptr);
    }
    return *this;
  }
  ~Streams() { reset(); }
  void reset() {
    if (up || hash || down) {
      DevScope d(dev);
      for (hipStream_t st : {up, hash, down})
        if (st) {
          (void)hipStreamSynchronize(st);
          release_stream_scratch(st);
          (void)hipStreamDestroy(st);
        }
    }
    dev = -1;
    up = hash = down = nullptr;
  }
  // New streams on device d; false if one could not be made.
  bool create(int d) {
    reset();
    dev = d;
    DevScope scope(d);
    return hipStreamCreateWithFlags(&hash, hipStreamNonBlocking) == hipSuccess &&
           hipStreamCreateWithFlags(&up, hipStreamNonBlocking) == hipSuccess &&
           hipStreamCreateWithFlags(&down, hipStreamNonBlocking) == hipSuccess;
  }
  explicit operator bool() const { return hash != nullptr; }
};

// Staging slots outlive writers: glfs.PostBlob opens a Writer per blob
// (machine.go:64), and pinned/device allocation costs far more than hashing a
// small blob.  Freed writers return their slots and streams here.  The pools
// are process-wide (keyed by device), so a writer may be created, used and
// freed on different threads (a goroutine migrating between OS threads).
inline DevicePool<WSlot> &slot_pool() {
  static auto *p = new DevicePool<WSlot>(64 * 4);
  return *p;
}
inline DevicePool<OneBuf> &one_pool() {
  static auto *p = new DevicePool<OneBuf>(16);
  return *p;
}
inline DevicePool<CtextBuf> &ctext_pool() {
  static auto *p = new DevicePool<CtextBuf>(4);
  return *p;
}
inline DevicePool<Streams> &stream_pool() {
  static auto *p = new DevicePool<Streams>(64);
  return *p;
}

// A writer lane: one device with its upload, hash and download streams.
// Batches go round-robin over the lanes (glfsx_writer_set_devices), so one
// Writer fed from one host stream hashes on several GPUs at once, each over
// its own PCIe link, while the Posts still replay in block order.
struct WLane {
  int dev = 0;
  hipStream_t ws = nullptr, s_up = nullptr, s_down = nullptr;
  Streams own;  // set: streams of its own (not the writer's home streams)
};

inline void take_slot(WSlot &x, int dev, int lane) {
  x = slot_pool().take(dev);
  x.dev = dev;
  x.lane = lane;
}

inline void give_slot(WSlot &sl) {
  sl.busy = false;
  sl.nblk = 0;
  sl.on_dev = false;
  slot_pool().give(std::move(sl));  // buffers are reused by the next writer
  sl = WSlot();
}

// Streams for device dev: from the pool, or new ones.
inline bool take_streams(Streams &s, int dev) {
  s = stream_pool().take(dev);
  if (s || s.create(dev)) return true;
  s.reset();
  return false;
}

// Batch slots: one being filled, one uploading/hashing, one downloading.
// GLFSX_SLOTS (2..4) and GLFSX_BATCH_MIB override the defaults (tuning).
constexpr int kMaxSlots = 4;

}  // namespace host
}  // namespace glfsx

// A writer owns everything it touches after creation (streams, batch slots,
// single-post staging, its device id and its last error text), so it does
// not depend on the thread that created it: bigblob.Writer is
// single-goroutine (blob.go:71-83), but a goroutine may run on any OS thread
// between cgo calls.
struct glfsx_writer {
  int dev = 0;  // home device: single posts (index nodes, tail) and device input
  // batch streams: uploads, kernels (also the single posts), downloads, so
  // batch k+1's H2D overlaps batch k's D2H on the full-duplex link
  glfsx::host::Streams home;
  hipStream_t ws = nullptr, s_up = nullptr, s_down = nullptr;  // home's
  uint64_t bs = 0;
  glfsx::host::Salts salts{};
  uint8_t cid_key[32]{};
  bool has_cid_key = false;
  glfsx_post_fn post = nullptr;
  void *post_ctx = nullptr;
  glfsx::IndexStack index;    // the index levels and their Post order (writer_book.h)
  std::vector<uint8_t> node;  // an index node above kMaxMedLen, zero padded
  uint64_t size = 0;
  glfsx::host::OneBuf one;             // single posts (index nodes, the tail block)
  // device input (write_device / write_ctext): events ordering the caller's
  // stream with the upload stream, and write_ctext's staging / temporaries
  glfsx::host::Event ev_in, ev_out;
  glfsx::host::CtextBuf cx;         // write_ctext's staging (from ctext_pool; dev < 0: none yet)
  std::vector<glfsx::host::WLane> lanes;  // lane 0 = the home device and streams by default
  std::vector<glfsx::host::WSlot> slot;   // a ring: slot i runs on lane i % lanes.size()
  int nslots = 3;            // slots per lane
  int cur = 0;               // slot being filled
  uint64_t seq = 0;
  glfsx::FillCursor fill;    // where the next byte goes in slot[cur] (writer_book.h)
  uint64_t reserved = 0;     // bytes lent out by glfsx_writer_reserve
  bool strict = false;       // deliver every completed block's Post before
                             // Write returns (blob.go:120-133 error timing)
  int sticky = 0;            // first error; the writer is dead afterwards
  std::string err;           // text of the last failed call on this writer
};
