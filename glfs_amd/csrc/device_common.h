// device_common.h -- device definitions shared by the kernel translation
// units (post_kernels.hip, tree_kernels.hip, xof_kernels.hip): the BLAKE3 IV
// and domain flags, the hex digits of a tree line, and the synthetic-data
// generator.  A stand-alone header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glfsx {
namespace {

constexpr uint32_t kIV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u,
                             0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu,
                             0x1F83D9ABu, 0x5BE0CD19u};
enum : uint32_t {
  kChunkStart = 1,
  kChunkEnd = 2,
  kParent = 4,
  kRoot = 8,
  kKeyed = 16,
};

// Lower-case hex digits of bytes 0 and 1 of x, in output order (hi(b0)
// lo(b0) hi(b1) lo(b1)) as one little-endian word: '0' + n, or 'a' - 10 + n.
__device__ __forceinline__ uint32_t hex4(uint32_t x) {
  const uint32_t n = ((x >> 4) & 0xFu) | ((x & 0xFu) << 8) |
                     ((x >> 12) & 0xFu) << 16 | ((x >> 8) & 0xFu) << 24;
  const uint32_t ge10 = ((n + 0x06060606u) >> 4) & 0x01010101u;  // nibble >= 10
  return n + 0x30303030u + ge10 * 39u;
}

// splitmix64: byte o of synthetic data = byte (o & 7) of a word of it.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

}  // namespace
}  // namespace glfsx
