// The host runtime's HIP-free units (glfs_amd/csrc/host.h): DevicePool and the
// job builders, stand-alone.  Built by tests/test_host_units.py with the host
// compiler under -fsanitize=address,undefined; no GPU call is made (nothing
// here instantiates a buffer or touches a stream).
#include <cstdio>
#include <cstdlib>

#include "host.h"

using namespace glfsx;
using namespace glfsx::host;

// The two key-word helpers live with the kernels (post_kernels.hip), which a
// CPU program cannot link: the same definitions from the BLAKE3 spec
// (little-endian key words, section 2.1; the IV, table 1).
namespace glfsx {
void words_from_key(uint32_t w[8], const uint8_t key[32]) {
  for (int i = 0; i < 8; ++i) {
    w[i] = 0;
    for (int b = 3; b >= 0; --b) w[i] = (w[i] << 8) | key[4 * i + b];
  }
}
void blake3_iv_words(uint32_t w[8]) {
  static const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                                 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
  memcpy(w, iv, sizeof iv);
}
}  // namespace glfsx

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                    \
    }                                                                \
  } while (0)

// A pooled resource that counts: `made` real resources constructed,
// `destroyed` of them released.  A moved-from or default one is empty.
struct Res {
  static int made, destroyed;
  int dev = -1;
  int id = 0;
  Res() = default;
  Res(int dev_, int id_) : dev(dev_), id(id_) { ++made; }
  Res(Res &&o) noexcept : dev(std::exchange(o.dev, -1)), id(std::exchange(o.id, 0)) {}
  Res &operator=(Res &&o) noexcept {
    if (this != &o) {
      release();
      dev = std::exchange(o.dev, -1);
      id = std::exchange(o.id, 0);
    }
    return *this;
  }
  ~Res() { release(); }
  void release() {
    if (id) ++destroyed;
    id = 0;
    dev = -1;
  }
};
int Res::made = 0;
int Res::destroyed = 0;

static void test_pool() {
  {
    DevicePool<Res> pool(3);
    Res e = pool.take(0);  // empty pool: an empty resource
    CHECK(e.dev < 0 && e.id == 0);
    pool.give(Res(0, 1));
    pool.give(Res(1, 2));
    CHECK(pool.size() == 2 && Res::destroyed == 0);
    CHECK(pool.take(2).id == 0);  // only for the matching device
    Res b = pool.take(1);
    CHECK(b.dev == 1 && b.id == 2);  // the same resource
    CHECK(pool.take(1).id == 0);
    Res a = pool.take(0);
    CHECK(a.dev == 0 && a.id == 1);
    CHECK(pool.size() == 0 && Res::destroyed == 0);
    // a moved-from resource destroys nothing
    {
      Res m(std::move(a));
      CHECK(a.id == 0 && a.dev < 0 && m.id == 1);
      a = std::move(m);
    }
    CHECK(Res::destroyed == 0 && a.id == 1);
    pool.give(std::move(a));
    pool.give(std::move(b));
    CHECK(a.id == 0 && b.id == 0 && pool.size() == 2);
    // beyond the cap: exactly the surplus is destroyed, what was pooled stays
    pool.give(Res(0, 3));
    CHECK(pool.size() == 3 && Res::destroyed == 0);
    pool.give(Res(0, 4));
    pool.give(Res(1, 5));
    CHECK(pool.size() == 3 && Res::destroyed == 2);
    CHECK(pool.take(0).id == 3);  // the last one pooled for the device first
    CHECK(Res::destroyed == 3);   // (the temporary just taken)
    // a resource of no device is not pooled
    pool.give(Res(-1, 6));
    CHECK(pool.size() == 2 && Res::destroyed == 4);
    // the counts balance but for what the pool still holds
    CHECK(Res::made == 6 && Res::made - Res::destroyed == int(pool.size()));
  }
  CHECK(Res::made == Res::destroyed);
}

static void test_jobs() {
  static uint8_t src[1], ct[1], refs[1];
  const uint64_t sizes[] = {128, 1000, 1ull << 20};
  for (uint64_t bs : sizes) {
    const uint64_t totals[] = {0, 1, bs - 1, bs, bs + 1, 3 * bs, 3 * bs + 5};
    for (uint64_t total : totals) {
      const uint64_t n = total / bs + (total % bs ? 1 : 0);
      const PostJob j = block_job(src, total, bs, ct, dense_refs(refs));
      CHECK(j.src == src && j.ctext == ct && j.out.refs == refs);
      CHECK(j.n == n);
      CHECK(j.last_len == (n ? total - (n - 1) * bs : 0));
      CHECK(j.stride == bs && j.msg_len == bs);
      CHECK(j.out.bf == UINT64_MAX && j.out.stride == 0);
      const PostJob k = block_job(src, total, bs, nullptr, node_refs(refs, bs));
      CHECK(k.ctext == nullptr && k.n == n && k.out.refs == refs);
      CHECK(k.out.bf == bs / 64 && k.out.stride == bs);
      const PostJob s = single_job(src, total, ct, refs);
      CHECK(s.src == src && s.ctext == ct && s.out.refs == refs);
      CHECK(s.n == 1 && s.stride == 0 && s.msg_len == total && s.last_len == total);
      CHECK(s.out.bf == UINT64_MAX && s.out.stride == 0);
    }
  }
  uint8_t salt[32], key[32];
  uint32_t salt_w[8], key_w[8], iv[8];
  for (int i = 0; i < 32; ++i) {
    salt[i] = uint8_t(0x80 + i);
    key[i] = uint8_t(3 * i + 1);
  }
  for (int i = 0; i < 8; ++i) {
    salt_w[i] = uint32_t(salt[4 * i]) | uint32_t(salt[4 * i + 1]) << 8 |
                uint32_t(salt[4 * i + 2]) << 16 | uint32_t(salt[4 * i + 3]) << 24;
    key_w[i] = uint32_t(key[4 * i]) | uint32_t(key[4 * i + 1]) << 8 |
               uint32_t(key[4 * i + 2]) << 16 | uint32_t(key[4 * i + 3]) << 24;
  }
  blake3_iv_words(iv);
  Salts salts;
  memcpy(salts.raw, salt, 32);
  memcpy(salts.index, key, 32);
  for (const uint8_t *cid : {static_cast<const uint8_t *>(nullptr),
                             static_cast<const uint8_t *>(key)}) {
    const uint32_t *want = cid ? key_w : iv;
    PostJob p{};
    OneDesc d{};
    SmallJob s{};
    p.cid_keyed = !cid;  // whatever was there is overwritten
    d.cid_keyed = !cid;
    s.cid_keyed = !cid;
    set_keys(p, salt, cid);
    set_keys(d, salt, cid);
    set_keys(s, salts, cid);
    CHECK(memcmp(p.salt, salt_w, 32) == 0 && memcmp(d.salt, salt_w, 32) == 0);
    CHECK(memcmp(s.raw_salt, salt_w, 32) == 0 && memcmp(s.index_salt, key_w, 32) == 0);
    CHECK(memcmp(p.cid_key, want, 32) == 0);
    CHECK(memcmp(d.cid_key, want, 32) == 0);
    CHECK(memcmp(s.cid_key, want, 32) == 0);
    CHECK(p.cid_keyed == (cid != nullptr));
    CHECK(d.cid_keyed == (cid ? 1u : 0u));
    CHECK(s.cid_keyed == (cid != nullptr));
  }
}

int main() {
  test_pool();
  test_jobs();
  if (g_failed) {
    fprintf(stderr, "host_units_test: %d checks failed\n", g_failed);
    return 1;
  }
  printf("host_units_test: ok\n");
  return 0;
}
