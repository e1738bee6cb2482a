// The host runtime's HIP-free units (glfs_amd/csrc/host.h): DevicePool and the
// job builders, stand-alone.  Built by tests/test_host_units.py with the host
// compiler under -fsanitize=address,undefined; no GPU call is made (nothing
// here instantiates a buffer or touches a stream).
#include <cstdarg>
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

template <size_t N>
static bool all_zero(const uint32_t (&w)[N]) {
  for (uint32_t x : w)
    if (x) return false;
  return true;
}

// The builders of the batch jobs: every field set, every other field zero.
static void test_batch_jobs() {
  static uint8_t src[1], ct[1], refs[1];
  static uint64_t offs[1], lens[1];
  static uint32_t status[1];
  const SmallJob s = small_job(src, ct, offs, lens, 7, 900, 512, refs);
  CHECK(s.src == src && s.ctext == ct && s.offs == offs && s.lens == lens && s.refs == refs);
  CHECK(s.n == 7 && s.max_len == 900 && s.small_max == 512);
  CHECK(all_zero(s.raw_salt) && all_zero(s.index_salt) && all_zero(s.cid_key) && !s.cid_keyed);
  CHECK(!s.hex_out && !s.hex_pos && !s.cid_wait && s.passes == 0);
  CHECK(small_job(src, nullptr, offs, lens, 1, 0, 0, refs).ctext == nullptr);
  const RaggedJob r = ragged_job(src, ct, offs, lens, 9, kRaggedAll, 1 << 20, refs);
  CHECK(r.src == src && r.ctext == ct && r.offs == offs && r.lens == lens && r.refs == refs);
  CHECK(r.n == 9 && r.lo == kRaggedAll && r.hi == 1 << 20);
  CHECK(all_zero(r.salt) && all_zero(r.cid_key) && !r.cid_keyed);
  for (uint64_t bs : {uint64_t(64), uint64_t(4096), uint64_t(1) << 20}) {
    for (uint64_t total : {uint64_t(0), uint64_t(1), bs - 1, bs, bs + 1, 3 * bs, 3 * bs + 5}) {
      const OpenJob o = open_job(ct, src, total, bs, refs, status);
      CHECK(o.ctext == ct && o.ptext == src && o.refs == refs && o.status == status);
      CHECK(o.bs == bs && o.n == (total ? total / bs + (total % bs ? 1 : 0) : 1));
      CHECK(o.last_len == total - (o.n - 1) * bs && o.last_len <= bs);
      CHECK(all_zero(o.salt) && all_zero(o.cid_key) && !o.salted && !o.cid_keyed);
    }
  }
  CHECK(open_job(ct, nullptr, 64, 64, refs, status).ptext == nullptr);
  const OpenRaggedJob g = open_ragged_job(ct, src, offs, lens, 5, 777, refs, status);
  CHECK(g.ctext == ct && g.ptext == src && g.offs == offs && g.lens == lens);
  CHECK(g.n == 5 && g.max_len == 777 && g.refs == refs && g.status == status);
  CHECK(all_zero(g.salt) && all_zero(g.cid_key) && !g.salted && !g.cid_keyed);
  static uint64_t name_offs[1], type_offs[1], sizes[1], block_sizes[1], scratch[8];
  static uint32_t modes[1];
  const TreeJob t = tree_job(3, src, name_offs, modes, ct, type_offs, refs, sizes, block_sizes,
                             scratch, 8, ct, 55);
  CHECK(t.n == 3 && t.names == src && t.name_offs == name_offs && t.modes == modes);
  CHECK(t.types == ct && t.type_offs == type_offs && t.roots == refs && t.sizes == sizes);
  CHECK(t.block_sizes == block_sizes && t.scratch == scratch && t.total == scratch + 7);
  CHECK(t.out == ct && t.cap == 55);
  CHECK(!t.line_ends && !t.hex_pos && t.prio == 0 && !t.prefix_host);
  // the read side's keys, with and without a salt and a CID key
  uint8_t salt[32], key[32];
  uint32_t salt_w[8], key_w[8], iv[8];
  for (int i = 0; i < 32; ++i) {
    salt[i] = uint8_t(0x40 + i);
    key[i] = uint8_t(5 * i + 2);
  }
  words_from_key(salt_w, salt);
  words_from_key(key_w, key);
  blake3_iv_words(iv);
  for (const uint8_t *sa : {static_cast<const uint8_t *>(nullptr), static_cast<const uint8_t *>(salt)})
    for (const uint8_t *cid : {static_cast<const uint8_t *>(nullptr),
                               static_cast<const uint8_t *>(key)}) {
      OpenJob o = open_job(ct, src, 100, 64, refs, status);
      OpenRaggedJob q = open_ragged_job(ct, src, offs, lens, 5, 777, refs, status);
      o.salted = q.salted = !sa;  // whatever was there is overwritten
      o.cid_keyed = q.cid_keyed = !cid;
      open_keys(o, sa, cid);
      open_keys(q, sa, cid);
      CHECK(o.salted == (sa != nullptr) && q.salted == (sa != nullptr));
      CHECK(o.cid_keyed == (cid != nullptr) && q.cid_keyed == (cid != nullptr));
      CHECK(memcmp(o.cid_key, cid ? key_w : iv, 32) == 0);
      CHECK(memcmp(q.cid_key, cid ? key_w : iv, 32) == 0);
      if (sa) CHECK(memcmp(o.salt, salt_w, 32) == 0 && memcmp(q.salt, salt_w, 32) == 0);
      else CHECK(all_zero(o.salt) && all_zero(q.salt));  // not read when unsalted
      CHECK(o.n == 2 && o.last_len == 36 && q.n == 5 && q.max_len == 777);  // the rest stays
    }
}

// The GLFSX_E_CORRUPT texts (fail() is runtime.cpp's: this one keeps the text).
static std::string g_text;
namespace glfsx {
namespace host {
int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_text = buf;
  return code;
}
}  // namespace host
}  // namespace glfsx

static void test_corrupt_texts() {
  CHECK(std::string(failed_checks(1)) == "failed its CID check");
  CHECK(std::string(failed_checks(2)) == "failed its DEK check");
  CHECK(std::string(failed_checks(3)) == "failed its CID and DEK checks");
  CHECK(corrupt_fail("block", 4, 70, 3, 2) == GLFSX_E_CORRUPT);
  CHECK(g_text == "block 4 of 70 failed its CID and DEK checks (2 bad in all)");
  CHECK(corrupt_fail("message", 0, 1, 1, 1) == GLFSX_E_CORRUPT);
  CHECK(g_text == "message 0 of 1 failed its CID check (1 bad in all)");
  CHECK(corrupt_fail("block", 18446744073709551615ull, 9, 2, 3) == GLFSX_E_CORRUPT);
  CHECK(g_text == "block 18446744073709551615 of 9 failed its DEK check (3 bad in all)");
}

int main() {
  test_pool();
  test_jobs();
  test_batch_jobs();
  test_corrupt_texts();
  if (g_failed) {
    fprintf(stderr, "host_units_test: %d checks failed\n", g_failed);
    return 1;
  }
  printf("host_units_test: ok\n");
  return 0;
}
