// writer_book.h -- the Writer's bookkeeping (bigblob/blob.go:120-206) as pure
// state: where the next byte goes in the batch being filled, and the stack of
// index levels with the order of their Posts.  No HIP, CPU-tested
// (tests/c/writer_book_test.cpp, the index stack against the oracle).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace glfsx {

// The fill position of the batch slot being written: `full` complete blocks
// of bs bytes and `partial` bytes of the next one, of batch_blocks at most
// (blob.go:120-133: a block is complete exactly when buffered + incoming
// reaches bs).
struct FillCursor {
  uint64_t bs = 0, batch_blocks = 1;
  uint64_t full = 0;     // complete blocks staged
  uint64_t partial = 0;  // bytes of the block being filled
  uint64_t used() const { return full * bs + partial; }
  uint64_t cap() const { return batch_blocks * bs; }  // a slot holds up to a batch
  uint64_t room() const { return cap() - used(); }
  // n <= room() more bytes are staged; true: the batch is full (submit it).
  bool add(uint64_t n) {
    const uint64_t u = used() + n;
    full = u / bs;
    partial = u % bs;
    return full == batch_blocks;
  }
  // The complete blocks are gone (submitted or posted); the partial block is
  // carried over to the front of the next staging.
  void carry() { full = 0; }
};

// The index levels of a blob being written (index.go Index per level).  A
// level's node holds only its refs (64 B each); it is zero padded to node_len
// bytes when posted (index.go:33-38), so a one-block blob never touches a
// bs-byte buffer.
//
// post(refs, present, len, out) -> int posts a node of len bytes whose first
// `present` bytes are the refs and whose remaining bytes are zero, and stores
// its ref to out; nonzero is an error, returned at once.
struct IndexStack {
  uint64_t bf = 0;        // refs per node (blob.go:107)
  uint64_t node_len = 0;  // the block size
  std::vector<std::vector<uint8_t>> levels{1};  // blob.go:111 (refs only)
  std::vector<uint64_t> counts{0};

  // blob.go:165-182 addRef
  template <class Post>
  int add(const uint8_t ref[64], Post &&post, size_t i = 0) {
    if (levels.size() <= i) {
      levels.emplace_back();
      counts.push_back(0);
    }
    levels[i].insert(levels[i].end(), ref, ref + 64);
    counts[i]++;
    if (counts[i] < bf) return 0;
    uint8_t r2[64];
    if (int e = post_node(i, r2, post)) return e;
    counts[i] = 0;
    return add(r2, post, i + 1);
  }

  // blob.go:184-206 finishIndexes: the root's ref to out.  kShouldNotHappen
  // (no value of post's): the reference's "should not happen" panic.
  static constexpr int kShouldNotHappen = 1 << 30;
  template <class Post>
  int finish(uint8_t out[64], Post &&post) {
    for (size_t i = 0; i < levels.size(); ++i) {
      if (i + 1 == levels.size()) {
        if (counts[i] == 0) return post(static_cast<const uint8_t *>(nullptr), 0, 0, out);
        if (counts[i] == 1) {
          memcpy(out, levels[i].data(), 64);
          return 0;
        }
      }
      if (counts[i] > 0) {
        uint8_t r[64];
        if (int e = post_node(i, r, post)) return e;
        if (int e = add(r, post, i + 1)) return e;
      }
    }
    return kShouldNotHappen;
  }

 private:
  template <class Post>
  int post_node(size_t i, uint8_t r[64], Post &post) {
    std::vector<uint8_t> &v = levels[i];
    const int e = post(static_cast<const uint8_t *>(v.data()), uint64_t(v.size()), node_len, r);
    v.clear();
    return e;
  }
};

}  // namespace glfsx
