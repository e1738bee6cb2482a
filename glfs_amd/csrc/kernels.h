// kernels.h -- internal interface between the host runtime (host.h and its
// units: runtime, oneshot, copy_pool, writer, create, blobs, read) and the
// gfx950 kernels: post_kernels.hip (the launches, with its fragments b3_arx.h,
// pass_kernels.h, quad_kernels.h, one_kernels.h, one_open_kernels.h,
// small_kernels.h, ragged_kernels.h, read_kernels.h, open_kernels.h and
// ragged_open_kernels.h holding the kernels by family; ragged_groups.h the
// host form's grouping, launch_plan.h every choice of kernel and launch shape
// as pure functions that the host half obeys, launch_log.h the record of such
// a choice, stream_scratch.h the per-stream scratch: free of device code),
// tree_kernels.hip and xof_kernels.hip (device_common.h: definitions the
// three share).  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "one_classes.h"

namespace glfsx {

// Where ref j of a pass lands: refs + (j / ref_bf) * ref_stride + (j % ref_bf) * 64.
// Dense output: ref_bf = UINT64_MAX, ref_stride = 0.  Index-node output:
// ref_bf = bf, ref_stride = block_size (bigblob/index.go:33-38: slot i of a
// node is bytes [64i, 64i+64), the rest of the node stays zero).
struct RefLayout {
  uint8_t *refs;
  uint64_t bf;
  uint64_t stride;
};

// One "post" of n equal messages (the last one possibly short) laid out at
// src + j*stride: DEK pass then ChaCha20+CID pass (bigblob/ref.go:98-161).
struct PostJob {
  const uint8_t *src;
  uint8_t *ctext;       // nullable; may alias src
  uint64_t stride;      // bytes between message starts
  uint64_t msg_len;     // length of messages 0..n-2
  uint64_t last_len;    // length of message n-1
  uint64_t n;           // number of messages (>= 1)
  RefLayout out;
  uint32_t salt[8];     // DEK key words (little-endian words of the salt)
  uint32_t cid_key[8];  // CID key words (IV when unkeyed)
  bool cid_keyed;
};

// Largest message (bigblob block or index node) the post kernels accept:
// 256 workgroups x 256 lanes x 64 BLAKE3 chunks (split mode, 4 GiB).
constexpr uint64_t kMaxMsgLen = 256ull * 256 * 64 * 1024;

// fused = false: never the one-launch split form (k_pass_dc), for callers
// that return before the stream is synchronised (its failure is only
// visible to fused_errors_take after the stream has drained).
hipError_t launch_post(const PostJob &job, hipStream_t s, bool fused = true);

// After stream s has drained: nonzero when a one-launch split post on it
// gave up waiting for a DEK since the last call (its refs and ctext are
// invalid; the caller fails or repeats the post with fused = false).
uint32_t fused_errors_take(hipStream_t s);
// Test hooks: the next fused launch leaves message skip_msg's ready flag
// unset (~0u: none); wait_us bounds the DEK wait (0: the 1 s default).
void fused_debug(uint32_t skip_msg, uint64_t wait_us);
// Timeouts seen by fused_errors_take so far (process-wide).
uint64_t fused_timeouts();
// The bulk passes' clock probe on the current device (k_pass): out[0] =
// shader-clock cycles, out[1] = 100 MHz ticks summed over every k_pass
// workgroup since the last reset; reset: zero them after reading.
// Synchronous (waits for the device).
hipError_t clock_probe(int reset, uint64_t out[2]);
// The launch log (launch_log.h), on from the first call: the first min(cap,
// kept) records of the bulk launches (k_pass, k_quad, k_pass_dc, k_open)
// since the last reset to out, kLaunchRecWords words each; returns how many
// were launched since then.  reset: empty the log after reading.  No HIP call.
size_t pass_log(int reset, uint32_t *out, size_t cap);
// The same for the aux log: the small-blob launches (k_small, k_small_q), the
// decrypt launches (k_decrypt_lines, k_decrypt), the levels of the ragged
// passes and the one-shot classes.
size_t aux_log(int reset, uint32_t *out, size_t cap);

// The second half of launch_post alone: ChaCha20 keyed by the DEK already in
// bytes [32,64) of each ref slot, ctext store, CID into bytes [0,32).
hipError_t launch_cid_pass(const PostJob &job, hipStream_t s);

// DEK-only pass (keyed BLAKE3, first 32 XOF bytes) over the same layout,
// writing 32-byte digests to out (at byte offset `out_off` of each ref slot).
hipError_t launch_keyed_hash(const PostJob &job, uint32_t out_off,
                             hipStream_t s);

// ChaCha20 XOR (zero nonce, counter 0) of n bytes with key words k.
hipError_t launch_chacha_xor(const uint32_t k[8], const uint8_t *src,
                             uint8_t *dst, uint64_t n, hipStream_t s);

// Many small blobs, one lane each (glfs.PostBlob batched): blob i is
// src[offs[i] .. offs[i]+lens[i]); if lens[i] <= kMaxSmallLen its root ref
// (CID || DEK) goes to refs + 64*i (empty blobs use index_salt); longer blobs
// are skipped (the caller posts them).
constexpr uint64_t kMaxSmallLen = 16ull * 1024;
// entries per workgroup of the tree-line kernels (tree_kernels.hip)
constexpr uint32_t kTreeWG = 256;
struct SmallJob {
  const uint8_t *src;
  uint8_t *ctext;  // nullable; same offsets as src
  const uint64_t *offs, *lens;  // device arrays
  uint64_t n, max_len;
  uint8_t *refs;
  uint32_t raw_salt[8], index_salt[8], cid_key[8];
  bool cid_keyed;
  // blobs of at most small_max bytes are hashed here: min(kMaxSmallLen,
  // the blob block size) -- a longer blob has several blocks and an index
  // node (blob.go:120-206), so the caller Creates it (0 = kMaxSmallLen)
  uint64_t small_max;
  // hex_out != nullptr: the CID pass also writes blob i's root as the tree
  // line's hex fields -- 64 lower-case digits of the CID at hex_out +
  // hex_pos[i] and of the DEK kDekAfterCid bytes later (TreeJob::hex_pos)
  uint8_t *hex_out;
  const uint64_t *hex_pos;
  hipEvent_t cid_wait;  // nullable: the CID pass waits for it (after the DEK pass)
  uint32_t passes;      // 1: the DEK pass only, 2: the CID pass only, 0: both
};

// The small route's limit for blobs of block size bs.
inline uint64_t small_max_for(uint64_t bs) { return bs < kMaxSmallLen ? bs : kMaxSmallLen; }
hipError_t launch_post_small(const SmallJob &job, hipStream_t s);

// Many messages of unequal length in throughput form (ragged_kernels.h):
// message i is src[offs[i] .. offs[i]+lens[i]); if lo < lens[i] <= hi its ref
// (CID || DEK, the DEK keyed by salt as given) goes to refs + 64*i and its
// ciphertext to ctext at the same offset; the other messages are skipped and
// their ref slots left alone (lo = kRaggedAll: no lower bound, the empty
// message included).  Work is handed out by BLAKE3 chunk, so it follows the
// bytes, not n x the longest message; a fixed number of launches whatever n
// (a plan of two, then at most three per pass) and one host wait, for the
// plan's totals.  hi <= kMaxRaggedLen.
constexpr uint64_t kMaxRaggedLen = 16ull << 20;
constexpr uint64_t kRaggedAll = ~0ull;
struct RaggedJob {
  const uint8_t *src;
  uint8_t *ctext;  // nullable; same offsets as src; may be src
  const uint64_t *offs, *lens;  // device arrays
  uint64_t n;
  uint64_t lo, hi;
  uint8_t *refs;
  uint32_t salt[8], cid_key[8];
  bool cid_keyed;
};
hipError_t launch_post_ragged(const RaggedJob &job, hipStream_t s);

// One-shot posts (ref.go:98-161 for one message of at most kMaxOneLen bytes:
// a glfs.PostBlob of a small blob, a Writer's tail block, an index node of a
// small-block blob): DEK, ChaCha20 and CID in one launch, one workgroup per
// descriptor.  src / ctext / ref may be pinned host memory (device pointers
// of it): the kernel reads the message once and writes ctext and ref
// straight into the caller's staging, so a post is one launch and a wait.
// Messages of kMaxOneLen < len <= kMaxMedLen (one_classes.h) take two launches
// (the medium pair: one workgroup per 64 KiB span, the last-arriving one
// merges) and need the device scratch below.
struct OneDesc {
  const uint8_t *src;  // 16-B aligned, device-accessible
  uint8_t *ctext;      // nullable, device-accessible, 16-B aligned
  uint8_t *ref;        // 64 B out: CID || DEK, 4-B aligned
  uint32_t len;        // <= kMaxMedLen
  uint32_t present;    // bytes [present, len) of the message are zero (not read)
  uint32_t cid_keyed;
  uint32_t salt[8];     // DEK key words
  uint32_t cid_key[8];  // CID key words (IV when unkeyed)
  // the medium pair only (device memory): the staged message (len rounded up to
  // 64 B), 8 words per 64 KiB span, an arrival counter (zero before the
  // launch, left at zero) and the DEK
  uint8_t *dmsg;
  uint32_t *cvs, *cnt, *dek;
  // nullable, pinned host memory: set to seq (release, system scope) once
  // ctext and ref are in the caller's staging
  uint32_t *flag;
  uint32_t seq;
};

// One-shot verified read (one_open_kernels.h; ref.go:113-126 getF with its
// checks for one block of at most kMaxOneLen bytes): one workgroup stages the
// ctext from the caller's pinned staging, decrypts it with the ref's DEK and
// hashes ctext and plaintext side by side; *status = 1 (CID mismatch) | 2
// (DEK mismatch), 0 when good, written every time; the plaintext is written
// either way.  The salted form (class kOneOpenSalted) checks both, the
// other one the CID alone (salt is not read, bit 1 never set).  A type of
// its own: k_one stages OneDesc into LDS by word count.
struct OneOpenDesc {
  const uint8_t *src;  // the ctext: 16-B aligned, device-accessible
  uint8_t *ptext;      // nullable (check only), device-accessible, 16-B aligned
  uint32_t *status;    // one word out, 4-B aligned
  uint32_t ref[16];    // the ref's words: CID then DEK
  uint32_t len;        // <= kMaxOneLen
  uint32_t cid_keyed;
  uint32_t salt[8];     // DEK key words (the salted form)
  uint32_t cid_key[8];  // CID key words (IV when unkeyed)
  // as OneDesc's: set to seq once status and plaintext are in place
  uint32_t *flag;
  uint32_t seq;
};
// One launch (the medium class: its pair) over the n requests of one-shot
// class c (one_classes.h), as launch_plan.h's one_rec says: h and d are the
// host's and the device's view of their n descriptors in pinned memory, max_len
// bounds their len.  One request goes to the kernel by value, from *h.  n == 0
// launches nothing; a length the class does not take is hipErrorInvalidValue.
hipError_t launch_one_class(OneClass c, const OneDesc *h, const OneDesc *d, uint32_t n,
                            uint64_t max_len, hipStream_t s);
hipError_t launch_one_class(OneClass c, const OneOpenDesc *h, const OneOpenDesc *d, uint32_t n,
                            uint64_t max_len, hipStream_t s);

// Read side: decrypt n contiguous blocks (bs % 64 == 0; the last one
// last_len bytes) with the DEKs in bytes [32,64) of refs[j] (dense).
hipError_t launch_decrypt(const uint8_t *ctext, uint8_t *ptext, uint64_t n,
                          uint64_t bs, uint64_t last_len, const uint8_t *refs,
                          hipStream_t s);

// Read side with the checks (open_kernels.h): block j of n contiguous blocks
// (bs % 64 == 0, bs <= kMaxMsgLen; the last one last_len bytes) is checked
// against refs[j] -- its ctext must hash to the CID and, when salted, its
// plaintext (ChaCha20 with the ref's DEK) to the DEK under `salt` as given --
// and decrypted to ptext when that is set.  status[j] (every j < n, no
// pre-zeroing) = 1 (CID mismatch) | 2 (DEK mismatch), 0 when both match; the
// plaintext is written either way.  Two routes with the same results: k_open
// (one pass, one workgroup per block: salted, bs <= 2 MiB) and the composed
// one (CID pass, launch_decrypt, DEK pass, k_open_compare) for everything
// else; set_open_route picks (0 auto, 1 composed, 2 fused wherever able;
// other values change nothing) and returns the previous value.
struct OpenJob {
  const uint8_t *ctext;
  uint8_t *ptext;               // nullable; may equal ctext
  uint64_t n, bs, last_len;
  const uint8_t *refs;          // dense, 64 B per block, 4-B aligned
  uint32_t *status;             // 4-B aligned
  uint32_t salt[8];
  uint32_t cid_key[8];          // the IV when unkeyed
  bool salted, cid_keyed;
};
hipError_t launch_open(const OpenJob &, hipStream_t);
int set_open_route(int route);

// The same checks over messages of unequal length in throughput form
// (ragged_open_kernels.h): message i is ctext[offs[i] .. offs[i]+lens[i]), its
// ref at refs + 64*i, its plaintext goes to ptext at the same offset and its
// status word (as OpenJob's) to status[i].  The ragged post's plan and
// structure: work follows the bytes, at most five launches whatever n and one
// host wait, for the plan's totals.  A message of more than max_len bytes
// (max_len <= kMaxRaggedLen) is neither read nor written and gets status 1.
// With ptext == ctext the messages must be disjoint.
struct OpenRaggedJob {
  const uint8_t *ctext;
  uint8_t *ptext;               // nullable; same offsets as ctext; may be ctext
  const uint64_t *offs, *lens;  // device arrays
  uint64_t n, max_len;
  const uint8_t *refs;          // 64 B per message, 4-B aligned
  uint32_t *status;             // 4-B aligned
  uint32_t salt[8];
  uint32_t cid_key[8];          // the IV when unkeyed
  bool salted, cid_keyed;
};
hipError_t launch_open_ragged(const OpenRaggedJob &, hipStream_t);

// Synthetic splitmix64 byte stream (see oracle_fill_splitmix); offset % 8 == 0.
hipError_t launch_fill(uint8_t *dst, uint64_t offset, uint64_t n, uint64_t seed,
                       hipStream_t s);

// Split mode (launch_plan.h pass_plan): a launch of fewer than `wgs`
// workgroups spreads each message over up to 64 workgroups.  0 disables it.
// Returns the previous value.
uint32_t set_split_target(uint32_t wgs);
// Latency-mode threshold in workgroups (launch_plan.h Knobs); returns the
// previous value.
uint32_t set_latency_wgs(uint32_t wgs);
// Drop all launch scratch kept for stream s on its device -- split mode,
// k_pass_dc, k_small_q, the ragged post, the verified read -- (call before
// destroying s, after it has drained).
void release_stream_scratch(hipStream_t s);

// Tree JSON lines on the device (tree_kernels.hip): see glfsx_tree_encode.
struct TreeJob {
  uint64_t n;
  const uint8_t *names;
  const uint64_t *name_offs;  // n + 1
  const uint32_t *modes;
  const uint8_t *types;
  const uint64_t *type_offs;  // n + 1
  const uint8_t *roots;       // 64 B per entry
  const uint64_t *sizes, *block_sizes;
  uint64_t *scratch;          // n + ceil(n / 256) words
  uint64_t *line_ends;        // nullable
  uint64_t *total;            // device word: total bytes
  uint8_t *out;               // nullable: lengths only
  uint64_t cap;               // bytes at out
  // hex_pos != nullptr: k_tree_write leaves the 64 hex digits of each cid
  // and dek unwritten and stores at hex_pos[i] the out offset of entry i's
  // first cid digit (its dek digits start kDekAfterCid bytes later); the
  // small-blob CID pass writes them (SmallJob::hex_out)
  uint64_t *hex_pos;
  // 1: the layout and static-line kernels run beside the small-blob DEK
  // pass (a 256-thread prefix, raised wave priority)
  uint32_t prio;
  // nullable, pinned host memory (device pointer) of ceil(n / 256) + 1
  // words: the layout's prefix kernel also stores the per-workgroup
  // exclusive prefix and then the total there (no copy kernel behind it)
  uint64_t *prefix_host;
};
// `<64 cid digits>","dek":"<64 dek digits>`: the dek's digits follow the
// cid's first digit by 64 + len("\",\"dek\":\"") bytes
constexpr uint32_t kDekAfterCid = 64 + 9;
hipError_t launch_tree_encode(const TreeJob &j, hipStream_t s);
// The same in two steps: the layout (line lengths, per-workgroup exclusive
// prefix at scratch + n, the total) -- it does not read the roots' values --
// and then the static lines (launch_tree_static).
hipError_t launch_tree_layout(const TreeJob &j, hipStream_t s);
// The lines without their hex digits (j.hex_pos set), in half workgroups
// small enough to run beside the small-blob DEK pass.
hipError_t launch_tree_static(const TreeJob &j, hipStream_t s);

// The inverse (tree_decode_kernels.h): see glfsx_tree_decode_device.  Seven
// launches whatever n or len.  len > 0, n_cap > 0.
constexpr uint32_t kTdSpan = 16 * 1024;  // bytes per workgroup of the count / index passes
struct TreeDecodeJob {
  const uint8_t *data;
  uint64_t len;
  uint64_t n_cap;     // lines the index and every per-line output hold
  // tree_decode_words(data, len, n_cap) words.  The first five are the
  // results once the launches have completed: n, bytes of names, bytes of
  // types, n_bad (a tail counted), tail
  uint64_t *scratch;
  uint8_t *names;     // every output nullable
  uint64_t names_cap;
  uint64_t *name_offs;
  uint32_t *modes;
  uint8_t *types;
  uint64_t types_cap;
  uint64_t *type_offs;
  uint8_t *roots;
  uint64_t *sizes, *block_sizes;
  uint32_t *status;
};
// spans are cut from the 16-byte boundary at or below data
inline uint64_t tree_decode_spans(const uint8_t *data, uint64_t len) {
  return ((reinterpret_cast<uintptr_t>(data) & 15) + len + kTdSpan - 1) / kTdSpan;
}
inline uint64_t tree_decode_wgs(uint64_t n_cap) { return (n_cap + kTreeWG - 1) / kTreeWG; }
inline uint64_t tree_decode_words(const uint8_t *data, uint64_t len, uint64_t n_cap) {
  return 8 + tree_decode_spans(data, len) + 2 * tree_decode_wgs(n_cap) + 3 * n_cap;
}
hipError_t launch_tree_decode(const TreeDecodeJob &j, hipStream_t s);

// Tree against tree (tree_join_kernels.h): see glfsx_tree_join_device and
// glfsx_tree_select_device.  One side's columns, device pointers (the layout
// of glfsx_tree_cols).
struct TreeCols {
  uint64_t n;
  const uint8_t *names;
  const uint64_t *name_offs;  // n + 1
  const uint32_t *modes;
  const uint8_t *types;
  const uint64_t *type_offs;  // n + 1
  const uint8_t *roots;       // 64 B per entry
  const uint64_t *sizes, *block_sizes;
  const uint32_t *status;     // nullable: zeros
};
// One launch: lane g < a.n looks a's entry g up in b, lane a.n + g b's entry
// g in a (tree_join.h).  Outputs nullable.
struct TreeJoinJob {
  TreeCols a, b;
  int64_t *a_match, *b_match;
  uint8_t *a_class;
};
hipError_t launch_tree_join(const TreeJoinJob &j, hipStream_t s);
// Four launches whatever k (k > 0): the selected strings' lengths scanned
// within each workgroup, k_tree_prefix over the workgroups' name and type
// totals, the write.  scratch: tree_select_words(k) words, the first three
// zero before the launches; after them they hold the bytes of the names, of
// the types, and 1 if a sel value named no entry.  The write kernel is
// launched only with write set, and writes nothing when that flag is set or
// a total exceeds its capacity.
struct TreeSelectJob {
  TreeCols a, b;
  const int64_t *sel;
  uint64_t k;
  uint64_t *scratch;
  bool write;
  uint8_t *names;             // every output nullable
  uint64_t names_cap;
  uint64_t *name_offs;        // k + 1
  uint32_t *modes;
  uint8_t *types;
  uint64_t types_cap;
  uint64_t *type_offs;        // k + 1
  uint8_t *roots;
  uint64_t *sizes, *block_sizes;
  uint32_t *status;
};
inline uint64_t tree_select_words(uint64_t k) {
  return 8 + 2 * ((k + kTreeWG - 1) / kTreeWG) + 2 * k;
}
hipError_t launch_tree_select(const TreeSelectJob &j, hipStream_t s);

// n blobs of len bytes (len % 8 == 0), blob b = the splitmix stream of seed
// seed0 + b (see oracle_fill_splitmix_blobs).
hipError_t launch_fill_blobs(uint8_t *dst, uint64_t n, uint64_t len, uint64_t seed0,
                             hipStream_t s);

#if GLFSX_WGTIME
hipError_t debug_wgtime(uint64_t *out);  // 8192 x 8 words (diagnostic builds)
#endif

// DeriveKey of any input length and output length (xof_kernels.hip): the
// hash state of one stream, carried across launches in device memory.
struct B3State {
  uint32_t key[8];
  uint32_t base;    // flags of every compression (kKeyed for DeriveKey)
  uint32_t depth;   // entries on the CV stack
  uint64_t chunks;  // chunks absorbed (a multiple of 256)
  uint32_t stack[64][8];
};
// `groups` whole 256-chunk groups at src, none of them holding the input's
// last byte.
hipError_t launch_b3_absorb(B3State *st, const uint8_t *src, uint64_t groups, hipStream_t s);
// The input's last n bytes (<= 256 KiB; 0 only for the empty input), then
// out_len bytes of XOF output.
hipError_t launch_b3_final(B3State *st, const uint8_t *src, uint64_t n, uint8_t *out,
                           uint64_t out_len, hipStream_t s);

void words_from_key(uint32_t w[8], const uint8_t key[32]);
void blake3_iv_words(uint32_t w[8]);

}  // namespace glfsx
