// tree_line.h -- the grammar of one canonical tree line, defined once.
//
// A tree blob is JSON lines (tree.go:300-316).  A line is canonical when it
// is byte for byte a line glfsx_tree_encode can write:
//   {"name":S,"mode":D,"ref":{"type":S,"cid":"H","dek":"H","size":D,"blockSize":D}}
// followed by one '\n'; H exactly 64 lower-case hex digits, D decimal with no
// sign and no leading zero (mode fits uint32, size and blockSize uint64), S a
// quoted string over the encoder's output alphabet (encoding/json's
// appendString with escapeHTML, tree.cpp json_string):
//   - an ASCII byte 0x20..0x7F other than " \ < > &
//   - a UTF-8 sequence utf8.DecodeRune accepts, other than U+2028 / U+2029
//   - \" \\ \b \f \n \r \t
//   - \u00XX (lower case) for the other bytes below 0x20
//   - \u003c \u003e \u0026 \u2028 \u2029 and \ufffd (written for each byte of
//     invalid UTF-8), lower case
// Nothing else: the decoders vouch only for what the encoder writes and
// report the rest (GLFSX_TREE_NONCANON) for a general JSON decoder.
//
// Pure functions, no HIP includes: the host decoder (tree.cpp) and the
// kernels (tree_decode_kernels.h) both parse through tl_parse, so they
// cannot disagree.  P is any byte pointer (`const uint8_t *` in any address
// space).  Every read is at an index below `end`, the index of the line's
// '\n': the input is untrusted.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TL_HD inline
#endif

namespace glfsx {

// What tl_parse learns about a canonical line (indexes are into p).
struct TlLine {
  uint64_t name_at;   // first byte after the name's opening quote
  uint64_t type_at;   // the same of the type
  uint64_t cid_at;    // the cid's first hex digit; the dek's follow 73 bytes later
  uint64_t name_len;  // decoded lengths
  uint64_t type_len;
  uint64_t size, block_size;
  uint32_t mode;
};
constexpr uint32_t kTlDekAfterCid = 64 + 9;  // `<64 digits>","dek":"`

TL_HD bool tl_lower_hex(uint32_t c) { return (c - '0') < 10u || (c - 'a') < 6u; }
TL_HD uint32_t tl_nibble(uint32_t c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// p[at..] == s (N - 1 bytes), all below end
template <class P, int N>
TL_HD bool tl_lit(P p, uint64_t *at, uint64_t end, const char (&s)[N]) {
  if (end - *at < uint64_t(N - 1)) return false;
  bool ok = true;
  for (int i = 0; i + 1 < N; ++i) ok &= p[*at + i] == uint8_t(s[i]);
  *at += N - 1;
  return ok;
}

// One escape at p[at] == '\\': its encoded length (2 or 6) and the code point
// it stands for; 0 length when it is not one the encoder writes.
template <class P>
TL_HD uint32_t tl_escape(P p, uint64_t at, uint64_t end, uint32_t *cp) {
  if (end - at < 2) return 0;
  switch (p[at + 1]) {
    case '"': *cp = '"'; return 2;
    case '\\': *cp = '\\'; return 2;
    case 'b': *cp = '\b'; return 2;
    case 'f': *cp = '\f'; return 2;
    case 'n': *cp = '\n'; return 2;
    case 'r': *cp = '\r'; return 2;
    case 't': *cp = '\t'; return 2;
    case 'u': break;
    default: return 0;
  }
  if (end - at < 6) return 0;
  uint32_t v = 0;
  for (int i = 2; i < 6; ++i) {
    const uint32_t c = p[at + i];
    if (!tl_lower_hex(c)) return 0;
    v = (v << 4) | tl_nibble(c);
  }
  *cp = v;
  if (v < 0x20)  // the control bytes without a short form
    return (v == '\b' || v == '\f' || v == '\n' || v == '\r' || v == '\t') ? 0 : 6;
  return (v == '<' || v == '>' || v == '&' || v == 0x2028 || v == 0x2029 || v == 0xFFFD) ? 6 : 0;
}

// Length of the valid UTF-8 sequence at p[at] (lead byte >= 0x80) as Go's
// utf8.DecodeRune accepts it, 0 if invalid; U+2028 / U+2029 count as invalid
// here (the encoder escapes them).
template <class P>
TL_HD uint32_t tl_rune(P p, uint64_t at, uint64_t end) {
  const uint32_t b0 = p[at];
  const uint64_t n = end - at;
  auto cont = [&](uint64_t i) { return i < n && (p[at + i] & 0xC0) == 0x80; };
  if (b0 >= 0xC2 && b0 <= 0xDF) return cont(1) ? 2 : 0;
  if (b0 >= 0xE0 && b0 <= 0xEF) {
    if (!cont(1) || !cont(2)) return 0;
    const uint32_t b1 = p[at + 1];
    if ((b0 == 0xE0 && b1 < 0xA0) || (b0 == 0xED && b1 > 0x9F)) return 0;
    if (b0 == 0xE2 && b1 == 0x80 && (p[at + 2] & 0xFE) == 0xA8) return 0;  // U+2028/9
    return 3;
  }
  if (b0 >= 0xF0 && b0 <= 0xF4) {
    if (!cont(1) || !cont(2) || !cont(3)) return 0;
    const uint32_t b1 = p[at + 1];
    if ((b0 == 0xF0 && b1 < 0x90) || (b0 == 0xF4 && b1 > 0x8F)) return 0;
    return 4;
  }
  return 0;
}

// A quoted string at p[*at]: on success *at is past the closing quote,
// *body the first byte after the opening one and *dec_len the decoded length.
template <class P>
TL_HD bool tl_string(P p, uint64_t *at, uint64_t end, uint64_t *body, uint64_t *dec_len) {
  uint64_t i = *at, n = 0;
  if (i >= end || p[i] != '"') return false;
  *body = ++i;
  while (i < end) {
    const uint32_t b = p[i];
    if (b == '"') {
      *at = i + 1;
      *dec_len = n;
      return true;
    }
    if (b == '\\') {
      uint32_t cp;
      const uint32_t k = tl_escape(p, i, end, &cp);
      if (!k) return false;
      i += k;
      n += cp < 0x80 ? 1 : 3;
    } else if (b < 0x80) {
      if (b < 0x20 || b == '<' || b == '>' || b == '&') return false;
      ++i;
      ++n;
    } else {
      const uint32_t k = tl_rune(p, i, end);
      if (!k) return false;
      i += k;
      n += k;
    }
  }
  return false;  // no closing quote before the line's end
}

// The decoded bytes of a string tl_string accepted, one at a time: next()
// returns the byte, or -1 at the closing quote.
template <class P>
struct TlUnescape {
  P p;
  uint64_t at;
  uint32_t pend = 0, npend = 0;
  TL_HD TlUnescape(P p_, uint64_t body) : p(p_), at(body) {}
  TL_HD int next() {
    if (npend) {
      const int b = int(pend & 0xFF);
      pend >>= 8;
      --npend;
      return b;
    }
    const uint32_t b = p[at];
    if (b == '"') return -1;
    if (b != '\\') {
      ++at;
      return int(b);
    }
    uint32_t cp = 0;
    // validated before: the escape is whole, so no read passes the quote
    at += tl_escape(p, at, ~0ull, &cp);
    if (cp < 0x80) return int(cp);
    pend = (0x80 | ((cp >> 6) & 0x3F)) | ((0x80 | (cp & 0x3F)) << 8);
    npend = 2;
    return int(0xE0 | (cp >> 12));
  }
};

// A decimal at p[*at] with no sign and no leading zero, at most `max`.
template <class P>
TL_HD bool tl_dec(P p, uint64_t *at, uint64_t end, uint64_t max, uint64_t *out) {
  uint64_t i = *at, v = 0;
  if (i >= end) return false;
  uint32_t d = uint32_t(p[i]) - '0';
  if (d > 9) return false;
  v = d;
  ++i;
  if (d != 0) {
    while (i < end && (d = uint32_t(p[i]) - '0') <= 9) {
      if (v > (max - d) / 10) return false;
      v = v * 10 + d;
      ++i;
    }
  } else if (i < end && uint32_t(p[i]) - '0' <= 9) {
    return false;  // a leading zero
  }
  if (v > max) return false;
  *at = i;
  *out = v;
  return true;
}

// Four lower-case hex digits (the bytes of w in memory order) to two bytes,
// the mirror of the encoder's hex4: *bad collects a non-zero word if any
// digit is not [0-9a-f].
TL_HD uint32_t tl_unhex4(uint32_t w, uint32_t *bad) {
  const uint32_t a = (w >> 6) & 0x01010101u;            // 1: a letter's column
  const uint32_t hi = w & 0xF0F0F0F0u;
  const uint32_t v = (w & 0x0F0F0F0Fu) + 9 * a;          // the value, if valid
  *bad |= hi ^ (0x30303030u + 0x30 * a);                 // 0x3_ digits, 0x6_ letters
  *bad |= v & 0x10101010u;                               // letters past f
  *bad |= (((v + 0x06060606u) >> 4) & 0x01010101u) ^ a;  // ':'..'?' and '`', 'p'..
  const uint32_t t = (v << 4) | (v >> 8);
  return (t & 0xFF) | ((t >> 8) & 0xFF00);
}

// 64 digits as 16 words -> 32 bytes as 8 words; false if any is not a digit
TL_HD bool tl_unhex64(const uint32_t w[16], uint32_t out[8]) {
  uint32_t bad = 0;
  for (int i = 0; i < 8; ++i)
    out[i] = tl_unhex4(w[2 * i], &bad) | (tl_unhex4(w[2 * i + 1], &bad) << 16);
  return bad == 0;
}

// 4 * nw bytes at p[at..] as little-endian words, byte by byte
template <class P>
TL_HD void tl_load_words(P p, uint64_t at, uint32_t *w, int nw) {
  for (int i = 0; i < nw; ++i)
    w[i] = uint32_t(p[at + 4 * i]) | (uint32_t(p[at + 4 * i + 1]) << 8) |
           (uint32_t(p[at + 4 * i + 2]) << 16) | (uint32_t(p[at + 4 * i + 3]) << 24);
}

// `"<64 hex digits>"` at p[*at]: only the digits' validity (the conversion
// is tl_unhex64 over the same bytes, by whoever writes the root)
template <class P>
TL_HD bool tl_hex_field(P p, uint64_t *at, uint64_t end) {
  if (end - *at < 66) return false;
  bool ok = p[*at] == '"' && p[*at + 65] == '"';
  uint32_t w[16], o[8];
  tl_load_words(p, *at + 1, w, 16);
  ok &= tl_unhex64(w, o);
  *at += 66;
  return ok;
}

// The line p[start, end) (p[end] is its '\n'): true and *L when canonical.
// hex: check the digits here (false: the caller checks them with tl_unhex64
// while converting; the quotes are checked either way).
template <class P>
TL_HD bool tl_parse(P p, uint64_t start, uint64_t end, TlLine *L, bool hex = true) {
  uint64_t at = start, v;
  if (!tl_lit(p, &at, end, "{\"name\":")) return false;
  if (!tl_string(p, &at, end, &L->name_at, &L->name_len)) return false;
  if (!tl_lit(p, &at, end, ",\"mode\":")) return false;
  if (!tl_dec(p, &at, end, 0xFFFFFFFFull, &v)) return false;
  L->mode = uint32_t(v);
  if (!tl_lit(p, &at, end, ",\"ref\":{\"type\":")) return false;
  if (!tl_string(p, &at, end, &L->type_at, &L->type_len)) return false;
  if (!tl_lit(p, &at, end, ",\"cid\":")) return false;
  L->cid_at = at + 1;
  if (hex) {
    if (!tl_hex_field(p, &at, end)) return false;
    if (!tl_lit(p, &at, end, ",\"dek\":")) return false;
    if (!tl_hex_field(p, &at, end)) return false;
  } else {
    if (end - at < 66 + 7 + 66) return false;
    if (p[at] != '"' || p[at + 65] != '"') return false;
    at += 66;
    if (!tl_lit(p, &at, end, ",\"dek\":")) return false;
    if (p[at] != '"' || p[at + 65] != '"') return false;
    at += 66;
  }
  if (!tl_lit(p, &at, end, ",\"size\":")) return false;
  if (!tl_dec(p, &at, end, ~0ull, &L->size)) return false;
  if (!tl_lit(p, &at, end, ",\"blockSize\":")) return false;
  if (!tl_dec(p, &at, end, ~0ull, &L->block_size)) return false;
  if (!tl_lit(p, &at, end, "}}")) return false;
  return at == end;
}

// TreeEntry.Validate (tree.go:80-89) without building CleanPath(name): the
// name is non-empty, has no leading or trailing '/', and its components are
// zero or more ".." followed by components none of which is "", "." or "..".
// Fed the decoded bytes one at a time.
struct TlNameCheck {
  uint32_t clen = 0, dots = 0;  // the current component: bytes, and how many are '.'
  bool any = false, bad = false, past_up = false;
  TL_HD void close() {  // a component ends
    const bool dot = clen == 1 && dots == 1, up = clen == 2 && dots == 2;
    if (clen == 0 || dot || (up && past_up)) bad = true;
    if (!up) past_up = true;
    clen = dots = 0;
  }
  TL_HD void feed(uint32_t b) {
    any = true;
    if (b == '/') {
      close();
    } else {
      ++clen;
      dots += b == '.';
    }
  }
  TL_HD bool ok() {  // once, after the last byte
    if (!any) return false;
    close();
    return !bad;
  }
};

// Name rule and order of a canonical line against the canonical line before
// it (have_prev): the GLFSX_TREE_NAME (4) and GLFSX_TREE_ORDER (2) bits.
// out != nullptr: also writes the decoded name there (name_len bytes).
template <class P, class Q>
TL_HD uint32_t tl_name_bits(P p, uint64_t name_at, Q q, uint64_t prev_name_at, bool have_prev,
                            uint8_t *out) {
  TlUnescape<P> u(p, name_at);
  TlUnescape<Q> w(q, prev_name_at);
  TlNameCheck chk;
  int cmp = 0;  // sign of name - prev over the bytes so far
  bool prev_open = have_prev;
  uint64_t o = 0;
  for (int b; (b = u.next()) >= 0;) {
    chk.feed(uint32_t(b));
    if (out) out[o++] = uint8_t(b);
    if (prev_open && cmp == 0) {
      const int c = w.next();
      if (c < 0) {
        cmp = 1;  // prev is a proper prefix: name > prev
      } else if (b != c) {
        cmp = b < c ? -1 : 1;
      }
    }
  }
  // all of name matched a prefix of prev (or all of it): name <= prev
  const bool le = have_prev && cmp <= 0;
  return (chk.ok() ? 0u : 4u) | (le ? 2u : 0u);
}

}  // namespace glfsx
