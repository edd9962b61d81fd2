// dfx_utf8_match.hpp -- the matcher of Utf8 string terms (deviation D9: `Utf8 column <op> Utf8 literal`, LIKE / NOT LIKE),
// usable on the device (hipcc: dfx_k_utf8pred.hip evaluates a term per row with it) and on the host (dfx_debug_utf8_term, so
// that a CPU test runs the code the kernel runs).  dfx_numparse.hpp works the same way.
//
// Ordering is Rust `str` ordering: unsigned byte-wise lexicographic, a proper prefix sorts first.  Equality is byte equality.
// LIKE: `%` any run of bytes (also none), `_` exactly one UTF-8 encoded character (a lead byte and its continuation bytes),
// no escape character, anchored at both ends.  A pattern is compiled ONCE (utf8_compile_term in dfx_expr_utf8.cpp, host) into a class and a table
// of `%`-separated segments; the first segment is anchored at the start, the last at the end, the middle ones are matched
// leftmost-first -- exact for this pattern language (a segment has a fixed number of characters), so nothing backtracks.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFX_U8 __host__ __device__ inline
#else
#define DFX_U8 inline
#endif

namespace dfx {

constexpr uint32_t kUtf8MaxLiteral = 4096;  // bytes of a literal / pattern (longer: DFX_NOT_IMPLEMENTED at compile time)

enum Utf8Class : uint32_t {
  U8_CMP = 0,       // three-way comparison with the literal (Eq NotEq Lt LtEq Gt GtEq, and LIKE without wildcards)
  U8_PREFIX = 1,    // abc%
  U8_SUFFIX = 2,    // %abc
  U8_CONTAINS = 3,  // %abc%
  U8_GENERAL = 4    // segments that may hold `_`
};
enum : uint32_t { U8F_LEAD = 1, U8F_TRAIL = 2, U8F_PCT = 4 };  // the pattern starts with %, ends with %, has a % at all

struct Utf8Seg {  // one segment of a general pattern: bytes [off, off + len) of the term's literal bytes
  uint16_t off, len;
};

// One compiled term.  `lit`: the literal (U8_CMP), the one segment (PREFIX / SUFFIX / CONTAINS) or the segments' bytes back
// to back (GENERAL, `segs` says where each lies).
struct Utf8Term {
  uint32_t cls;      // Utf8Class
  uint32_t m;        // U8_CMP: three-way mask of the outcomes that pass (1 value < literal, 2 equal, 4 greater)
  uint32_t inv;      // NOT LIKE: the complement on non-null rows
  uint32_t if_null;  // what a null slot gives (arrow 0.12 bool_op over Option<T>: None sorts below every value)
  uint32_t lit_len;
  uint32_t n_segs;
  uint32_t min_len;  // LIKE: a value with fewer bytes cannot match
  uint32_t flags;    // U8F_*
};

// The image of a term's bytes, as the host builds it, the device buffer holds it and the kernel stages it to LDS: the literal
// bytes, zero-padded to a 4-byte boundary, then the segment table.  These two functions are the only statement of that layout.
DFX_U8 uint32_t utf8_term_segs_at(const Utf8Term& t) { return (t.lit_len + 3u) & ~3u; }
DFX_U8 uint32_t utf8_term_image_bytes(const Utf8Term& t) { return utf8_term_segs_at(t) + t.n_segs * (uint32_t)sizeof(Utf8Seg); }  // whole 4-byte words

// the operator of a comparison term (dfx_operator Eq .. GtEq, already mirrored for a literal on the left) as a three-way mask
DFX_U8 uint32_t utf8_cmp_mask(int op) { return op == 0 ? 2u : op == 1 ? 5u : op == 2 ? 1u : op == 3 ? 3u : op == 4 ? 4u : 6u; }
DFX_U8 uint32_t utf8_cmp_if_null(uint32_t m) { return m & 1u; }  // None < Some(literal): the terms that pass "less" pass

// 1: a < b, 2: equal, 4: a > b
DFX_U8 uint32_t utf8_three_way(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
  const uint32_t n = la < lb ? la : lb;
  for (uint32_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return a[i] < b[i] ? 1u : 4u;
  return la < lb ? 1u : la == lb ? 2u : 4u;
}

DFX_U8 bool utf8_bytes_equal(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

DFX_U8 bool utf8_is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// segment `seg` against v at byte `pos`, not beyond `limit`; *end: where the match stops.  `_` takes one byte and the
// continuation bytes that follow it.
DFX_U8 bool utf8_seg_forward(const uint8_t* v, uint32_t pos, uint32_t limit, const uint8_t* seg, uint32_t slen, uint32_t* end) {
  for (uint32_t i = 0; i < slen; ++i) {
    if (pos >= limit) return false;
    if (seg[i] == (uint8_t)'_') {
      ++pos;
      while (pos < limit && utf8_is_cont(v[pos])) ++pos;
    } else {
      if (v[pos] != seg[i]) return false;
      ++pos;
    }
  }
  *end = pos;
  return true;
}

// the same from the right: the segment must end at `end` and start at or after `lo`; *start: where it begins.  `_` takes the
// continuation bytes before `end` and the lead byte before them.
DFX_U8 bool utf8_seg_backward(const uint8_t* v, uint32_t lo, uint32_t end, const uint8_t* seg, uint32_t slen, uint32_t* start) {
  for (uint32_t i = slen; i > 0; --i) {
    if (end <= lo) return false;
    if (seg[i - 1] == (uint8_t)'_') {
      --end;
      while (end > lo && utf8_is_cont(v[end])) --end;
      if (utf8_is_cont(v[end])) return false;  // ran into `lo` inside a character
    } else {
      if (v[end - 1] != seg[i - 1]) return false;
      --end;
    }
  }
  *start = end;
  return true;
}

DFX_U8 bool utf8_like_general(const Utf8Term& t, const uint8_t* lit, const Utf8Seg* segs, const uint8_t* v, uint32_t vlen) {
  uint32_t pos = 0, end = vlen, i0 = 0, i1 = t.n_segs;
  if (!(t.flags & U8F_PCT)) {  // `_` and literal bytes only: the one segment is the whole value
    if (t.n_segs == 0) return vlen == 0;
    return utf8_seg_forward(v, 0, vlen, lit + segs[0].off, segs[0].len, &pos) && pos == vlen;
  }
  if (!(t.flags & U8F_LEAD) && i0 < i1) {
    if (!utf8_seg_forward(v, 0, vlen, lit + segs[0].off, segs[0].len, &pos)) return false;
    ++i0;
  }
  if (!(t.flags & U8F_TRAIL) && i0 < i1) {
    if (!utf8_seg_backward(v, pos, vlen, lit + segs[i1 - 1].off, segs[i1 - 1].len, &end)) return false;
    --i1;
  }
  for (uint32_t i = i0; i < i1; ++i) {  // leftmost-first between the anchors
    const uint8_t* seg = lit + segs[i].off;
    const uint32_t slen = segs[i].len;
    bool found = false;
    for (uint32_t p = pos; p < end; ++p) {
      if (utf8_is_cont(v[p])) continue;  // a segment starts on a character boundary
      uint32_t e;
      if (utf8_seg_forward(v, p, end, seg, slen, &e)) {
        pos = e;
        found = true;
        break;
      }
    }
    if (!found) return false;
  }
  return true;
}

// a term over one NON-NULL value (a null slot gives t.if_null)
DFX_U8 bool utf8_term_eval(const Utf8Term& t, const uint8_t* lit, const Utf8Seg* segs, const uint8_t* v, uint32_t vlen) {
  bool r;
  switch (t.cls) {
    case U8_CMP:
      if ((t.m == 2u || t.m == 5u) && vlen != t.lit_len) return t.m == 5u;  // equality: the length decides first
      return (utf8_three_way(v, vlen, lit, t.lit_len) & t.m) != 0u;
    case U8_PREFIX: r = vlen >= t.lit_len && utf8_bytes_equal(v, lit, t.lit_len); break;
    case U8_SUFFIX: r = vlen >= t.lit_len && utf8_bytes_equal(v + (vlen - t.lit_len), lit, t.lit_len); break;
    case U8_CONTAINS: {
      r = false;
      if (vlen >= t.lit_len)
        for (uint32_t p = 0; p + t.lit_len <= vlen && !r; ++p) r = utf8_bytes_equal(v + p, lit, t.lit_len);
      break;
    }
    default: r = vlen >= t.min_len && utf8_like_general(t, lit, segs, v, vlen); break;
  }
  return r != (t.inv != 0u);
}

}  // namespace dfx
