// dfx_numfmt.hpp -- number -> CSV cell text (deviation D11: the CSV writer), usable on the device (hipcc: dfx_k_csvwrite.hip
// formats every cell with it) and on the host (dfx_debug_format_value, tests/native/numfmt_fuzz.cpp: a CPU test runs the code
// the kernel runs).  dfx_numparse.hpp, its inverse, and dfx_utf8_match.hpp work the same way.  Integer arithmetic only.
//
// Float64 / Float32: the SHORTEST decimal digit string that parses back to the same bits in that width, the closest to the
// exact value among the shortest (Schubfach: R. Giulietti, "The Schubfach way to render doubles", 2020 -- one 128-bit
// product with a rounded-up power of ten per interval bound, tools/gen_pow10_table.py), laid out as Rust's `{:?}`:
//   1e-4 <= |x| < 1e16 and zero: positional with at least one digit after the point  (1.0  0.1  123456.789  -0.0)
//   otherwise                  : d[.ddd]e[-]x, no '+', no leading zeros in the exponent (1e16  1.5e-5  5e-324)
//   NaN (every payload), inf, -inf.
// Bounds: a Float64 cell is at most 24 bytes (-1.2345678901234567e-308: sign, 17 digits, point, e-308), a Float32 cell at
// most 19 (-1234567800000000.0: sign, 16 integer digits, ".0"), an integer cell at most 20.
// Utf8: a cell is quoted iff it holds ',', '"', CR or LF (or the caller forces it: the empty cell of a one-column file);
// inside quotes every '"' is doubled.
#pragma once
#include <stdint.h>

#include "dfx_pow10_table.hpp"

#if defined(__HIPCC__)
#define DFX_NF __host__ __device__ inline
#else
#define DFX_NF inline
#endif

namespace dfx {

constexpr int kNfMaxF64 = 24;
constexpr int kNfMaxF32 = 19;
constexpr int kNfMaxInt = 20;
constexpr int kNfMaxCell = 24;  // of any fixed-width type

struct NfDecimal {  // digits * 10^exp10, digits without trailing zeros
  uint64_t digits;
  int32_t exp10;
};

DFX_NF void nf_mul64(uint64_t a, uint64_t b, uint64_t* lo, uint64_t* hi) {
  const unsigned __int128 p = (unsigned __int128)a * b;  // (the device compiler expands it into 32-bit multiplies)
  *lo = (uint64_t)p;
  *hi = (uint64_t)(p >> 64);
}

// floor(log2(10^e)), |e| <= 1233;  floor(log10(2^e)) and floor(log10(3/4 * 2^e)), |e| <= 1500  (arithmetic shifts)
DFX_NF int32_t nf_floor_log2_pow10(int32_t e) { return (e * 1741647) >> 19; }
DFX_NF int32_t nf_floor_log10_pow2(int32_t e, bool three_quarters) { return (e * 1262611 - (three_quarters ? 524031 : 0)) >> 22; }

// floor(g * cp / 2^128) with the dropped bits ORed into bit 0 ("round to odd"): g = {ghi, glo}
DFX_NF uint64_t nf_round_to_odd64(uint64_t ghi, uint64_t glo, uint64_t cp) {
  uint64_t xlo, xhi, ylo, yhi;
  nf_mul64(glo, cp, &xlo, &xhi);
  nf_mul64(ghi, cp, &ylo, &yhi);
  const uint64_t mid = ylo + xhi;
  const uint64_t top = yhi + (uint64_t)(mid < xhi);
  return top | (uint64_t)(mid > 1);
}
// the binary32 flavour: floor(g * cp / 2^64), 64-bit g
DFX_NF uint32_t nf_round_to_odd32(uint64_t g, uint32_t cp) {
  uint64_t lo, hi;
  nf_mul64(g, (uint64_t)cp, &lo, &hi);
  return (uint32_t)hi | (uint32_t)((uint32_t)(lo >> 32) > 1u);
}

DFX_NF NfDecimal nf_strip_zeros(uint64_t d, int32_t e) {
  while (d != 0 && d % 10u == 0) {
    d /= 10u;
    ++e;
  }
  NfDecimal r = {d, e};
  return r;
}

// the choice among the candidates (figures 4 and 6 of the paper): vbl / vb / vbr are 4 * {lower bound, value, upper bound}
// scaled by 10^-k, rounded to odd
DFX_NF NfDecimal nf_pick(uint64_t vbl, uint64_t vb, uint64_t vbr, bool even, int32_t k) {
  const uint64_t lower = vbl + (even ? 0u : 1u);
  const uint64_t upper = vbr - (even ? 0u : 1u);
  const uint64_t s = vb / 4;
  if (s >= 10) {  // one digit fewer?
    const uint64_t sp = s / 10;
    const bool up_inside = lower <= 40 * sp;
    const bool wp_inside = 40 * sp + 40 <= upper;
    if (up_inside != wp_inside) return nf_strip_zeros(sp + (wp_inside ? 1u : 0u), k + 1);
  }
  const bool u_inside = lower <= 4 * s;
  const bool w_inside = 4 * s + 4 <= upper;
  if (u_inside != w_inside) return nf_strip_zeros(s + (w_inside ? 1u : 0u), k);
  const uint64_t mid = 4 * s + 2;  // both or neither: the closer one, ties to even
  const bool round_up = vb > mid || (vb == mid && (s & 1) != 0);
  return nf_strip_zeros(s + (round_up ? 1u : 0u), k);
}

// finite, non-zero: fraction bits and biased exponent of a binary64
DFX_NF NfDecimal nf_shortest_f64(uint64_t frac, uint32_t bexp) {
  uint64_t c;
  int32_t q;
  if (bexp != 0) {
    c = (1ull << 52) | frac;
    q = (int32_t)bexp - 1075;
    if (0 <= -q && -q < 53 && (c & ((1ull << -q) - 1)) == 0) return nf_strip_zeros(c >> -q, 0);  // an integer below 2^53
  } else {
    c = frac;
    q = 1 - 1075;
  }
  const bool even = (c & 1) == 0;
  const bool lower_closer = frac == 0 && bexp > 1;
  const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1u : 0u);
  const uint64_t cb = 4 * c;
  const uint64_t cbr = 4 * c + 2;
  const int32_t k = nf_floor_log10_pow2(q, lower_closer);
  const int32_t h = q + nf_floor_log2_pow10(-k) + 1;  // 1 .. 4
  const uint64_t ghi = kPow10Table[2 * (-k - kPow10Smallest)], glo = kPow10Table[2 * (-k - kPow10Smallest) + 1];
  const uint64_t vbl = nf_round_to_odd64(ghi, glo, cbl << h);
  const uint64_t vb = nf_round_to_odd64(ghi, glo, cb << h);
  const uint64_t vbr = nf_round_to_odd64(ghi, glo, cbr << h);
  return nf_pick(vbl, vb, vbr, even, k);
}

DFX_NF NfDecimal nf_shortest_f32(uint32_t frac, uint32_t bexp) {
  uint32_t c;
  int32_t q;
  if (bexp != 0) {
    c = (1u << 23) | frac;
    q = (int32_t)bexp - 150;
    if (0 <= -q && -q < 24 && (c & ((1u << -q) - 1)) == 0) return nf_strip_zeros(c >> -q, 0);
  } else {
    c = frac;
    q = 1 - 150;
  }
  const bool even = (c & 1) == 0;
  const bool lower_closer = frac == 0 && bexp > 1;
  const uint32_t cbl = 4 * c - 2 + (lower_closer ? 1u : 0u);
  const uint32_t cb = 4 * c;
  const uint32_t cbr = 4 * c + 2;
  const int32_t k = nf_floor_log10_pow2(q, lower_closer);
  const int32_t h = q + nf_floor_log2_pow10(-k) + 1;
  // ceil(g128 / 2^64): the 64-bit rounded-up power of ten
  const uint64_t g = kPow10Table[2 * (-k - kPow10Smallest)] + (kPow10Table[2 * (-k - kPow10Smallest) + 1] != 0 ? 1u : 0u);
  const uint32_t vbl = nf_round_to_odd32(g, cbl << h);
  const uint32_t vb = nf_round_to_odd32(g, cb << h);
  const uint32_t vbr = nf_round_to_odd32(g, cbr << h);
  return nf_pick(vbl, vb, vbr, even, k);
}

DFX_NF int nf_count_digits(uint64_t v) {
  int n = 1;
  while (v >= 10000) {
    v /= 10000u;
    n += 4;
  }
  uint32_t w = (uint32_t)v;
  while (w >= 10) {
    w /= 10u;
    ++n;
  }
  return n;
}

// decimal digits of v into out[0, nd), nd = nf_count_digits(v)
DFX_NF void nf_put_digits(uint64_t v, int nd, uint8_t* out) {
  for (int i = nd - 1; i >= 0; --i) {
    out[i] = (uint8_t)('0' + (uint32_t)(v % 10u));
    v /= 10u;
  }
}

DFX_NF int nf_format_u64(uint64_t v, uint8_t* out) {
  const int nd = nf_count_digits(v);
  nf_put_digits(v, nd, out);
  return nd;
}
DFX_NF int nf_format_i64(int64_t v, uint8_t* out) {
  if (v >= 0) return nf_format_u64((uint64_t)v, out);
  out[0] = '-';
  return 1 + nf_format_u64(0ull - (uint64_t)v, out + 1);
}

// Rust `{:?}` of neg, digits * 10^exp10 (digits != 0, no trailing zeros).  Returns the length (<= 24 for <= 17 digits).
DFX_NF int nf_layout(bool neg, uint64_t digits, int32_t exp10, uint8_t* out) {
  int n = 0;
  if (neg) out[n++] = '-';
  const int nd = nf_count_digits(digits);
  const int32_t E = nd - 1 + exp10;  // scientific exponent
  if (E >= -4 && E < 16) {
    if (E < 0) {  // 0.000ddd
      out[n++] = '0';
      out[n++] = '.';
      for (int i = 0; i < -E - 1; ++i) out[n++] = '0';
      nf_put_digits(digits, nd, out + n);
      return n + nd;
    }
    if (exp10 >= 0) {  // ddd000.0
      nf_put_digits(digits, nd, out + n);
      n += nd;
      for (int i = 0; i < exp10; ++i) out[n++] = '0';
      out[n++] = '.';
      out[n++] = '0';
      return n;
    }
    const int il = E + 1;  // dd.ddd: il integer digits
    uint64_t v = digits;
    for (int i = nd - 1; i >= 0; --i) {
      out[n + i + (i >= il ? 1 : 0)] = (uint8_t)('0' + (uint32_t)(v % 10u));
      v /= 10u;
    }
    out[n + il] = '.';
    return n + nd + 1;
  }
  if (nd == 1) {
    out[n++] = (uint8_t)('0' + (uint32_t)digits);
  } else {  // d.ddd
    uint64_t v = digits;
    for (int i = nd - 1; i >= 1; --i) {
      out[n + i + 1] = (uint8_t)('0' + (uint32_t)(v % 10u));
      v /= 10u;
    }
    out[n] = (uint8_t)('0' + (uint32_t)v);
    out[n + 1] = '.';
    n += nd + 1;
  }
  out[n++] = 'e';
  uint32_t ae = (uint32_t)E;
  if (E < 0) {
    out[n++] = '-';
    ae = (uint32_t)-E;
  }
  return n + nf_format_u64(ae, out + n);
}

DFX_NF int nf_put3(uint8_t* out, char a, char b, char c) {
  out[0] = (uint8_t)a;
  out[1] = (uint8_t)b;
  out[2] = (uint8_t)c;
  return 3;
}

DFX_NF int nf_format_f64(uint64_t bits, uint8_t* out) {
  const bool neg = (bits >> 63) != 0;
  const uint32_t bexp = (uint32_t)(bits >> 52) & 0x7FFu;
  const uint64_t frac = bits & ((1ull << 52) - 1);
  if (bexp == 0x7FFu) {
    if (frac != 0) return nf_put3(out, 'N', 'a', 'N');
    if (neg) *out++ = '-';
    return nf_put3(out, 'i', 'n', 'f') + (neg ? 1 : 0);
  }
  if (bexp == 0 && frac == 0) {
    if (neg) *out++ = '-';
    return nf_put3(out, '0', '.', '0') + (neg ? 1 : 0);
  }
  const NfDecimal d = nf_shortest_f64(frac, bexp);
  return nf_layout(neg, d.digits, d.exp10, out);
}

DFX_NF int nf_format_f32(uint32_t bits, uint8_t* out) {
  const bool neg = (bits >> 31) != 0;
  const uint32_t bexp = (bits >> 23) & 0xFFu;
  const uint32_t frac = bits & ((1u << 23) - 1);
  if (bexp == 0xFFu) {
    if (frac != 0) return nf_put3(out, 'N', 'a', 'N');
    if (neg) *out++ = '-';
    return nf_put3(out, 'i', 'n', 'f') + (neg ? 1 : 0);
  }
  if (bexp == 0 && frac == 0) {
    if (neg) *out++ = '-';
    return nf_put3(out, '0', '.', '0') + (neg ? 1 : 0);
  }
  const NfDecimal d = nf_shortest_f32(frac, bexp);
  return nf_layout(neg, d.digits, d.exp10, out);
}

// One value of a fixed-width type (dtype: dfx_dtype / DevType 1 Boolean .. 11 Float64; bits: the value in the low bits, wider
// bits ignored).  out: room for kNfMaxCell bytes.  Returns the length, 0 for another dtype.
DFX_NF int nf_format_value(int dtype, uint64_t bits, uint8_t* out) {
  switch (dtype) {
    case 1:
      if (bits & 1) {
        out[0] = 't', out[1] = 'r', out[2] = 'u', out[3] = 'e';
        return 4;
      }
      out[0] = 'f', out[1] = 'a', out[2] = 'l', out[3] = 's', out[4] = 'e';
      return 5;
    case 2: return nf_format_i64((int64_t)(int8_t)(uint8_t)bits, out);
    case 3: return nf_format_i64((int64_t)(int16_t)(uint16_t)bits, out);
    case 4: return nf_format_i64((int64_t)(int32_t)(uint32_t)bits, out);
    case 5: return nf_format_i64((int64_t)bits, out);
    case 6: return nf_format_u64(bits & 0xFFull, out);
    case 7: return nf_format_u64(bits & 0xFFFFull, out);
    case 8: return nf_format_u64(bits & 0xFFFFFFFFull, out);
    case 9: return nf_format_u64(bits, out);
    case 10: return nf_format_f32((uint32_t)bits, out);
    case 11: return nf_format_f64(bits, out);
    default: return 0;
  }
}
// the longest cell of a fixed-width type (what the kernel sizes a row's slot by)
DFX_NF int nf_max_cell(int dtype) {
  switch (dtype) {
    case 1: return 5;
    case 2: return 4;
    case 3: return 6;
    case 4: return 11;
    case 5: return 20;
    case 6: return 3;
    case 7: return 5;
    case 8: return 10;
    case 9: return 20;
    case 10: return kNfMaxF32;
    case 11: return kNfMaxF64;
    default: return 0;
  }
}

// ---- Utf8 cells ------------------------------------------------------------------------------------------------------------
DFX_NF bool nf_csv_special(uint8_t c) { return c == ',' || c == '"' || c == '\r' || c == '\n'; }
// the quoting decision of s[0, n): *quotes = the '"' bytes; returns whether the cell holds a byte that needs quotes
DFX_NF bool nf_csv_scan(const uint8_t* s, uint64_t n, uint64_t* quotes) {
  uint64_t q = 0;
  bool special = false;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t c = s[i];
    q += c == '"' ? 1u : 0u;
    special = special || nf_csv_special(c);
  }
  *quotes = q;
  return special;
}
DFX_NF uint64_t nf_csv_cell_len(uint64_t n, uint64_t quotes, bool quoted) { return quoted ? n + quotes + 2 : n; }
// writes the cell; returns nf_csv_cell_len
DFX_NF uint64_t nf_csv_put_cell(const uint8_t* s, uint64_t n, bool quoted, uint8_t* out) {
  if (!quoted) {
    for (uint64_t i = 0; i < n; ++i) out[i] = s[i];
    return n;
  }
  uint64_t o = 0;
  out[o++] = '"';
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t c = s[i];
    if (c == '"') out[o++] = '"';
    out[o++] = c;
  }
  out[o++] = '"';
  return o;
}

}  // namespace dfx
