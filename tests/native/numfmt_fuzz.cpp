// Host build of csrc/dfx_numfmt.hpp (the CSV writer's cell formatter, deviation D11) checked against glibc and against its
// own inverse, csrc/dfx_numparse.hpp.  For every Float64 / Float32 input:
//   (i)   np_parse_f64 / np_parse_f32 of the output returns the input's bits (NaN: a NaN);
//   (ii)  glibc strtod / strtof does too;
//   (iii) no decimal with one significant digit fewer round-trips: the nearest one (%.{p-2}e) and both of its neighbours;
//         and the digits ARE the nearest decimal of their length (%.{p-1}e) whenever that one round-trips: the closest among the shortest;
//   (iv)  the length bounds hold: 24 bytes (Float64), 19 bytes (Float32: -1234567800000000.0);
//   (v)   the layout is positional iff 1e-4 <= |x| < 1e16 or x == 0, with no '+' and no leading zero in an exponent.
// Integers: every type's extremes and random values against snprintf.
// usage: numfmt_fuzz <random inputs per float type> <seed>   -> prints "ok ..." (with the single-core rate) or the first mismatch, exit 1
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <random>
#include <string>
#include <vector>

#include "../../datafusion_archive_amd/csrc/dfx_numfmt.hpp"
#include "../../datafusion_archive_amd/csrc/dfx_numparse.hpp"

static long long n64 = 0, n32 = 0, nint = 0;

struct Parts {
  std::string digits;  // significant digits, no leading / trailing zeros ("" for zero)
  bool sci = false;
  bool ok = true;
};
static Parts split(const std::string& s) {
  Parts p;
  size_t i = 0;
  if (i < s.size() && s[i] == '-') ++i;
  std::string d;
  bool point = false;
  int after_point = 0;
  for (; i < s.size() && s[i] != 'e'; ++i) {
    if (s[i] == '.') {
      if (point) p.ok = false;
      point = true;
    } else if (s[i] >= '0' && s[i] <= '9') {
      d += s[i];
      if (point) ++after_point;
    } else {
      p.ok = false;
    }
  }
  if (i < s.size()) {  // exponent: e[-]digits, no '+', no leading zero
    p.sci = true;
    ++i;
    if (i < s.size() && s[i] == '-') ++i;
    if (i >= s.size() || s[i] == '0' || s[i] == '+') p.ok = false;
    for (; i < s.size(); ++i)
      if (s[i] < '0' || s[i] > '9') p.ok = false;
    if (point && after_point == 0) p.ok = false;
    if (d.size() > 1 && !point) p.ok = false;
  } else if (!point || after_point == 0) {
    p.ok = false;  // positional: at least one digit after the point
  }
  size_t b = d.find_first_not_of('0');
  if (b == std::string::npos) {
    p.digits = "";
    return p;
  }
  size_t e = d.find_last_not_of('0');
  p.digits = d.substr(b, e - b + 1);
  return p;
}

// mantissa digits and exponent of a %.{p-1}e string
static void sci_parts(const char* buf, std::string* mant, int* exp10) {
  mant->clear();
  const char* c = buf;
  if (*c == '-') ++c;
  for (; *c && *c != 'e'; ++c)
    if (*c != '.') *mant += *c;
  *exp10 = atoi(c + 1);
}

template <class F, class U>
static bool check_float(U bits, int max_len, const char* what) {
  F x;
  memcpy(&x, &bits, sizeof x);
  uint8_t out[64];
  memset(out, 0x7f, sizeof out);
  const int len = sizeof(F) == 8 ? dfx::nf_format_f64((uint64_t)bits, out) : dfx::nf_format_f32((uint32_t)bits, out);
  if (len <= 0 || len > max_len || out[len] != 0x7f) {
    printf("MISMATCH %s %llx: length %d beyond the bound %d\n", what, (unsigned long long)bits, len, max_len);
    return false;
  }
  const std::string s((const char*)out, (size_t)len);
  if (x != x) return s == "NaN";
  if (isinf(x)) return s == (x < 0 ? "-inf" : "inf");
  // (i) the library's own reader
  F back = 0;
  const int rc = sizeof(F) == 8 ? dfx::np_parse_f64(out, len, (double*)(void*)&back) : dfx::np_parse_f32(out, len, (float*)(void*)&back);
  if (rc != dfx::NP_OK || memcmp(&back, &x, sizeof x) != 0) {
    printf("MISMATCH %s %llx: '%s' np_parse rc %d gives %.17g\n", what, (unsigned long long)bits, s.c_str(), rc, (double)back);
    return false;
  }
  // (ii) glibc
  const F g = sizeof(F) == 8 ? (F)strtod(s.c_str(), nullptr) : (F)strtof(s.c_str(), nullptr);
  if (memcmp(&g, &x, sizeof x) != 0) {
    printf("MISMATCH %s %llx: '%s' strtod gives %.17g\n", what, (unsigned long long)bits, s.c_str(), (double)g);
    return false;
  }
  // (v) layout
  const Parts p = split(s);
  const F ax = x < 0 ? -x : x;
  const bool positional = x == 0 || (ax >= (F)1e-4 && ax < (F)1e16);
  if (!p.ok || p.sci == positional || (x == 0 && s != (signbit(x) ? "-0.0" : "0.0"))) {
    printf("MISMATCH %s %llx: layout of '%s'\n", what, (unsigned long long)bits, s.c_str());
    return false;
  }
  if (x == 0) return true;
  // (iii) shortest, and the closest of that length
  const int n = (int)p.digits.size();
  char buf[64];
  std::string mant;
  int e10 = 0;
  snprintf(buf, sizeof buf, "%.*e", n - 1, (double)ax);
  sci_parts(buf, &mant, &e10);
  size_t e = mant.find_last_not_of('0');
  // (at a power of two the interval below the value is half as wide: the nearest decimal may lie outside it, and then it is no candidate)
  const F near = sizeof(F) == 8 ? (F)strtod(buf, nullptr) : (F)strtof(buf, nullptr);
  if (mant.substr(0, e + 1) != p.digits && memcmp(&near, &ax, sizeof ax) == 0) {
    printf("MISMATCH %s %llx: '%s' is not the closest %d-digit decimal %s\n", what, (unsigned long long)bits, s.c_str(), n, buf);
    return false;
  }
  if (n >= 2) {
    snprintf(buf, sizeof buf, "%.*e", n - 2, (double)ax);
    sci_parts(buf, &mant, &e10);
    const long long m = atoll(mant.c_str());
    for (long long d = -1; d <= 1; ++d) {
      char cand[64];
      snprintf(cand, sizeof cand, "%llde%d", m + d, e10 - (n - 2));
      const F c = sizeof(F) == 8 ? (F)strtod(cand, nullptr) : (F)strtof(cand, nullptr);
      if (memcmp(&c, &ax, sizeof ax) == 0) {
        printf("MISMATCH %s %llx: '%s' is not shortest, %s round-trips\n", what, (unsigned long long)bits, s.c_str(), cand);
        return false;
      }
    }
  }
  return true;
}

static bool f64(uint64_t b) {
  ++n64;
  return check_float<double, uint64_t>(b, dfx::kNfMaxF64, "f64") && check_float<double, uint64_t>(b ^ (1ull << 63), dfx::kNfMaxF64, "f64");
}
static bool f32(uint32_t b) {
  ++n32;
  return check_float<float, uint32_t>(b, dfx::kNfMaxF32, "f32") && check_float<float, uint32_t>(b ^ (1u << 31), dfx::kNfMaxF32, "f32");
}
static bool around64(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return f64(b) && f64(b + 1) && (b == 0 || f64(b - 1));
}
static bool around32(float d) {
  uint32_t b;
  memcpy(&b, &d, 4);
  return f32(b) && f32(b + 1) && (b == 0 || f32(b - 1));
}

static bool check_int(int dtype, uint64_t bits, long long sv, unsigned long long uv, bool is_signed) {
  uint8_t out[64];
  memset(out, 0x7f, sizeof out);
  const int len = dfx::nf_format_value(dtype, bits, out);
  char want[64];
  if (is_signed) snprintf(want, sizeof want, "%lld", sv);
  else snprintf(want, sizeof want, "%llu", uv);
  ++nint;
  if (len != (int)strlen(want) || memcmp(out, want, (size_t)len) != 0 || out[len] != 0x7f || len > dfx::nf_max_cell(dtype)) {
    printf("MISMATCH int dtype %d: %s formatted as '%.*s'\n", dtype, want, len, (const char*)out);
    return false;
  }
  return true;
}
static bool int_all_types(uint64_t r) {
  return check_int(2, r, (int8_t)r, 0, true) && check_int(3, r, (int16_t)r, 0, true) && check_int(4, r, (int32_t)r, 0, true) &&
         check_int(5, r, (int64_t)r, 0, true) && check_int(6, r, 0, (uint8_t)r, false) && check_int(7, r, 0, (uint16_t)r, false) &&
         check_int(8, r, 0, (uint32_t)r, false) && check_int(9, r, 0, r, false);
}

int main(int argc, char** argv) {
  const long long iters = argc > 1 ? atoll(argv[1]) : 2000000;
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
  // the special list: zeros, infinities, NaNs, the subnormal range's ends, the extremes, the layout thresholds
  const uint64_t s64[] = {0ull, 0x7FF0000000000000ull, 0x7FF8000000000000ull, 0x7FF0000000000001ull, 0x7FFFFFFFFFFFFFFFull,
                          1ull, 2ull, 0x000FFFFFFFFFFFFFull, 0x0010000000000000ull, 0x0010000000000001ull, 0x7FEFFFFFFFFFFFFFull,
                          0x3FF0000000000000ull, 0x3FB999999999999Aull, 0x4340000000000000ull, 0x433FFFFFFFFFFFFFull};
  for (uint64_t b : s64)
    if (!f64(b)) return 1;
  const uint32_t s32[] = {0u, 0x7F800000u, 0x7FC00000u, 0x7F800001u, 0x7FFFFFFFu, 1u, 2u, 0x007FFFFFu, 0x00800000u, 0x00800001u,
                          0x7F7FFFFFu, 0x3F800000u, 0x3DCCCCCDu, 0x4B800000u, 0x4B7FFFFFu};
  for (uint32_t b : s32)
    if (!f32(b)) return 1;
  if (!around64(1e-4) || !around64(1e16) || !around64(9.999999999999999e-5) || !around64(9999999999999998.0)) return 1;
  if (!around32(1e-4f) || !around32(1e16f) || !around32(9.999999e-5f) || !around32(9.999999e15f)) return 1;
  for (uint64_t e = 0; e < 2047; ++e)  // every power of two (e == 0: the subnormal ones below)
    if (!f64(e << 52) || !f64((e << 52) | 1) || (e > 0 && !f64((e << 52) - 1))) return 1;
  for (int i = 0; i < 52; ++i)
    if (!f64(1ull << i) || !f64((1ull << i) + 1) || !f64((1ull << i) - 1)) return 1;
  for (uint32_t e = 0; e < 255; ++e)
    if (!f32(e << 23) || !f32((e << 23) | 1) || (e > 0 && !f32((e << 23) - 1))) return 1;
  for (int i = 0; i < 23; ++i)
    if (!f32(1u << i) || !f32((1u << i) + 1) || !f32((1u << i) - 1)) return 1;
  char buf[64];
  for (int k = -324; k <= 308; ++k) {  // every power of ten and its two neighbours
    snprintf(buf, sizeof buf, "1e%d", k);
    if (!around64(strtod(buf, nullptr))) return 1;
    if (k >= -46 && k <= 38 && !around32(strtof(buf, nullptr))) return 1;
  }
  const long long special64 = n64, special32 = n32;
  for (long long i = 0; i < iters / 8; ++i)  // the subnormal range
    if (!f64(rng() & 0x000FFFFFFFFFFFFFull) || !f32((uint32_t)rng() & 0x007FFFFFu)) return 1;
  for (long long i = 0; i < iters; ++i)  // uniformly random bit patterns
    if (!f64(rng()) || !f32((uint32_t)rng())) return 1;
  // integers: the extremes of every type, then random values
  const uint64_t ext[] = {0ull, 1ull, 0x7Full, 0x80ull, 0xFFull, 0x7FFFull, 0x8000ull, 0xFFFFull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull,
                          0x7FFFFFFFFFFFFFFFull, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull, 9ull, 10ull, 99ull, 100ull, 9999ull, 10000ull,
                          9999999999ull, 10000000000ull, 9999999999999999999ull, 10000000000000000000ull};
  for (uint64_t b : ext)
    if (!int_all_types(b)) return 1;
  for (long long i = 0; i < iters / 2; ++i) {
    const uint64_t r = rng() >> (rng() % 64);  // every magnitude
    if (!int_all_types(r) || !int_all_types(0ull - r)) return 1;
  }
  // Utf8 quoting: the written cell is the input with quotes doubled, wrapped iff it holds a special byte
  const char* strs[] = {"", "plain", "a,b", "\"", "\"\"", "say \"hi\"", "line\nbreak", "cr\rhere", "\"lead", "trail\"", "gr\xc3\xbc\xc3\x9f, dich"};
  for (const char* t : strs) {
    const uint64_t n = strlen(t);
    uint64_t q = 0;
    const bool sp = dfx::nf_csv_scan((const uint8_t*)t, n, &q);
    uint8_t cell[64];
    const uint64_t l = dfx::nf_csv_put_cell((const uint8_t*)t, n, sp, cell);
    std::string want;
    bool any = false;
    for (const char* c = t; *c; ++c) {
      any = any || strchr(",\"\r\n", *c) != nullptr;
      if (*c == '"') want += '"';
      want += *c;
    }
    if (any) want = "\"" + want + "\"";
    if (sp != any || l != dfx::nf_csv_cell_len(n, q, sp) || std::string((const char*)cell, (size_t)l) != want) {
      printf("MISMATCH utf8 cell of '%s'\n", t);
      return 1;
    }
  }
  // the single-core rate of the formatter alone (no checks): random Float64 bit patterns
  std::vector<uint64_t> v(1 << 20);
  for (auto& b : v) b = rng();
  uint8_t out[64];
  unsigned long long sink = 0, keep = 0;
  const clock_t t0 = clock();
  for (int rep = 0; rep < 8; ++rep)
    for (uint64_t b : v) {
      sink += (unsigned)dfx::nf_format_f64(b, out);
      keep ^= out[1];
    }
  const double sec = (double)(clock() - t0) / CLOCKS_PER_SEC;
  printf("ok: %lld Float64 and %lld Float32 inputs (%lld / %lld special, each with both signs) round-trip through np_parse and strtod, are shortest and closest, "
         "within 24 / 19 bytes; %lld integers agree with snprintf; host formatter: %.3g Float64 cells/s on one core (%.1f bytes/cell)\n",
         n64, n32, special64, special32, nint, (double)v.size() * 8 / (sec > 0 ? sec : 1e-9), (double)sink / (8.0 * (double)v.size()) + 0.0 * (double)(keep & 1));
  return 0;
}
