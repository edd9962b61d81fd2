// value_shadow_rule.cpp -- the decision rule of an operand column's Float32 shadow (csrc/dfx_value_shadow.hpp) as a stand-alone
// program, with the device stubbed: when a shadow is built (the option, the second qualifying query), the memory rule at its
// boundary, silent drops, the refusal that lasts, slices, two columns of one table.  The stub applies the build kernel's
// exactness rule on the host.  tests/test_value_shadow_rule.py builds it plain and with -fsanitize=address,undefined.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../datafusion_archive_amd/csrc/dfx_value_shadow.hpp"

using namespace dfx;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                    \
    }                                                                \
  } while (0)

struct StubDevice {  // host memory stands in for HBM
  size_t free_now = 0;
  int allocs = 0, narrows = 0, fail_allocs = 0;
  bool refuse_narrow = false;
  ValueShadowDevice ops() {
    ValueShadowDevice d;
    d.free_bytes = [this]() { return free_now; };
    d.alloc = [this](size_t bytes) -> std::shared_ptr<void> {
      if (fail_allocs > 0) {
        --fail_allocs;
        return nullptr;
      }
      ++allocs;
      return std::shared_ptr<void>(malloc(bytes), free);
    };
    d.narrow = [this](const void* src, int64_t rows, void* dst, uint32_t* inexact) -> bool {
      if (refuse_narrow) return false;
      ++narrows;
      uint32_t bad = 0;
      for (int64_t i = 0; i < rows; ++i) {
        const double v = ((const double*)src)[i];
        // (a finite value beyond the Float32 range is refused like any other inexact one; the cast itself must stay defined here)
        const float f = isnan(v) || (isfinite(v) && fabs(v) > 3.5e38) ? 0.0f : (float)v;
        const double back = (double)f;
        uint32_t w;
        memcpy(&w, &f, 4);
        const bool denormal = (w & 0x7F800000u) == 0 && (w & 0x007FFFFFu) != 0;
        if (memcmp(&back, &v, 8) != 0 || isnan(v) || denormal) bad = 1;
        ((uint32_t*)dst)[i] = w;
      }
      memset((uint8_t*)dst + (size_t)rows * 4, 0xAB, kValueShadowPad);  // (the padding is part of the allocation)
      *inexact = bad;
      return true;
    };
    return d;
  }
};

static double* column(int64_t rows, double scale = 1.0 / 1024.0) {
  double* p = (double*)aligned_alloc(64, ((size_t)rows * 8 + 63) / 64 * 64);
  for (int64_t i = 0; i < rows; ++i) p[i] = (double)((uint64_t)(i * 2654435761u) & 0xFFFFFull) * scale;  // m * 2^-10, m < 2^20
  return p;
}
static float word(const uint32_t* w, int64_t i) {
  float f;
  memcpy(&f, w + i, 4);
  return f;
}

int main() {
  const int64_t rows = 1000 + 77;
  const size_t copy = (size_t)rows * 4 + kValueShadowPad;
  {  // auto: the second qualifying query builds, the third builds nothing more; later questions of one query never count
    double* col = column(rows);
    ValueShadows vs;
    vs.add_column(col, rows);
    StubDevice dev;
    dev.free_now = 1 << 20;
    bool built = true;
    CHECK(vs.acquire(col, -1, true, 1000, dev.ops(), &built) == nullptr && !built);
    CHECK(vs.acquire(col, -1, false, 1000, dev.ops(), &built) == nullptr && !built);
    int q = 0;
    CHECK(vs.state_of(col, &q) == 0 && q == 1);
    const uint32_t* w = vs.acquire(col, -1, true, 1000, dev.ops(), &built);
    CHECK(w != nullptr && built && dev.narrows == 1);
    for (int64_t i = 0; w && i < rows; ++i) CHECK((double)word(w, i) == col[i]);
    CHECK(vs.acquire(col, -1, true, 1000, dev.ops(), &built) == w && !built && dev.narrows == 1);
    CHECK(vs.bytes_held() == copy && vs.state_of(col) == 1);
    // slices: multiples of 64 rows only; outside the column: nothing
    CHECK(vs.acquire(col + 64 * 3, -1, false, 0, dev.ops(), &built) == w + 64 * 3);
    CHECK(vs.acquire(col + 100, -1, false, 0, dev.ops(), &built) == nullptr);
    CHECK(vs.acquire(col + rows, -1, false, 0, dev.ops(), &built) == nullptr);
    CHECK(vs.acquire(col, 0, true, 0, dev.ops(), &built) == nullptr);  // the option says never: not even read
    free(col);
  }
  {  // option 0 never builds; option 1: the first query builds, a query's later question cannot
    double* col = column(rows);
    ValueShadows vs;
    vs.add_column(col, rows);
    StubDevice dev;
    dev.free_now = 1 << 20;
    bool built = false;
    for (int q = 0; q < 3; ++q) CHECK(vs.acquire(col, 0, true, 0, dev.ops(), &built) == nullptr && !built);
    CHECK(dev.allocs == 0 && dev.narrows == 0 && vs.state_of(col) == 0);
    CHECK(vs.acquire(col, 1, false, 0, dev.ops(), &built) == nullptr && !built);
    CHECK(vs.acquire(col, 1, true, 0, dev.ops(), &built) != nullptr && built);
    free(col);
  }
  {  // the memory rule at its boundary: after the copy as much must stay free as the query holds
    double* col = column(rows);
    ValueShadows vs;
    vs.add_column(col, rows);
    StubDevice dev;
    bool built = false;
    dev.free_now = copy + 4999;
    CHECK(vs.acquire(col, 1, true, 5000, dev.ops(), &built) == nullptr && dev.allocs == 0);
    dev.free_now = copy - 1;
    CHECK(vs.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && dev.allocs == 0);
    CHECK(vs.state_of(col) == 0);  // dropped silently: the next query asks again
    dev.free_now = copy + 5000;
    CHECK(vs.acquire(col, 1, true, 5000, dev.ops(), &built) != nullptr && built && dev.allocs == 1);
    free(col);
  }
  {  // an allocation that fails, a device that refuses: dropped, the column stays eligible
    double* col = column(rows);
    ValueShadows vs;
    vs.add_column(col, rows);
    StubDevice dev;
    dev.free_now = 1 << 20;
    dev.fail_allocs = 1;
    bool built = false;
    CHECK(vs.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && !built && vs.state_of(col) == 0);
    dev.refuse_narrow = true;
    CHECK(vs.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && !built && vs.state_of(col) == 0 && vs.bytes_held() == 0);
    dev.refuse_narrow = false;
    CHECK(vs.acquire(col, 1, true, 0, dev.ops(), &built) != nullptr && built);
    free(col);
  }
  {  // one value late in the column that is not exactly a normal float: the copy is freed, the column never tried again
    const double odd[5] = {1.0 + ldexp(1.0, -24) /* 25-bit mantissa */, NAN, ldexp(1.0, -140) /* Float32 denormal */, 1e300, 0.1};
    for (int which = 0; which < 5; ++which) {
      double* col = column(rows);
      col[rows - 3] = odd[which];
      ValueShadows vs;
      vs.add_column(col, rows);
      StubDevice dev;
      dev.free_now = 1 << 20;
      bool built = false;
      CHECK(vs.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && !built && dev.narrows == 1);
      CHECK(vs.state_of(col) == 2 && vs.bytes_held() == 0);
      CHECK(vs.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && dev.narrows == 1 && dev.allocs == 1);
      free(col);
    }
  }
  {  // +-0, +-infinity, the largest and the smallest normal float are exact; a misaligned or empty column is never registered
    double* col = column(rows);
    const double fine[6] = {0.0, -0.0, INFINITY, -INFINITY, (double)3.4028234663852886e38f, ldexp(1.0, -126)};
    for (int i = 0; i < 6; ++i) col[i] = fine[i];
    ValueShadows vs;
    vs.add_column(col, rows);
    vs.add_column((const uint8_t*)col + 8, rows - 1);
    vs.add_column(col, 0);
    StubDevice dev;
    dev.free_now = 1 << 20;
    bool built = false;
    const uint32_t* w = vs.acquire(col, 1, true, 0, dev.ops(), &built);
    CHECK(w && built);
    for (int i = 0; w && i < 6; ++i) {
      const double back = (double)word(w, i);
      CHECK(memcmp(&back, &fine[i], 8) == 0);
    }
    CHECK(vs.state_of((const uint8_t*)col + 8) == -1);
    free(col);
  }
  {  // two columns of one table: each its own count, copy and verdict
    double* a = column(rows);
    double* b = column(rows, 0.1);  // (multiples of 0.1: not Float32-exact)
    ValueShadows vs;
    vs.add_column(a, rows);
    vs.add_column(b, rows);
    StubDevice dev;
    dev.free_now = 1 << 20;
    bool built = false;
    CHECK(vs.acquire(a, -1, true, 0, dev.ops(), &built) == nullptr);
    CHECK(vs.acquire(b, -1, true, 0, dev.ops(), &built) == nullptr && dev.narrows == 0);
    const uint32_t* wa = vs.acquire(a, -1, true, 0, dev.ops(), &built);
    CHECK(wa != nullptr && built && vs.state_of(b) == 0);
    CHECK(vs.acquire(b, -1, true, 0, dev.ops(), &built) == nullptr && !built && vs.state_of(b) == 2);
    CHECK(vs.acquire(a, -1, true, 0, dev.ops(), &built) == wa && vs.state_of(a) == 1 && vs.bytes_held() == copy);
    free(a);
    free(b);
  }
  if (failures) return 1;
  printf("ok: value shadow rule\n");
  return 0;
}
