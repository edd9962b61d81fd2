// key_shadow_rule.cpp -- the decision rule of the key column's Int32 shadow (csrc/dfx_key_shadow.hpp) as a stand-alone program,
// with the device stubbed: when a shadow is built (the option, the second qualifying query), the memory rule, silent drops,
// rejection for good, slices.  tests/test_key_shadow_rule.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../datafusion_archive_amd/csrc/dfx_key_shadow.hpp"

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
  KeyShadowDevice ops() {
    KeyShadowDevice d;
    d.free_bytes = [this]() { return free_now; };
    d.alloc = [this](size_t bytes) -> std::shared_ptr<void> {
      if (fail_allocs > 0) {
        --fail_allocs;
        return nullptr;
      }
      ++allocs;
      return std::shared_ptr<void>(malloc(bytes), free);
    };
    d.narrow = [this](const void* src, int64_t rows, void* dst, uint32_t* dropped) -> bool {
      if (refuse_narrow) return false;
      ++narrows;
      uint32_t hi = 0;
      for (int64_t i = 0; i < rows; ++i) {
        const uint64_t k = ((const uint64_t*)src)[i];
        hi |= (uint32_t)(k >> 32);
        ((uint32_t*)dst)[i] = (uint32_t)k;
      }
      memset((uint8_t*)dst + (size_t)rows * 4, 0xAB, kKeyShadowPad);  // (the padding is part of the allocation)
      *dropped = hi;
      return true;
    };
    return d;
  }
};

static uint64_t* column(int64_t rows) {
  uint64_t* p = (uint64_t*)aligned_alloc(64, ((size_t)rows * 8 + 63) / 64 * 64);
  for (int64_t i = 0; i < rows; ++i) p[i] = (uint64_t)(i * 2654435761u) & 0xFFFFFFFFull;
  return p;
}

int main() {
  const int64_t rows = 1000 + 77;
  const size_t copy = (size_t)rows * 4 + kKeyShadowPad;
  {  // auto: the second qualifying query builds, the third builds nothing more; later questions of one query never count
    uint64_t* col = column(rows);
    KeyShadows ks;
    ks.add_column(col, rows);
    StubDevice dev;
    dev.free_now = 1 << 20;
    bool built = true;
    CHECK(ks.acquire(col, -1, true, 1000, dev.ops(), &built) == nullptr && !built);
    CHECK(ks.acquire(col, -1, false, 1000, dev.ops(), &built) == nullptr && !built);
    CHECK(ks.acquire(col, -1, false, 1000, dev.ops(), &built) == nullptr);
    int q = 0;
    CHECK(ks.state_of(col, &q) == 0 && q == 1);
    const uint32_t* w = ks.acquire(col, -1, true, 1000, dev.ops(), &built);
    CHECK(w != nullptr && built && dev.narrows == 1);
    for (int64_t i = 0; w && i < rows; ++i) CHECK(w[i] == (uint32_t)col[i]);
    CHECK(ks.acquire(col, -1, true, 1000, dev.ops(), &built) == w && !built && dev.narrows == 1);
    CHECK(ks.bytes_held() == copy);
    // slices: multiples of 64 rows only; outside the column: nothing
    CHECK(ks.acquire(col + 128, -1, false, 0, dev.ops(), &built) == w + 128);
    CHECK(ks.acquire(col + 100, -1, false, 0, dev.ops(), &built) == nullptr);
    CHECK(ks.acquire(col + rows, -1, false, 0, dev.ops(), &built) == nullptr);
    CHECK(ks.acquire(col, 0, true, 0, dev.ops(), &built) == nullptr);  // the option says never: not even read
    free(col);
  }
  {  // option 1: the first query builds; a query's later question cannot
    uint64_t* col = column(rows);
    KeyShadows ks;
    ks.add_column(col, rows);
    StubDevice dev;
    dev.free_now = 1 << 20;
    bool built = false;
    CHECK(ks.acquire(col, 1, false, 0, dev.ops(), &built) == nullptr && !built);
    CHECK(ks.acquire(col, 1, true, 0, dev.ops(), &built) != nullptr && built);
    free(col);
  }
  {  // the memory rule: after the copy as much must stay free as the query holds
    uint64_t* col = column(rows);
    KeyShadows ks;
    ks.add_column(col, rows);
    StubDevice dev;
    bool built = false;
    dev.free_now = copy + 4999;
    CHECK(ks.acquire(col, 1, true, 5000, dev.ops(), &built) == nullptr && dev.allocs == 0);
    dev.free_now = copy - 1;
    CHECK(ks.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && dev.allocs == 0);
    CHECK(ks.state_of(col) == 0);  // dropped silently: the next query asks again
    dev.free_now = copy + 5000;
    CHECK(ks.acquire(col, 1, true, 5000, dev.ops(), &built) != nullptr && built && dev.allocs == 1);
    free(col);
  }
  {  // an allocation that fails, a device that refuses: dropped, asked again
    uint64_t* col = column(rows);
    KeyShadows ks;
    ks.add_column(col, rows);
    StubDevice dev;
    dev.free_now = 1 << 20;
    dev.fail_allocs = 1;
    bool built = false;
    CHECK(ks.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && !built);
    dev.refuse_narrow = true;
    CHECK(ks.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && !built && ks.state_of(col) == 0);
    dev.refuse_narrow = false;
    CHECK(ks.acquire(col, 1, true, 0, dev.ops(), &built) != nullptr && built);
    free(col);
  }
  {  // one key >= 2^32 and one negative key late in the column: the copy is freed, the column never tried again
    for (int which = 0; which < 2; ++which) {
      uint64_t* col = column(rows);
      col[rows - 3] = which ? (uint64_t)-7ll : (1ull << 32) + 5;
      KeyShadows ks;
      ks.add_column(col, rows);
      StubDevice dev;
      dev.free_now = 1 << 20;
      bool built = false;
      CHECK(ks.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && !built && dev.narrows == 1);
      CHECK(ks.state_of(col) == 2 && ks.bytes_held() == 0);
      CHECK(ks.acquire(col, 1, true, 0, dev.ops(), &built) == nullptr && dev.narrows == 1 && dev.allocs == 1);
      free(col);
    }
  }
  {  // boundary keys narrow: 2^32 - 1 and 0; a misaligned or empty column is never registered
    uint64_t* col = column(rows);
    col[0] = 0xFFFFFFFFull;
    col[1] = 0;
    KeyShadows ks;
    ks.add_column(col, rows);
    ks.add_column((const uint8_t*)col + 8, rows - 1);
    ks.add_column(col, 0);
    StubDevice dev;
    dev.free_now = 1 << 20;
    bool built = false;
    const uint32_t* w = ks.acquire(col, 1, true, 0, dev.ops(), &built);
    CHECK(w && w[0] == 0xFFFFFFFFu && w[1] == 0);
    CHECK(ks.state_of((const uint8_t*)col + 8) == -1);
    free(col);
  }
  if (failures) return 1;
  printf("ok: key shadow rule\n");
  return 0;
}
