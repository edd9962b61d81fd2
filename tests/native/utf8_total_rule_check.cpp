// utf8_total_rule_check.cpp -- the rule a Utf8 column's byte total is judged by and the slot of a scan's 64-bit grand total
// (csrc/dfx_scan_rules.hpp) as a stand-alone program, each against values written out by hand.  The totals include the ones an int32
// read-back of the last offset misjudged: 2^32 and beyond come back as small positive numbers.
// tests/test_utf8_total_rule_host.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>

#include "../../datafusion_archive_amd/csrc/dfx_scan_rules.hpp"

using namespace dfx;

static int failures = 0, checks = 0;
#define CHECK(cond)                                    \
  do {                                                 \
    ++checks;                                          \
    if (!(cond)) {                                     \
      printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++failures;                                      \
    }                                                  \
  } while (0)

static void total_rule() {
  CHECK(!utf8_total_exceeds_offsets(0));
  CHECK(!utf8_total_exceeds_offsets((1ull << 31) - 1));  // the largest int32 offset: fits
  CHECK(utf8_total_exceeds_offsets(1ull << 31));         // negative as int32
  CHECK(utf8_total_exceeds_offsets((1ull << 32) - 1));   // -1 as int32
  CHECK(utf8_total_exceeds_offsets(1ull << 32));         // 0 as int32
  CHECK(utf8_total_exceeds_offsets((1ull << 32) + 5));   // 5 as int32
  CHECK(utf8_total_exceeds_offsets(3ull << 31));         // three 1.5 GB batches: 2^31 as uint32
  // what the old judgement (`(int32_t)total < 0`) said of the same sums: it let the wrapped ones through
  CHECK((int32_t)(uint32_t)(1ull << 32) >= 0 && (int32_t)(uint32_t)((1ull << 32) + 5) >= 0);
}

static void total_slot() {
  struct Row {
    int64_t n, blocks;
  };
  const Row rows[] = {{0, 1}, {1, 1}, {4095, 1}, {4096, 1}, {4097, 2}, {(int64_t)1 << 24, 4096}};
  for (const Row& r : rows) {
    CHECK(scan_blocks(r.n) == r.blocks);
    CHECK(scan_blocks(r.n) == (r.n > 0 ? (r.n + 4096 - 1) / 4096 : 1));  // the launcher's grid (scan_impl, dfx_k_core.hip)
    CHECK(scan_blocks(r.n) >= 1);                                        // slot 0 is a block's sum, never the total
    CHECK(scan_blocks(r.n) < r.n / 4096 + 4);                            // inside the words every caller allocates
  }
  CHECK(kScanChunk == 4096);
}

int main() {
  total_rule();
  total_slot();
  if (failures) {
    printf("%d of %d checks FAILED\n", failures, checks);
    return 1;
  }
  printf("ok: %d checks of the Utf8 total rule and the scan's total slot\n", checks);
  return 0;
}
