// agg_rules_check.cpp -- the grouped aggregate's numeric rules (csrc/dfx_agg_rules.hpp) as a stand-alone program: the probing
// block, the grown table, the rebuild and replay-in-place conditions, the fill bound, the window-closing rule, the LDS front cache's
// slots and copies and the spill list's window rows, each against inputs and expected outputs written out by hand.
// tests/test_agg_rules_host.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>

#include "../../datafusion_archive_amd/csrc/dfx_agg_rules.hpp"

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

static void probing_block() {
  struct Row {
    int kw, widest;
    uint64_t cap, slots;
  };
  const Row rows[] = {
      {1, 1, 1ull << 20, 8192},  // 16384 / 2
      {1, 3, 1ull << 20, 4096},  // 16384 / 4
      {2, 1, 1ull << 20, 4096},  // 16384 / 3 = 5461: the power of two below
      {8, 8, 1ull << 20, 1024},
      {1, 1, 1ull << 10, 1024},  // clipped to the table
      {0, 1, 1ull << 20, 8192},  // no key words: taken as one
      {4, 4, 1ull << 20, 2048},
      {3, 2, 1ull << 20, 2048},  // 16384 / 5 = 3276
      {1, 32, 1ull << 20, 256},  // 16384 / 33 = 496
      {1, 1, 32, 32},            // a table below the 64-slot floor
  };
  for (const Row& r : rows) CHECK(probe_block_slots(r.kw, r.widest, r.cap) == r.slots);
}

static void growth() {
  CHECK(ceil_log2(1) == 0);
  CHECK(ceil_log2(2) == 1);
  CHECK(ceil_log2(3) == 2);
  CHECK(ceil_log2(4) == 2);
  CHECK(ceil_log2(5) == 3);
  CHECK(ceil_log2(65536) == 16);
  CHECK(ceil_log2(65537) == 17);
  CHECK(grown_table_log2(14, 9000, 0, 0) == 16);            // 4 x 9001 needs 2^16 as well: never less than two doublings
  CHECK(grown_table_log2(20, 100, 0, 0) == 22);             // the two doublings win
  CHECK(grown_table_log2(14, 9000, 300000, 0) == 21);       // 4 x 309001 = 1236004 > 2^20
  CHECK(grown_table_log2(14, 9000, 300000, 300000) == 16);  // the rows before replay_from are in the table already
  CHECK(grown_table_log2(14, 9000, 300000, 299999) == 16);  // 4 x 9002
  CHECK(grown_table_log2(30, 10, 0, 0) == 32);              // the caller refuses it:
  CHECK(grown_table_log2(30, 10, 0, 0) > 31);
  CHECK(grown_table_log2(29, 10, 0, 0) == 31);              // ... and takes this one
  CHECK(grown_table_log2(10, 1ull << 29, 0, 0) == 32);      // 4 x (2^29 + 1) > 2^31
  CHECK(grown_table_log2(10, (1ull << 29) - 1, 0, 0) == 31);
}

static void rebuild() {
  CHECK(!needs_rebuild(0, 0, 5, 10));
  CHECK(needs_rebuild(1, 0, 5, 10));    // a spilled row
  CHECK(needs_rebuild(0, 1, 5, 10));    // an exhausted probe sequence
  CHECK(!needs_rebuild(0, 0, 10, 10));  // at the load limit
  CHECK(needs_rebuild(0, 0, 11, 10));   // past it
  CHECK(needs_rebuild(1ull << 40, 0, 0, 10));
  // (option, spilled, saturated, occupied, load limit, spill capacity)
  CHECK(replay_in_place_ok(1, 100, 0, 5, 10, 200));  // twice the rows fit the list exactly
  CHECK(!replay_in_place_ok(1, 100, 0, 5, 10, 199));
  CHECK(!replay_in_place_ok(0, 100, 0, 5, 10, 200));  // switched off
  CHECK(!replay_in_place_ok(1, 0, 0, 5, 10, 200));    // nothing spilled
  CHECK(!replay_in_place_ok(1, 100, 1, 5, 10, 200));  // the table is full
  CHECK(replay_in_place_ok(1, 100, 0, 10, 10, 200));
  CHECK(!replay_in_place_ok(1, 100, 0, 11, 10, 200));
}

static void fill_bound() {
  // (old bound, CTRL_MAX_FILL, batch_seq, the snapshot's seq, worst)
  CHECK(fill_bound_after(1000, 100, 5, 4, 50) == 100);  // the snapshot follows the last launch
  CHECK(fill_bound_after(1000, 100, 7, 4, 50) == 200);  // two launches later
  CHECK(fill_bound_after(150, 100, 7, 4, 50) == 150);   // the old bound is the smaller one
  CHECK(fill_bound_after(1000, 100, 4, 4, 50) == 100);  // never fewer than no launches
  CHECK(fill_bound_after(1000, 100, 0, 4, 50) == 100);
  CHECK(fill_bound_after(~0ull, 4000000000u, 3, 0, 4000000000u) == 12000000000ull);  // 64-bit all the way
}

static void window() {
  // (calibrating, pending, agg.partition_defer_batches, pair scan, fill bound, worst, cap_rows)
  CHECK(window_must_close(false, 0, 1, false, 0, 10, 1000));   // a window of one batch
  CHECK(!window_must_close(false, 0, 4, false, 0, 10, 1000));
  CHECK(!window_must_close(false, 2, 4, false, 0, 10, 1000));
  CHECK(window_must_close(false, 3, 4, false, 0, 10, 1000));   // pending + 1 >= 4
  CHECK(window_must_close(false, 7, 4, false, 0, 10, 1000));
  CHECK(!window_must_close(false, 0, 4, false, 980, 10, 1000));  // 980 + 2 x 10 = cap_rows: stays open
  CHECK(window_must_close(false, 0, 4, false, 981, 10, 1000));
  CHECK(window_must_close(true, 0, 4, false, 0, 10, 1000));    // the calibration slice is aggregated at once
  CHECK(window_must_close(true, 0, 8, true, 0, 0, 1000));
  CHECK(!window_must_close(false, 1, 8, false, 0, 10, 1000));
  CHECK(window_must_close(false, 1, 8, true, 0, 10, 1000));    // the pair scan's windows hold two batches
  CHECK(!window_must_close(false, 0, 8, true, 0, 10, 1000));
  CHECK(window_must_close(false, 0, 1, true, 0, 10, 1000));    // ... or one
  CHECK(window_must_close(false, 0, 0, false, 0, 10, 1000));   // an option of 0 counts as 1
  CHECK(window_must_close(false, 0, -3, false, 0, 10, 1000));
  CHECK(window_must_close(false, 0, 0, true, 0, 10, 1000));
  CHECK(window_must_close(false, 0, 4, false, 0, 4294967295u, 4294967295u));  // 2 x worst does not wrap
  CHECK(window_max_batches(8, false) == 8);
  CHECK(window_max_batches(8, true) == 2);
  CHECK(window_max_batches(0, true) == 1);
}

static void front_cache() {
  struct Row {
    int lds_slots, lds_copies;
    bool calibrating, calibrated;
    uint64_t occupied;
    int kw, na, slots, copies;
  };
  const Row rows[] = {
      {-1, -1, false, false, 0, 1, 1, 4096, 1},    // 16 bytes a slot: 64 KB exactly
      {-1, -1, false, false, 0, 1, 2, 2048, 1},    // 24 x 4096 = 96 KB: halved once
      {-1, -1, false, false, 0, 2, 1, 2048, 1},    // (3 x 8 + 4) x 4096 = 112 KB
      {-1, -1, true, false, 0, 1, 1, 512, 1},      // the calibration slice
      {-1, -1, false, true, 10, 1, 1, 4096, 16},   // few groups: sixteen sub-tables of 256 slots
      {-1, -1, false, true, 100, 1, 1, 4096, 4},
      {-1, -1, false, true, 16, 1, 1, 4096, 16},
      {-1, -1, false, true, 17, 1, 1, 4096, 4},
      {-1, -1, false, true, 128, 1, 1, 4096, 4},
      {-1, -1, false, true, 129, 1, 1, 4096, 1},
      {-1, 0, false, true, 10, 1, 1, 4096, 16},    // 0 is "auto" as well
      {128, 16, false, false, 0, 1, 1, 128, 2},    // 128 / 16, / 8, / 4 are below 64 slots a copy; 128 / 2 is 64
      {128, 16, false, true, 10, 1, 1, 128, 2},    // an explicit count is not overridden by the group count
      {-1, -1, false, true, 10, 1, 8, 512, 8},     // 72 bytes a slot: 512 slots, eight copies of 64
      {-1, -1, false, false, 0, 8, 8, 256, 1},     // (16 x 8 + 4) x 512 = 66 KB still exceeds
      {1024, -1, true, false, 0, 1, 1, 1024, 1},   // explicit slots hold for the calibration slice too
      {0, -1, false, true, 10, 1, 1, 0, 1},        // no cache: one copy of nothing
      {8192, -1, false, false, 0, 1, 1, 4096, 1},  // more than fits
      {32, 4, false, false, 0, 1, 1, 32, 1},
  };
  for (const Row& r : rows) {
    const FrontCacheShape s = front_cache_shape(r.lds_slots, r.lds_copies, r.calibrating, r.calibrated, r.occupied, r.kw, r.na);
    CHECK(s.slots == r.slots && s.copies == r.copies);
    if (s.slots != r.slots || s.copies != r.copies)
      printf("  front cache (%d, %d, kw %d, na %d): got {%d, %d}, want {%d, %d}\n", r.lds_slots, r.lds_copies, r.kw, r.na, s.slots, s.copies, r.slots, r.copies);
  }
}

static void spill_window() {
  // (partitioned, pair scan, shared operand, agg.partition_defer_batches, batch rows, rows the regions are laid out for)
  CHECK(spill_window_rows(false, false, false, 8, 1000, 2000) == 0);
  CHECK(spill_window_rows(false, true, false, 8, 1000, 2000) == 0);
  CHECK(spill_window_rows(true, false, false, 4, 1000, 2000) == 8000);  // four batches of the longer length
  CHECK(spill_window_rows(true, false, false, 0, 1000, 500) == 1000);
  CHECK(spill_window_rows(true, false, true, 3, 10, 10) == 30);
  CHECK(spill_window_rows(true, true, false, 8, 1000, 500) == 4000);    // two batches, a row spilled once per operand
  CHECK(spill_window_rows(true, true, true, 8, 1000, 500) == 2000);     // planes of one operand: once
  CHECK(spill_window_rows(true, true, false, 1, 1000, 500) == 2000);
  CHECK(spill_window_rows(true, false, false, 8, (int64_t)1 << 31, 0) == (int64_t)1 << 34);  // 64-bit rows
}

int main() {
  probing_block();
  growth();
  rebuild();
  fill_bound();
  window();
  front_cache();
  spill_window();
  if (failures) {
    printf("%d of %d checks FAILED\n", failures, checks);
    return 1;
  }
  printf("ok: %d checks of the aggregate's numeric rules\n", checks);
  return 0;
}
