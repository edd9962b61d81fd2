// row8_layout_check.cpp -- the 8-byte routed row form (PTF_ROW8) as a stand-alone program: choose_routed_layout
// (csrc/dfx_pass1_layout.hpp) and choose_pass2 (csrc/dfx_pass2_forms.hpp) against values written out by hand for the headline's
// table -- 256 table blocks of 8192 slots, 256 producers, batches of 2^27 rows --, the shapes that must NOT get the form, and the
// LDS bytes of the wave-specialised pass 1 for both scanner splits.
// tests/test_row8_layout.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <string.h>

#include "../../datafusion_archive_amd/csrc/dfx_pass1_layout.hpp"
#include "../../datafusion_archive_amd/csrc/dfx_pass2_forms.hpp"

using namespace dfx;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// One narrow key, SUM(v), 2^27-row batches, 256 blocks of 8192 slots, 256 CUs, the defaults of AggOptions (dfx_relation.hpp).
static RoutedLayoutQuery headline(bool both_shadows) {
  RoutedLayoutQuery q = {};
  q.rows = (int64_t)1 << 27, q.kw = 1, q.na = 1;
  q.block_slots = 8192, q.table_slots = (uint64_t)256 * 8192, q.cu_count = 256;
  q.phase = PairPhase::none;
  q.narrow = true;
  q.has_pred = true;
  q.opt.narrow_keys = -1, q.opt.narrow_chunk16 = 1, q.opt.hot_keys = -1, q.opt.pass2_stream = 1;
  q.opt.pass1_ws = 8, q.opt.pass1_ws_dense = 0, q.opt.pass1_ws_dense_scanners = 4;
  q.opt.partition_mode = 2, q.opt.partition_layout = 1, q.opt.partition_block = 1024;
  q.both_shadows = both_shadows;
  return q;
}

static void no_flag(int line, const RoutedLayoutQuery& q) {
  const RoutedLayout r = choose_routed_layout(q);
  if ((r.PT.flags & PTF_ROW8) || (r.want_flags & PTF_ROW8)) {
    printf("FAILED line %d: PTF_ROW8 set (flags %u, want %u)\n", line, r.PT.flags, r.want_flags);
    ++failures;
  }
}

int main() {
  static_assert(kNarrowLine, "the form exists in the LINE-chunk geometry only");
  static_assert(kRow8ChunkRows * kRow8Dwords * 4 == 128 && kRow8RingRows / kRow8ChunkRows == 3, "sixteen rows are one line; three ring slots");
  static_assert(kRow8TripRows * kRow8Dwords * 4 == (int)kRow8TripBytes && kRow8CapQuantum % kRow8ChunkRows == 0 && kRow8CapQuantum % kRow8TripRows == 0,
                "a trip is 64 rows of 8 bytes; the quantum is whole lines and whole trips");
  static_assert(PTF_ROW8 == 2048u, "the flag's value");

  // ---- the 12-byte layout of the same query: the input false reproduces it (the default) ---------------------------------------
  const RoutedLayout r12 = choose_routed_layout(headline(false));
  CHECK(r12.kind == RoutedLayoutKind::ring16 && r12.PT.flags == (PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_STREAM_PASS2));
  CHECK(r12.want_flags == PTF_NARROW);
  CHECK(r12.PT.cap_rows == 4480 && r12.worst == 4480 && r12.PT.win_stride == 96 && r12.PT.part_stride == 7168 && r12.PT.prod_stride == 1835008);
  CHECK(r12.row_bytes == (size_t)3758096384ull);
  {
    RoutedLayoutQuery q = headline(false);
    RoutedLayoutQuery d = {};
    CHECK(!d.both_shadows);  // the default
    (void)q;
  }

  // ---- flag on -------------------------------------------------------------------------------------------------------------------
  const RoutedLayout r8 = choose_routed_layout(headline(true));
  CHECK(r8.kind == RoutedLayoutKind::ring16);
  CHECK(r8.PT.flags == (PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_STREAM_PASS2 | PTF_ROW8));
  CHECK(r8.want_flags == (PTF_NARROW | PTF_ROW8));
  CHECK(r8.PT.n_parts == 256 && r8.PT.n_producers == 256 && r8.PT.n_words == 2 && r8.PT.ws_scanners == 8 && r8.PT.mode == 2 && r8.PT.block == 1024);
  // avg = 2^27 / 65536 + 1 = 2049; worst = ceil((4098 + 64) / 64) * 64 = 4224; one batch per window
  CHECK(r8.worst == 4224 && r8.PT.cap_rows == 4224 && r8.PT.cap_rows % kRow8CapQuantum == 0);
  CHECK(r8.PT.win_stride == 64);                                  // words: 64 rows x 8 bytes
  CHECK(r8.PT.part_stride == (uint64_t)r8.PT.cap_rows * 8 / 8);   // region_words
  CHECK(r8.PT.part_stride == 4224 && r8.PT.prod_stride == 1081344);
  CHECK(r8.row_bytes == (size_t)2214592512ull && r8.cnt_bytes == 262144);
  CHECK(3 * r8.row_bytes <= 2 * r12.row_bytes);
  CHECK(partition_launchable(r8.PT) && partition_stage_bytes(r8.PT) == 130240);
  CHECK(partition_row8_consistent(r8.PT.flags | PTF_KEY4 | PTF_VAL4));
  CHECK(!partition_row8_consistent(r8.PT.flags) && !partition_row8_consistent(r8.PT.flags | PTF_KEY4));  // never without PTF_VAL4
  CHECK(!partition_row8_consistent(r8.PT.flags | PTF_KEY4 | PTF_VAL4 | PTF_SHARED));
  CHECK(partition_row8_consistent(r12.PT.flags) && partition_row8_consistent(r12.PT.flags | PTF_KEY4 | PTF_VAL4));
  {  // the dense split: four scanners, twelve queues
    RoutedLayoutQuery q = headline(true);
    q.has_pred = false, q.mostly_seen = true;
    const RoutedLayout d = choose_routed_layout(q);
    CHECK((d.PT.flags & PTF_ROW8) && d.PT.ws_scanners == 4 && partition_stage_bytes(d.PT) == 138496);
  }
  {  // tiny regions (tests): one quantum
    RoutedLayoutQuery q = headline(true);
    q.opt.partition_cap_rows = 1;
    const RoutedLayout d = choose_routed_layout(q);
    CHECK((d.PT.flags & PTF_ROW8) && d.PT.cap_rows == 64 && d.PT.part_stride == 64 && d.PT.win_stride == 64);
    q.both_shadows = false;
    CHECK(choose_routed_layout(q).PT.cap_rows == 320);
  }
  {  // a pad keeps every region on a line
    RoutedLayoutQuery q = headline(true);
    q.opt.partition_pad = 8;
    const RoutedLayout d = choose_routed_layout(q);
    CHECK(d.PT.prod_stride == 1081344 + 16 && d.PT.prod_stride % 16 == 0 && d.PT.part_stride % 16 == 0);
  }

  // ---- pass 1's LDS: 4 bytes less per queue row, within the budget for both splits -------------------------------------------------
  CHECK(partition_ws_bytes(256, 8) == 138432 && partition_ws_bytes(256, 4) == 150784);
  CHECK(partition_ws_bytes(256, 8, 1, true) == 138432 - 8 * kWsQueueRows * 4 && partition_ws_bytes(256, 4, 1, true) == 150784 - 12 * kWsQueueRows * 4);
  CHECK(partition_ws_bytes(256, 8, 1, true) <= kPass1LdsBudget && partition_ws_bytes(256, 4, 1, true) <= kPass1LdsBudget);

  // ---- pass 2: the narrow form over rows of its own, narrow's LDS (a parked row is widened first: twelve bytes) ------------------
  {
    const Pass2Choice c = choose_pass2(r8.PT.flags, 1, 1, r8.PT.n_words, 8192, r8.PT.n_producers, 0, kNarrowLine);
    CHECK(c.form == Pass2Form::narrow && c.n_launches == 1 && c.launch[0].rows == Pass2Rows::narrow8);
    CHECK(c.lds_bytes == 8192 * 12 + 16 * 128 * 12 && c.lds_bytes == pass2_lds_bytes(Pass2Form::narrow, 8192, 1, 256) && c.lds_bytes <= kP2LdsLimit);
    const Pass2Choice c12 = choose_pass2(r12.PT.flags, 1, 1, r12.PT.n_words, 8192, r12.PT.n_producers, 0, kNarrowLine);
    CHECK(c12.form == Pass2Form::narrow && c12.launch[0].rows == Pass2Rows::narrow && c12.lds_bytes == c.lds_bytes);
    CHECK(choose_pass2(r8.PT.flags, 2, 1, 2, 8192, 256, 0, kNarrowLine).form == Pass2Form::refused);
    CHECK(choose_pass2(r8.PT.flags, 1, 1, 2, 8192, 256, 0, false).form == Pass2Form::refused);
    CHECK(choose_pass2(r8.PT.flags & ~PTF_CHUNK16, 1, 1, 2, 8192, 256, 0, kNarrowLine).form == Pass2Form::refused);
  }

  // ---- the shapes that keep their rows ---------------------------------------------------------------------------------------------
  no_flag(__LINE__, headline(false));
  {
    RoutedLayoutQuery q = headline(true);  // two aggregates of different operands (no pair scan: ring8 / sort rows)
    q.na = 2;
    no_flag(__LINE__, q);
  }
  {
    RoutedLayoutQuery q = headline(true);  // the shared operand
    q.na = 2, q.shared_operand = q.same_operand_all = true, q.split_distinct = 1;
    no_flag(__LINE__, q);
    q.phase = PairPhase::planes;           // ... and its planes
    no_flag(__LINE__, q);
  }
  {
    RoutedLayoutQuery q = headline(true);  // the pair phase
    q.na = 2, q.phase = PairPhase::pair, q.split_distinct = 2, q.split_ops = 2, q.split_arg1 = 1;
    no_flag(__LINE__, q);
    CHECK(choose_routed_layout(q).kind == RoutedLayoutKind::pair_rows);
  }
  {
    RoutedLayoutQuery q = headline(true);  // hot keys
    q.opt.hot_keys = 1;
    no_flag(__LINE__, q);
    CHECK(choose_routed_layout(q).PT.flags & PTF_HOT);
    q.opt.hot_keys = -1, q.skew_seen = true;
    no_flag(__LINE__, q);
  }
  {
    RoutedLayoutQuery q = headline(true);  // the windowed scratch layout
    q.opt.partition_layout = 2;
    no_flag(__LINE__, q);
  }
  {
    RoutedLayoutQuery q = headline(true);  // wide keys
    q.narrow = false;
    no_flag(__LINE__, q);
    q.narrow = true, q.opt.narrow_keys = 0;
    no_flag(__LINE__, q);
  }
  {
    RoutedLayoutQuery q = headline(true);  // no wave-specialised kernel, no large chunks, two key words
    q.opt.pass1_ws = 0;
    no_flag(__LINE__, q);
    q.opt.pass1_ws = 8, q.opt.narrow_chunk16 = 0;
    no_flag(__LINE__, q);
    q.opt.narrow_chunk16 = 1, q.kw = 2;
    no_flag(__LINE__, q);
  }

  if (failures) {
    printf("%d check(s) failed\n", failures);
    return 1;
  }
  printf("ok: row8 layout, LDS and pass-2 form\n");
  return 0;
}
