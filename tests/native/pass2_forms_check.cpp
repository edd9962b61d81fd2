// pass2_forms_check.cpp -- the forms of pass 2 of the partitioned GROUP BY and their choice (csrc/dfx_pass2_forms.hpp) as a
// stand-alone program: choose_pass2 over every combination of the five flags that matter, na 1..8, kw 1..2, n_words 2..3, table
// blocks of 4096 and 8192 slots and (pair forms) every operand pattern, against tables written out by hand from the if-chain of
// launch_partition_agg that this function replaced.  tests/test_pass2_forms.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <string.h>

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

// What the flag word alone decided in the old chain: F the flat kernels (or, one aggregate of 16-byte rows under
// PTF_STREAM_PASS2, the streamed wide form), S shared operand, L one launch per plane of a shared operand, R pair, N narrow.
// flat_check: the flat kernels' LDS bytes were checked first -- not under PTF_PAIR / PTF_PLANES, whatever branch followed.
struct FlagRow {
  bool narrow, shared, planes, pair, stream;
  char branch;
  bool flat_check;
};
static const FlagRow kFlagRows[32] = {
    // narrow shared planes pair stream
    {0, 0, 0, 0, 0, 'F', true},  {1, 0, 0, 0, 0, 'N', true},  {0, 1, 0, 0, 0, 'F', true},  {1, 1, 0, 0, 0, 'S', true},
    {0, 0, 1, 0, 0, 'F', false}, {1, 0, 1, 0, 0, 'N', false}, {0, 1, 1, 0, 0, 'F', false}, {1, 1, 1, 0, 0, 'L', false},
    {0, 0, 0, 1, 0, 'F', false}, {1, 0, 0, 1, 0, 'R', false}, {0, 1, 0, 1, 0, 'F', false}, {1, 1, 0, 1, 0, 'S', false},
    {0, 0, 1, 1, 0, 'F', false}, {1, 0, 1, 1, 0, 'R', false}, {0, 1, 1, 1, 0, 'F', false}, {1, 1, 1, 1, 0, 'L', false},
    {0, 0, 0, 0, 1, 'F', true},  {1, 0, 0, 0, 1, 'N', true},  {0, 1, 0, 0, 1, 'F', true},  {1, 1, 0, 0, 1, 'S', true},
    {0, 0, 1, 0, 1, 'F', false}, {1, 0, 1, 0, 1, 'N', false}, {0, 1, 1, 0, 1, 'F', false}, {1, 1, 1, 0, 1, 'L', false},
    {0, 0, 0, 1, 1, 'F', false}, {1, 0, 0, 1, 1, 'R', false}, {0, 1, 0, 1, 1, 'F', false}, {1, 1, 0, 1, 1, 'S', false},
    {0, 0, 1, 1, 1, 'F', false}, {1, 0, 1, 1, 1, 'R', false}, {0, 1, 1, 1, 1, 'F', false}, {1, 1, 1, 1, 1, 'L', false},
};

// LDS bytes, [block: 4096 / 8192 slots].  256 producers.
static const size_t kLimit = 163584;  // 160 KB - 256
// flat kernels: slots x (1 + na) x 8 + 257 x 4 + 16, na = 1..8
static const size_t kFlatBytes[2][8] = {{66580, 99348, 132116, 164884, 197652, 230420, 263188, 295956},
                                        {132116, 197652, 263188, 328724, 394260, 459796, 525332, 590868}};
static const size_t kStreamWideBytes[2] = {90112, 155648};  // slots x 16 + 16 waves x 96 rows x 16
static const size_t kNarrowBytes[2] = {73728, 122880};      // slots x 12 + 16 waves x 128 rows x 12: narrow, planes, pair
static const size_t kSharedBytes[2][2] = {{106496, 139264}, {188416, 253952}};  // slots x (4 + 8 na) + the same queues, na = 2, 3

struct Want {
  const char* form;  // "refused" or a form's name
  size_t lds = 0;
  int n = 0;
  bool lean = true;  // a launch of k_partition_agg_lean: the row form matters
  Pass2Rows rows[kMaxAggs] = {};
  uint32_t operand[kMaxAggs] = {}, spills[kMaxAggs] = {};
  bool snap[kMaxAggs] = {};
};

// the old chain, branch by branch
static Want expected(const FlagRow& f, int na, int kw, uint32_t n_words, int blk, uint32_t pair_ops, bool narrow_line) {
  Want w;
  w.form = "refused";
  if (f.flat_check && kFlatBytes[blk][na - 1] > kLimit) return w;
  const auto one = [&](const char* form, size_t lds, Pass2Rows rows) {
    w.form = form;
    w.lds = lds;
    w.n = 1;
    w.rows[0] = rows;
    w.snap[0] = true;
  };
  switch (f.branch) {
    case 'S':
      if (na < 2 || na > 3 || kw != 1 || kSharedBytes[blk][na - 2] > kLimit) return w;
      one("shared_operand", kSharedBytes[blk][na - 2], Pass2Rows::narrow);
      break;
    case 'L':
      if (na < 2 || kw != 1) return w;
      w.form = "planes";
      w.lds = kNarrowBytes[blk];
      w.n = na;
      for (int a = 0; a < na; ++a) {
        w.rows[a] = Pass2Rows::narrow_xf;
        w.spills[a] = a == na - 1;
        w.snap[a] = a == na - 1;
      }
      break;
    case 'R':
      if (na < 2 || kw != 1 || !narrow_line) return w;
      w.form = f.planes ? "pair_planes" : "pair";
      w.lds = kNarrowBytes[blk];
      w.n = na;
      for (int a = 0; a < na; ++a) {
        w.operand[a] = (pair_ops >> a) & 1u;
        w.rows[a] = w.operand[a] == 0 ? (f.planes ? Pass2Rows::pair0_xf : Pass2Rows::pair0) : (f.planes ? Pass2Rows::narrow_xf : Pass2Rows::narrow);
        w.spills[a] = 1;  // unless a later accumulator takes the same operand
        for (int b = a + 1; b < na; ++b)
          if (((pair_ops >> b) & 1u) == w.operand[a]) w.spills[a] = 0;
        w.snap[a] = a == na - 1;
      }
      break;
    case 'N':
      if (na != 1 || kw != 1) return w;
      one("narrow", kNarrowBytes[blk], Pass2Rows::narrow);
      break;
    default:  // 'F'
      if (na == 1 && f.stream && n_words == 2) one("stream_wide", kStreamWideBytes[blk], Pass2Rows::wide);
      else one(na == 1 ? "flat_one" : "flat_any", kFlatBytes[blk][na - 1], Pass2Rows::wide), w.lean = false;
      break;
  }
  return w;
}

static const char* name_of(Pass2Form f) { return f == Pass2Form::refused ? "refused" : kPass2FormName[(int)f]; }

static bool same(const Pass2Choice& c, const Want& w) {
  if (strcmp(name_of(c.form), w.form) != 0) return false;
  if (c.form == Pass2Form::refused) return true;
  if (c.lds_bytes != w.lds || c.n_launches != w.n) return false;
  for (int a = 0; a < w.n; ++a) {
    const Pass2Launch& l = c.launch[a];
    if (w.lean && l.rows != w.rows[a]) return false;
    if (l.operand != w.operand[a] || l.plane_spills != w.spills[a] || l.keeps_snap != w.snap[a]) return false;
  }
  return true;
}

int main() {
  // ---- the list ----
  const int kPass2Forms = (int)(sizeof(kPass2FormName) / sizeof(kPass2FormName[0]));
  CHECK(kPass2Forms == 8 && (int)Pass2Form::pair_planes == 7 && (int)Pass2Form::refused < 0);
  for (int i = 0; i < kPass2Forms; ++i)
    for (int j = 0; j < i; ++j) CHECK(strcmp(kPass2FormName[i], kPass2FormName[j]) != 0);
  CHECK(strcmp(kPass2FormName[(int)Pass2Form::flat_one], "flat_one") == 0 && strcmp(kPass2FormName[(int)Pass2Form::pair_planes], "pair_planes") == 0);

  // ---- choose_pass2 ----
  long cells = 0;
  int seen[8] = {};
  for (int fi = 0; fi < 32; ++fi) {
    const FlagRow& f = kFlagRows[fi];
    // (the flags pass 2 does not look at must not matter: set on every other row)
    const uint32_t flags = (f.narrow ? PTF_NARROW : 0u) | (f.shared ? PTF_SHARED : 0u) | (f.planes ? PTF_PLANES : 0u) | (f.pair ? PTF_PAIR : 0u) |
                           (f.stream ? PTF_STREAM_PASS2 : 0u) | ((fi & 1) ? (PTF_CHUNK16 | PTF_WS | PTF_KEY4 | PTF_RESUME | PTF_HOT) : 0u);
    for (int na = 1; na <= 8; ++na)
      for (int kw = 1; kw <= 2; ++kw)
        for (uint32_t n_words = 2; n_words <= 3; ++n_words)
          for (int blk = 0; blk < 2; ++blk)
            for (int line = 0; line < 2; ++line) {
              const uint32_t n_ops = f.branch == 'R' ? 1u << na : 2u;  // (the other forms: the pattern must not matter)
              for (uint32_t pair_ops = 0; pair_ops < n_ops; ++pair_ops) {
                const Want w = expected(f, na, kw, n_words, blk, pair_ops, line != 0);
                const Pass2Choice c = choose_pass2(flags, na, kw, n_words, blk ? 8192u : 4096u, 256u, pair_ops, line != 0);
                if (!same(c, w)) {
                  printf("FAILED choose_pass2(flags 0x%x, na %d, kw %d, n_words %u, slots %d, pair_ops 0x%x, line %d) = %s, %zu bytes, %d launches; expected %s, %zu, %d\n",
                         flags, na, kw, n_words, blk ? 8192 : 4096, pair_ops, line, name_of(c.form), c.lds_bytes, c.n_launches, w.form, w.lds, w.n);
                  ++failures;
                }
                if (c.form != Pass2Form::refused) ++seen[(int)c.form];
                ++cells;
              }
            }
  }
  for (int i = 0; i < kPass2Forms; ++i) CHECK(seen[i] > 0);  // every form is reached

  // ---- cells by hand, end to end ----
  {  // AVG-like pair: accumulator 0 on operand 0, accumulator 1 on operand 1
    const Pass2Choice c = choose_pass2(PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_PAIR, 2, 1, 3, 8192, 256, 0x2, true);
    CHECK(c.form == Pass2Form::pair && c.lds_bytes == 122880 && c.n_launches == 2);
    CHECK(c.launch[0].rows == Pass2Rows::pair0 && c.launch[0].operand == 0 && c.launch[0].plane_spills == 1 && !c.launch[0].keeps_snap);
    CHECK(c.launch[1].rows == Pass2Rows::narrow && c.launch[1].operand == 1 && c.launch[1].plane_spills == 1 && c.launch[1].keeps_snap);
  }
  {  // three aggregates, operands 0, 1, 1: the second launch leaves the spilling to the third
    const Pass2Choice c = choose_pass2(PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_PAIR | PTF_PLANES, 3, 1, 3, 8192, 256, 0x6, true);
    CHECK(c.form == Pass2Form::pair_planes && c.lds_bytes == 122880 && c.n_launches == 3);
    CHECK(c.launch[0].rows == Pass2Rows::pair0_xf && c.launch[0].operand == 0 && c.launch[0].plane_spills == 1 && !c.launch[0].keeps_snap);
    CHECK(c.launch[1].rows == Pass2Rows::narrow_xf && c.launch[1].operand == 1 && c.launch[1].plane_spills == 0 && !c.launch[1].keeps_snap);
    CHECK(c.launch[2].rows == Pass2Rows::narrow_xf && c.launch[2].operand == 1 && c.launch[2].plane_spills == 1 && c.launch[2].keeps_snap);
  }
  // the producers: 1024 at the most, whatever the form; the flat kernels' prefix array grows with them
  CHECK(choose_pass2(0, 1, 1, 2, 4096, 1024, 0, true).form == Pass2Form::flat_one);
  CHECK(choose_pass2(0, 1, 1, 2, 4096, 1024, 0, true).lds_bytes == 4096 * 16 + 1025 * 4 + 16);
  CHECK(choose_pass2(0, 1, 1, 2, 4096, 1025, 0, true).form == Pass2Form::refused);
  CHECK(choose_pass2(PTF_NARROW | PTF_PAIR, 2, 1, 3, 8192, 1025, 0x2, true).form == Pass2Form::refused);
  // the oddity that stays: PTF_PLANES alone takes a narrow launch past the flat kernels' check (it passes at this size anyway)
  CHECK(choose_pass2(PTF_NARROW | PTF_PLANES, 1, 1, 2, 8192, 256, 0, true).form == Pass2Form::narrow);
  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("ok: %d forms, %ld cells of choose_pass2\n", kPass2Forms, cells);
  return 0;
}
