// pass1_units_check.cpp -- the list of pass-1 units of the partitioned GROUP BY and the choice of the scan plan's unit
// (csrc/dfx_pass1_units.hpp) as a stand-alone program: plan_unit over every (column count, gen, pair, one_value, PTF_KEY4) against a
// table written out by hand from the dispatcher this function replaced, and the list itself -- distinct names, one launcher slot
// per unit in the enum's order.  tests/test_pass1_units.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <string.h>

#include "../../datafusion_archive_amd/csrc/dfx_pass1_units.hpp"

using namespace dfx;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// the launcher table as dfx_k_partition.hip builds it, with launchers that say which unit they are
#define X(name) \
  static int launch_pass1_##name() { return (int)Pass1Unit::name; }
DFX_PASS1_UNITS(X)
#undef X
typedef int (*Launch)();
#define X(name) launch_pass1_##name,
static const Launch kLaunch[] = {DFX_PASS1_UNITS(X)};
#undef X

struct Cell {
  int cls, genk;  // plan_c<cls>_g<genk>
};
// [gen][column class: <= 2, exactly 3, 4 columns]
static const Cell kExpected[8][3] = {
    {{2, 0}, {3, 0}, {4, 0}},  // gen 0
    {{2, 1}, {3, 1}, {4, 1}},  // 1
    {{2, 2}, {3, 2}, {4, 2}},  // 2
    {{2, 3}, {3, 3}, {4, 3}},  // 3
    {{2, 4}, {4, 4}, {4, 4}},  // 4
    {{2, 1}, {3, 1}, {4, 1}},  // 5
    {{2, 6}, {4, 6}, {4, 6}},  // 6
    {{2, 3}, {3, 3}, {4, 3}},  // 7
};

static const char* name_of(Pass1Unit u) { return u == Pass1Unit::none ? "none" : kPass1UnitName[(int)u]; }

int main() {
  // ---- the list ----
  CHECK(kPass1Units == 29);
  CHECK((int)(sizeof(kLaunch) / sizeof(kLaunch[0])) == kPass1Units);
  for (int i = 0; i < kPass1Units; ++i) {
    CHECK(kPass1UnitName[i] != nullptr && kPass1UnitName[i][0] != 0);
    CHECK(kLaunch[i] != nullptr && kLaunch[i]() == i);  // slot i launches unit i
    for (int j = 0; j < i; ++j) CHECK(strcmp(kPass1UnitName[i], kPass1UnitName[j]) != 0);
  }
  CHECK((int)Pass1Unit::none < 0);

  // ---- plan_unit ----
  int cells = 0;
  for (int n_cols = 1; n_cols <= 4; ++n_cols)
    for (uint32_t gen = 0; gen < 8; ++gen)
      for (int pair = 0; pair < 2; ++pair)
        for (int one_value = 0; one_value < 2; ++one_value)
          for (int key4 = 0; key4 < 2; ++key4) {
            char want[32];
            if (!one_value && !pair && (gen & 4)) {
              snprintf(want, sizeof want, "none");  // bit 2 without a fixed-slot binding or a pair scan
            } else if (key4 && gen != 4) {
              snprintf(want, sizeof want, "none");  // over a shadow only the key may be a 4-byte column, and no bitmaps
            } else if (pair && n_cols != 3 && n_cols != 4) {
              snprintf(want, sizeof want, "none");  // the pair kernels: key + two operands (+ one predicate column)
            } else if (pair && (gen & 4)) {
              snprintf(want, sizeof want, "pair_key4_c%d", n_cols);
            } else {
              const Cell& e = kExpected[gen][n_cols <= 2 ? 0 : n_cols == 3 ? 1 : 2];
              snprintf(want, sizeof want, "plan_c%d_g%d", e.cls, e.genk);
            }
            const Pass1Unit got = plan_unit(n_cols, gen, pair != 0, one_value != 0, key4 != 0);
            if (strcmp(name_of(got), want) != 0) {
              printf("FAILED plan_unit(n_cols %d, gen %u, pair %d, one_value %d, key4 %d) = %s, expected %s\n", n_cols, gen, pair, one_value,
                     key4, name_of(got), want);
              ++failures;
            }
            ++cells;
          }
  CHECK(cells == 4 * 8 * 2 * 2 * 2);
  // gen's bits above bit 2 are not the unit's business
  CHECK(plan_unit(2, 8 | 1, false, true, false) == Pass1Unit::plan_c2_g1);
  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("ok: %d units, %d cells of plan_unit\n", kPass1Units, cells);
  return 0;
}
