// dfx_pass1_units.hpp -- pass 1 of the partitioned GROUP BY: THE list of its kernel units, and which scan-plan unit a bound
// plan takes.  One unit = one translation unit dfx_k_partition_<name>.hip (they compile in parallel, about a minute each) that
// defines launch_pass1_<name>.  From this list come the enum, the printable names, the launcher declarations and the table from
// enum to launcher (dfx_k_partition.hip) and the build's source list (build.py reads the names out of the list).  A new pass-1
// flavour is one name here, its one-line file, and its place in select_pass1 (dfx_k_partition.hip).
// Host only and free of HIP: tests/native/pass1_units_check.cpp holds plan_unit against a table written out by hand.
#pragma once
#include <stdint.h>

namespace dfx {

// static_*: a compile-time signature (dfx_sigs.hpp).  fast_* / interp_*: the generic row sources, <= 2 / 4 / 8 columns (ring,
// sorted and direct kernels only).  plan_c<C>_g<G>: the scan plan (PlanPolicy) -- column class <= 2, exactly 3, <= 4 columns; G =
// the GENK the kernels are compiled for: bit 0 4-byte columns widened, bit 1 validity bitmaps, bit 2 (instead of bit 0) the
// key is the only 4-byte column (the multi-value flavours of the g4 / g6 units are never launched: bit 2 belongs to the one-key,
// one-value binding).  key4_*: the signature over the key column's Int32 shadow, two keys per lane (PTF_KEY4; the
// wave-specialised kernel alone; the same two units hold the kernels over both shadows, PTF_VAL4, and those that route 8-byte
// rows, PTF_ROW8).  pair_key4_*: the pair scan over a 4-byte key, 3 / 4 columns (the pair kernel alone; the pair
// scan over 8-byte keys is a flavour of plan_c3_* / plan_c4_* g0..g3).
#define DFX_PASS1_UNITS(X)                                                                   \
  X(static_key_sum_pred2) X(static_key_sum) X(static_key_aff_sum_pred2)                      \
  X(fast_c2) X(interp_c2) X(fast_c4) X(interp_c4) X(fast_c8) X(interp_c8)                    \
  X(plan_c2_g0) X(plan_c2_g1) X(plan_c2_g2) X(plan_c2_g3) X(plan_c2_g4) X(plan_c2_g6)        \
  X(plan_c3_g0) X(plan_c3_g1) X(plan_c3_g2) X(plan_c3_g3)                                    \
  X(plan_c4_g0) X(plan_c4_g1) X(plan_c4_g2) X(plan_c4_g3) X(plan_c4_g4) X(plan_c4_g6)        \
  X(key4_static_key_sum_pred2) X(key4_static_key_sum) X(pair_key4_c3) X(pair_key4_c4)

enum class Pass1Unit : int {
  none = -1,  // no unit takes the launch
#define X(name) name,
  DFX_PASS1_UNITS(X)
#undef X
};
#define X(name) +1
constexpr int kPass1Units = 0 DFX_PASS1_UNITS(X);
#undef X
#define X(name) #name,
constexpr const char* kPass1UnitName[kPass1Units] = {DFX_PASS1_UNITS(X)};
#undef X

// The scan-plan unit of a bound plan, or none.  n_cols, gen: DevScanPlan's, as bind_scan_plan left them; pair: PTF_PAIR (two
// operands per routed row: slot look-ups in the wave-specialised kernel); one_value: the flavours that find the key in slot 0 and
// the routed value in slot 1 (narrow rows, the wave-specialised kernel); key4: PTF_KEY4.
constexpr Pass1Unit plan_unit(int n_cols, uint32_t gen, bool pair, bool one_value, bool key4) {
  using U = Pass1Unit;
  // [column class][gen & 7]: bit 0 wins over bit 2, and three columns with a 4-byte key take the <= 4 column unit
  constexpr U by_gen[3][8] = {
      {U::plan_c2_g0, U::plan_c2_g1, U::plan_c2_g2, U::plan_c2_g3, U::plan_c2_g4, U::plan_c2_g1, U::plan_c2_g6, U::plan_c2_g3},
      {U::plan_c3_g0, U::plan_c3_g1, U::plan_c3_g2, U::plan_c3_g3, U::plan_c4_g4, U::plan_c3_g1, U::plan_c4_g6, U::plan_c3_g3},
      {U::plan_c4_g0, U::plan_c4_g1, U::plan_c4_g2, U::plan_c4_g3, U::plan_c4_g4, U::plan_c4_g1, U::plan_c4_g6, U::plan_c4_g3}};
  if (!one_value && !pair && (gen & 4)) return U::none;  // (cannot happen: bind_scan_plan gives bit 2 to fixed-slot bindings and to the pair scan over a shadow)
  // Over a shadow only the forms that load the key as a 4-byte word.  A second 4-byte slot -- COUNT(k) GROUP BY k binds the key
  // twice -- would take the generic 4-byte-column form (the aligned 8 bytes that hold the element, a lane select), which the pair
  // kernels ran at half the speed of the 8-byte key: such launches keep the 8-byte column.
  if (key4 && (gen & 7) != 4) return U::none;  // (pair scan: 10.2 ms against 5.5 ms of pass 1 per 10^9 rows)
  if (pair && n_cols != 3 && n_cols != 4) return U::none;  // (the pair kernels: key + two operand columns, and one more predicate column)
  if (pair && (gen & 4)) return n_cols == 3 ? U::pair_key4_c3 : U::pair_key4_c4;  // (one 4-byte load per lane)
  return by_gen[n_cols <= 2 ? 0 : n_cols == 3 ? 1 : 2][gen & 7];
}

}  // namespace dfx
