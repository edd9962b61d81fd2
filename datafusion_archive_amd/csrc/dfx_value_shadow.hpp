// dfx_value_shadow.hpp -- the Float32 shadow of a resident Float64 operand column: when it is built, when
// it is refused, and the memory rule.  Host only and free of HIP, like dfx_key_shadow.hpp, whose rule this IS: the same state
// machine per column (the option -1 / 0 / 1, the second qualifying query, the memory rule, one lock per table held across the
// build, slices on multiples of 64 rows, 64 bytes of padding, silent drops, refusal for good), run by a KeyShadows of its own.
// Only the meaning of the device call differs: it stores (float)v per element and returns a non-zero word when some element is
// not EXACTLY that float -- the bits of (double)(float)v differ from v's (a 25-bit mantissa, a value out of range), v is a NaN, or
// (float)v is a Float32 denormal (the scanners' widening must not depend on the denormal mode of the conversion instructions).
// +-0, +-infinity and every normal Float32 value are accepted.  A scan that reads an accepted column from its 4-byte copy and
// widens it gets every bit of every value back: no result can change.
// tests/native/value_shadow_rule.cpp runs the rule with the device stubbed, under the host sanitizers.
#pragma once
#include "dfx_key_shadow.hpp"

namespace dfx {

// free_bytes, alloc: as for the key shadow.  narrow(src, rows, dst, inexact): rows Float64 values from src as Float32 into dst on
// the query's stream; *inexact != 0: some element has no exact Float32 form.  false: the device refused (the column stays eligible)
typedef KeyShadowDevice ValueShadowDevice;
constexpr size_t kValueShadowPad = kKeyShadowPad;  // bytes behind the last element: the scanners' pair loads read one element past an odd row count

class ValueShadows {
 public:
  // a null-free Float64 column of the table being made (before any scan can ask)
  void add_column(const void* values, int64_t rows) { rule_.add_column(values, rows); }
  // The Float32 words of the operand rows that start at `values` (a slice of a registered column), or null.  option:
  // agg.value_shadow; first_ask, query_bytes, built: KeyShadows::acquire.
  const uint32_t* acquire(const void* values, int option, bool first_ask, size_t query_bytes, const ValueShadowDevice& dev, bool* built) {
    return rule_.acquire(values, option, first_ask, query_bytes, dev, built);
  }
  const uint32_t* peek(const void* values) const { return rule_.peek(values); }  // the words if the copy exists; no side effects
  const void* column_of(const void* values, int64_t* rows, int64_t* row) const { return rule_.column_of(values, rows, row); }
  size_t bytes_held() const { return rule_.bytes_held(); }
  // (tests) -1 unknown, 0 nothing built, 1 built, 2 refused (not Float32-exact); *queries: askers so far
  int state_of(const void* values, int* queries = nullptr) const { return rule_.state_of(values, queries); }

 private:
  KeyShadows rule_;
};

}  // namespace dfx
