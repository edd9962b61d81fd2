// dfx_k_parquet_write_inl.hpp -- what the two kernel units of the Parquet writer (dfx_k_parquet_write.hip: PLAIN pages;
// dfx_k_parquet_write_dict.hip: the "dictionary" option) share on the device: a lane's row of a tile, the wave reductions, and the
// ORing of bits into aligned words of a zeroed buffer.
#pragma once
#include "dfx_k_base_inl.hpp"
#include "dfx_parquet_write.hpp"

namespace dfx {
namespace {

using namespace pqw;

constexpr int kPqwBlock = 256;
typedef uint32_t pqw_u32 __attribute__((aligned(1)));  // values sit at any byte of a body
typedef uint64_t pqw_u64 __attribute__((aligned(1)));

DEV uint64_t pqw_wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += shfl_xor_u64(v, d);
  return v;
}
DEV uint64_t pqw_wave_or(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v |= shfl_xor_u64(v, d);
  return v;
}

struct PqwRow {  // one lane's row of a tile
  bool valid;
  int64_t begin;  // Utf8: the value's bytes, clamped
  uint32_t len;
};
// the lane's row: validity from the bitmap at its bit offset (all ones without one); a Utf8 value's extent clamped into [lo, hi)
DEV PqwRow pqw_row(const DevPqwCol& col, int64_t row, bool in, int64_t rows) {
  PqwRow r;
  r.valid = in && (col.validity == nullptr || get_bit(col.validity, col.bit_offset + row));
  r.begin = 0;
  r.len = 0;
  if (col.dtype == T_UTF8 && r.valid) {
    const int64_t lo = (int64_t)col.offsets[0], hi = (int64_t)col.offsets[rows];
    int64_t b = (int64_t)col.offsets[row], e = (int64_t)col.offsets[row + 1];
    b = b < lo ? lo : b > hi ? hi : b;
    e = e < b ? b : e > hi ? hi : e;
    r.begin = b;
    r.len = (uint32_t)(e - b);
  }
  return r;
}

// ORs the 64 bits of v into the buffer from absolute bit `bit` on: lanes 0..2 take one aligned word each, a word without a bit is skipped
DEV void pqw_or_bits(uint32_t* out32, uint64_t bit, uint64_t v, int lane) {
  if (lane > 2) return;
  const uint32_t sh = (uint32_t)(bit & 31u);
  const uint32_t w0 = (uint32_t)(v << sh);
  const uint32_t w1 = (uint32_t)(sh ? v >> (32u - sh) : v >> 32);
  const uint32_t w2 = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
  const uint32_t w = lane == 0 ? w0 : lane == 1 ? w1 : w2;
  if (w) __hip_atomic_fetch_or(out32 + (bit >> 5) + (uint64_t)lane, w, RLX_AGENT);
}

}  // namespace
}  // namespace dfx
