// dfx_k_base_inl.hpp -- the device-side helpers every kernel translation unit may use: vector typedefs, bit casts, the shadow
// conversions, the group hashes, canonical loads / typed stores, Rust's numeric casts, the wave shuffles.  Everything here is
// __device__ __forceinline__ (or __host__ __device__ inline), so each .hip translation unit gets its own copy and they compile in
// parallel; nothing here is emitted unless a kernel uses it.
// Who includes it: every kernel unit, directly (the text, sort, dictionary, Utf8 and Parquet kernels need nothing else) or through
// dfx_k_acc_inl.hpp (accumulators, group table) and dfx_k_interp_inl.hpp (the expression interpreter, under the row-source policies).
#pragma once
#include <hip/hip_runtime.h>

#include "dfx_kernels.hpp"

namespace dfx {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef uint64_t u64x4 __attribute__((ext_vector_type(4)));
typedef uint64_t u64x16 __attribute__((ext_vector_type(16)));
typedef uint64_t u64x8 __attribute__((ext_vector_type(8)));

#define DEV __device__ __forceinline__
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---------------------------------------------------------------------------------------------
// scalar helpers
// ---------------------------------------------------------------------------------------------
DEV double as_f64(uint64_t x) { return __longlong_as_double((long long)x); }
DEV uint64_t f64_bits(double x) { return (uint64_t)__double_as_longlong(x); }
DEV float as_f32(uint64_t x) { return __uint_as_float((uint32_t)x); }
DEV uint64_t f32_bits(float x) { return (uint64_t)__float_as_uint(x); }
// The Float32 shadow of a Float64 column (dfx_value_shadow.hpp).  shadow_widen is THE conversion from a shadow word back to the
// column's value: the build kernel accepts an element only if this very function returns its bits, and the scanners call nothing
// else.  shadow_narrow: the word stored for v, and whether v is refused -- other bits after widening, any NaN (a NaN's payload can
// survive the round trip; none is accepted), or a Float32 denormal (zero exponent field, non-zero mantissa: whether v_cvt_f64_f32
// flushes it is a mode of the wave, so no accepted value ever asks).  +-0, +-infinity and normal floats widen exactly in every mode.
DEV uint64_t shadow_widen(uint32_t w) { return f64_bits((double)__uint_as_float(w)); }
DEV uint32_t shadow_narrow(uint64_t v, bool* refused) {
  const uint32_t w = __float_as_uint((float)as_f64(v));
  const bool nan = (v & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
  const bool denormal = (w & 0x7F800000u) == 0u && (w & 0x007FFFFFu) != 0u;
  *refused = shadow_widen(w) != v || nan || denormal;
  return w;
}
DEV bool get_bit(const uint8_t* bm, int64_t i) { return (bm[i >> 3] >> (i & 7)) & 1; }
DEV int lane_id() { return (int)(threadIdx.x & 63); }

__host__ __device__ inline uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Group-key hash.  Every scanned (or routed) row pays for it, and 64-bit multiplies are ~8 quarter-rate
// VALU ops each on CDNA, so the hash is built from three 32-bit multiplies per key word (murmur3-style
// two-block mix + fmix32 finaliser; ~2.5x cheaper than a splitmix64 finaliser).  The 32 hash bits are
// returned in the HIGH half: table slot = h >> (64 - log2 capacity), capacity <= 2^31.
__host__ __device__ inline uint32_t hash_word(uint64_t k, uint32_t seed) {
  uint32_t x = ((uint32_t)k ^ seed) * 0xCC9E2D51u;
  x ^= x >> 15;
  x ^= (uint32_t)(k >> 32);
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  return x ^ (x >> 16);
}
// hash_word restricted to keys below 2^32 is a bijection of the low word (odd multiplies and xor-shifts, the high
// word's xor is zero): its inverse, for the seed hash_keys<1> uses.  Multiplicative inverses modulo 2^32.
constexpr uint32_t kHashSeed0 = 0x9E3779B9u;
__host__ __device__ inline uint32_t unhash_word32(uint32_t h) {
  uint32_t x = h;
  x ^= x >> 16;
  x *= 0x7ED1B41Du;  // 0xC2B2AE35^-1
  x ^= x >> 13;
  x ^= x >> 26;
  x *= 0xA5CB9243u;  // 0x85EBCA6B^-1
  x ^= x >> 15;
  x ^= x >> 30;
  x *= 0xDEE13BB1u;  // 0xCC9E2D51^-1
  return x ^ kHashSeed0;
}
template <int KW>
__host__ __device__ inline uint64_t hash_keys(const uint64_t* key) {
  uint32_t h = hash_word(key[0], kHashSeed0);
#pragma unroll
  for (int w = 1; w < KW; ++w) h = hash_word(key[w], h);
  return (uint64_t)h << 32;
}
// owner rank of a group in the multi-GPU exchange: bits independent of the slot index
__host__ __device__ inline uint32_t hash_rank(uint64_t h, uint32_t world) {
  uint32_t x = (uint32_t)(h >> 32) ^ 0x5BD1E995u;
  x *= 0x2C1B3C6Du;
  x ^= x >> 15;
  x *= 0x297A2D39u;
  x ^= x >> 16;
  return x % world;
}

DEV bool is_signed_int(uint8_t t) { return t >= T_I8 && t <= T_I64; }
DEV bool is_int(uint8_t t) { return t >= T_I8 && t <= T_U64; }

// canonical 64-bit image of a value of dtype t: signed ints sign-extended, unsigned zero-extended,
// f32 as its bit pattern in the low dword, f64 as its bit pattern, Boolean 0/1
DEV uint64_t wrap_to(uint8_t t, uint64_t x) {
  switch (t) {
    case T_I8: return (uint64_t)(int64_t)(int8_t)x;
    case T_I16: return (uint64_t)(int64_t)(int16_t)x;
    case T_I32: return (uint64_t)(int64_t)(int32_t)x;
    case T_U8: return (uint64_t)(uint8_t)x;
    case T_U16: return (uint64_t)(uint16_t)x;
    case T_U32: return (uint64_t)(uint32_t)x;
    default: return x;
  }
}

DEV uint64_t load_canonical(uint8_t t, const void* base, int64_t row, int64_t bit_offset) {
  switch (t) {
    case T_F64: case T_I64: case T_U64: return ((const uint64_t*)base)[row];
    case T_I32: return (uint64_t)(int64_t)((const int32_t*)base)[row];
    case T_U32: case T_F32: return (uint64_t)((const uint32_t*)base)[row];
    case T_I16: return (uint64_t)(int64_t)((const int16_t*)base)[row];
    case T_U16: return (uint64_t)((const uint16_t*)base)[row];
    case T_I8: return (uint64_t)(int64_t)((const int8_t*)base)[row];
    case T_U8: return (uint64_t)((const uint8_t*)base)[row];
    case T_BOOL: return (uint64_t)get_bit((const uint8_t*)base, bit_offset + row);
    default: return 0;
  }
}

DEV void store_typed(uint8_t t, void* base, int64_t row, uint64_t v) {
  switch (t) {
    case T_F64: case T_I64: case T_U64: ((uint64_t*)base)[row] = v; break;
    case T_I32: case T_U32: case T_F32: ((uint32_t*)base)[row] = (uint32_t)v; break;
    case T_I16: case T_U16: ((uint16_t*)base)[row] = (uint16_t)v; break;
    case T_I8: case T_U8: ((uint8_t*)base)[row] = (uint8_t)v; break;
    default: break;
  }
}

// Rust `as` numeric casts (float -> int saturating, NaN -> 0); same table as oracle cast_val
DEV int64_t sat_to_i64(double x, int64_t lo, int64_t hi) {
  if (x != x) return 0;
  if (x <= (double)lo) return lo;
  if (x >= (double)hi) return hi;
  return (int64_t)x;
}
DEV uint64_t sat_to_u64(double x, uint64_t hi) {
  if (x != x) return 0;
  if (x <= 0.0) return 0;
  if (x >= (double)hi) return hi;
  return (uint64_t)x;
}

DEV uint64_t cast_value(uint8_t from, uint8_t to, uint64_t v) {
  if (from == to) return v;
  if (is_int(from)) {
    if (is_int(to)) return wrap_to(to, v);
    if (to == T_F64) return f64_bits(is_signed_int(from) ? (double)(int64_t)v : (double)v);
    return f32_bits(is_signed_int(from) ? (float)(int64_t)v : (float)v);
  }
  const double x = (from == T_F32) ? (double)as_f32(v) : as_f64(v);
  switch (to) {
    case T_F32: return (from == T_F32) ? v : f32_bits((float)as_f64(v));
    case T_F64: return f64_bits(x);
    case T_I8: return (uint64_t)sat_to_i64(x, -128, 127);
    case T_I16: return (uint64_t)sat_to_i64(x, -32768, 32767);
    case T_I32: return (uint64_t)sat_to_i64(x, -2147483648ll, 2147483647ll);
    case T_I64: return (uint64_t)sat_to_i64(x, (int64_t)0x8000000000000000ull, 0x7FFFFFFFFFFFFFFFll);
    case T_U8: return sat_to_u64(x, 255ull);
    case T_U16: return sat_to_u64(x, 65535ull);
    case T_U32: return sat_to_u64(x, 4294967295ull);
    case T_U64: return sat_to_u64(x, 0xFFFFFFFFFFFFFFFFull);
    default: return 0;
  }
}

DEV uint64_t shfl_xor_u64(uint64_t v, int m) { return (uint64_t)__shfl_xor((unsigned long long)v, m, 64); }
DEV uint64_t wave_inclusive_scan(uint64_t v) {  // (the scans of dfx_k_core.hip and k_compact of dfx_k_filter.hip)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = __shfl_up(v, d, 64);
    if (lane_id() >= d) v += o;
  }
  return v;
}

}  // namespace dfx
