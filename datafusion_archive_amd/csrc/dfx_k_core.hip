// dfx_k_core.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the projection / aggregate path: scans, projection, the
// reduce fold, fills and shadows, finalisation, synthetic columns, the per-KW table entry points.  (The filter operator's
// kernels: dfx_k_filter.hip; profiler and grid sizing: dfx_launch.cpp.)
// Memory-bound integer/f64 work: no MFMA.  Design rules used throughout:
//   * one wave owns 64 consecutive rows at a time, so every global access is a fully coalesced
//     512-byte (8 B/lane) request and `__ballot` of a per-row predicate IS the Arrow LSB-first
//     bitmap word of those rows;
//   * expression intermediates live in VGPR register files indexed by wave-uniform indices
//     (s_set_gpr_idx), never in memory; literals come from the kernarg segment by scalar load;
//   * all inter-workgroup state (group table, counters) is touched only with agent-scope atomics:
//     per-XCD L2s are not coherent, atomics are (MI355X_MICROARCH.md, inter-workgroup visibility);
//   * grids are sized to a few resident workgroups per CU on 256 CUs and stride over tiles.
// Compile with -ffp-contract=off (the reference never fuses a*b+c) and -munsafe-fp-atomics
// (hardware global_atomic_add_f64 / ds_add_f64 instead of CAS loops).
#include "dfx_kernels.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "dfx_k_acc_inl.hpp"
#include "dfx_k_policy_inl.hpp"
#include "dfx_launch.hpp"

namespace dfx {

uint32_t host_unhash_word32(uint32_t image) { return unhash_word32(image); }
uint64_t host_hash_keys(const uint64_t* key, int kw) {
  switch (kw) {
    case 1: return hash_keys<1>(key);
    case 2: return hash_keys<2>(key);
    case 3: return hash_keys<3>(key);
    case 4: return hash_keys<4>(key);
    default: return hash_keys<8>(key);
  }
}

// ---------------------------------------------------------------------------------------------
// exclusive scans (tile counts -> offsets; string lengths -> offsets)
// ---------------------------------------------------------------------------------------------
// (kScanChunk elements per block, scan_blocks(n) blocks: dfx_scan_rules.hpp)

// block-wide exclusive scan of one value per thread; returns the exclusive prefix, *total = block sum
DEV uint64_t block_exclusive_scan(uint64_t v, uint64_t* total, uint64_t* lds4) {
  const uint64_t inc = wave_inclusive_scan(v);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 63) lds4[wave] = inc;
  __syncthreads();
  uint64_t base = 0;
  for (int w = 0; w < wave; ++w) base += lds4[w];
  *total = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  __syncthreads();
  return base + inc - v;
}

template <typename TIN>
__global__ __launch_bounds__(kBlock) void k_scan_local(const TIN* __restrict__ in, int64_t n,
                                                       uint64_t* __restrict__ block_sums) {
  __shared__ uint64_t lds4[4];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * 16;
  uint64_t sum = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (base + i < n) sum += (uint64_t)in[base + i];
  uint64_t total;
  block_exclusive_scan(sum, &total, lds4);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_scan_sums(uint64_t* __restrict__ block_sums, int64_t nb) {
  // single block: exclusive scan of block_sums in place; block_sums[nb] = grand total
  __shared__ uint64_t lds4[4];
  uint64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += kBlock) {
    const int64_t i = b0 + threadIdx.x;
    const uint64_t v = i < nb ? block_sums[i] : 0;
    uint64_t total;
    const uint64_t ex = block_exclusive_scan(v, &total, lds4);
    if (i < nb) block_sums[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) block_sums[nb] = carry;
}

template <typename TIN, typename TOUT>
__global__ __launch_bounds__(kBlock) void k_scan_apply(const TIN* __restrict__ in, int64_t n,
                                                       const uint64_t* __restrict__ block_sums,
                                                       int64_t nb, TOUT* __restrict__ out) {
  __shared__ uint64_t lds4[4];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * 16;
  uint64_t v[16];
  uint64_t sum = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    v[i] = (base + i < n) ? (uint64_t)in[base + i] : 0;
    sum += v[i];
  }
  uint64_t total;
  uint64_t run = block_sums[blockIdx.x] + block_exclusive_scan(sum, &total, lds4);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (base + i < n) out[base + i] = (TOUT)run;
    run += v[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = (TOUT)block_sums[nb];
}
__global__ __launch_bounds__(kBlock) void k_utf8_lengths(const int32_t* __restrict__ offsets, int64_t n,
                                                         int32_t* __restrict__ lengths,
                                                         int32_t* __restrict__ starts) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int32_t a = offsets[i], b = offsets[i + 1];
    lengths[i] = b - a;
    starts[i] = a;
  }
}

__global__ __launch_bounds__(kBlock) void k_utf8_gather(const uint8_t* __restrict__ data,
                                                        const int32_t* __restrict__ src_starts,
                                                        const int32_t* __restrict__ dst_offsets,
                                                        int64_t m, uint8_t* __restrict__ out) {
  // one 16-lane group per output string: lanes stride over the bytes
  const int64_t gid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 4;
  const int sub = threadIdx.x & 15;
  const int64_t stride = ((int64_t)gridDim.x * kBlock) >> 4;
  for (int64_t i = gid; i < m; i += stride) {
    const int32_t s = src_starts[i], d = dst_offsets[i], len = dst_offsets[i + 1] - d;
    for (int32_t b = sub; b < len; b += 16) out[d + b] = data[s + b];
  }
}

// ---------------------------------------------------------------------------------------------
// K2/K3 project
// ---------------------------------------------------------------------------------------------
template <typename POL>
__global__ __launch_bounds__(kBlock) void k_project(const DevProgram P, const DevColumns C,
                                                    const DevProjectPlan plan, const int64_t n,
                                                    uint32_t* __restrict__ ctrl) {
  typedef typename POL::COLV COLV;
  constexpr int U = POL::U;
  const int lane = lane_id();
  const int64_t n_words = (n + 63) >> 6;
  const int64_t wave_global = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
  DevFastPlan F_unused;
  F_unused.valid = 0;
  uint32_t err = 0;
  for (int64_t w0 = wave_global * U; w0 < n_words; w0 += n_waves * U) {
    COLV col[U];
    uint32_t cv[U];
    FOR_U {
      const int64_t row = (w0 + u) * 64 + lane;
      POL::load(P, C, row, row < n, col[u], cv[u]);
    }
#pragma nounroll
    for (int uu = 0; uu < U; ++uu) {
      const int64_t w = w0 + uu;
      if (w >= n_words) break;  // wave-uniform
      COLV cur;
      uint32_t curv;
      DFX_SELECT_BANK(uu, col, cv, cur, curv)
      const int64_t row = w * 64 + lane;
      const bool inb = row < n;
      u64x16 reg;
      uint32_t rv = 0;
      POL::eval(P, F_unused, cur, curv, reg, rv, inb, err);
#pragma unroll
      for (int o = 0; o < kMaxOut; ++o) {
        if (o < plan.n_out) {
          uint64_t v;
          bool valid;
          fetch(P, cur, reg, curv, rv, plan.out[o], v, valid);
          const uint8_t t = plan.out_dtype[o];
          if (t == T_BOOL) {
            const uint64_t bits = __ballot(inb && (v & 1));
            if (lane == 0) ((uint64_t*)plan.out_values[o])[w] = bits;
          } else if (inb) {
            store_typed(t, plan.out_values[o], row, v);
          }
          if (plan.out_validity[o] != nullptr) {
            const uint64_t vb = __ballot(inb && valid);
            if (lane == 0) plan.out_validity[o][w] = vb;
          }
        }
      }
    }
  }
  if (err) atomicOr(&ctrl[CTRL_ERROR], err);
}

// AccumulatorSet::accumulate_scalar for the batch scalars (aggregate.rs:107-145/:176-214/:245-283),
// executed by one thread; then re-arms the batch partials with their identities.
// func: 0 min, 1 max, 2 sum, 3 count.  state[2a] = has, state[2a+1] = value bits (canonical).
__global__ void k_reduce_fold(const DevTable T, const uint8_t* __restrict__ arg_dtype,
                              const uint8_t* __restrict__ func, uint64_t* __restrict__ partial,
                              uint64_t* __restrict__ state, uint32_t* __restrict__ ctrl) {
  // one wave: lane = copy of the batch partial (kReduceSlots == 64).  Combine the copies per aggregate with a
  // shuffle tree (all three words are associative and commutative), re-arm them; lane a then folds aggregate a.
  static_assert(kReduceSlots == 64, "one lane per partial copy");
  const int lane = threadIdx.x;
  uint64_t* mine = partial + (size_t)lane * kReduceSlotWords;
  uint64_t passed = mine[3];
  mine[3] = 0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) passed += shfl_xor_u64(passed, m);
  if (lane == 0 && passed && T.stats) atomicAdd((unsigned long long*)&T.stats[STAT_PASSED], (unsigned long long)passed);
  (void)ctrl;
  uint64_t accw = 0, cnt = 0, first = ~0ull;
  for (int a = 0; a < T.na; ++a) {
    uint64_t x = mine[4 * a + 0], c = mine[4 * a + 1], f1 = mine[4 * a + 2];
    mine[4 * a + 0] = T.acc_init[a];
    mine[4 * a + 1] = 0;
    mine[4 * a + 2] = ~0ull;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const uint64_t ox = shfl_xor_u64(x, m), oc = shfl_xor_u64(c, m), of = shfl_xor_u64(f1, m);
      if (oc) x = c ? acc_combine(T.acc_kind[a], x, ox) : ox;  // copies without valid rows hold the identity
      c += oc;
      f1 = of < f1 ? of : f1;
    }
    if (lane == a) {
      accw = x;
      cnt = c;
      first = f1;
    }
  }
  const int a = lane;
  if (a >= T.na) return;
  const uint8_t t = arg_dtype[a], f = func[a];
  bool has = cnt != 0;
  uint64_t val = accw;
  if (f == 3) {
    has = true;  // deviation D3: COUNT of a batch is always Some(n)
  } else if (has && (t == T_F64 || t == T_F32) && f != 2) {
    double d = (first & 1) ? __longlong_as_double(0x7FF8000000000000ll) : f64_from_ordered(accw);
    val = (t == T_F64) ? f64_bits(d) : f32_bits((float)d);
  } else if (has && f == 2 && is_int(t)) {
    val = wrap_to(t, accw);
  }
  if (!has) return;  // Option::None: accumulator unchanged (or stays None)
  if (!state[2 * a]) {
    state[2 * a] = 1;
    state[2 * a + 1] = val;
    return;
  }
  const uint64_t cur = state[2 * a + 1];
  uint64_t out;
  if (f == 3) {
    out = cur + val;
  } else if (t == T_F64) {
    const double x = as_f64(cur), y = as_f64(val);
    out = f64_bits(f == 0 ? fmin(x, y) : f == 1 ? fmax(x, y) : x + y);
  } else if (t == T_F32) {
    const float x = as_f32(cur), y = as_f32(val);
    out = f32_bits(f == 0 ? fminf(x, y) : f == 1 ? fmaxf(x, y) : x + y);
  } else if (is_signed_int(t)) {
    const int64_t x = (int64_t)cur, y = (int64_t)val;
    out = f == 0 ? (uint64_t)(x < y ? x : y) : f == 1 ? (uint64_t)(x > y ? x : y) : wrap_to(t, cur + val);
  } else {
    out = f == 0 ? (cur < val ? cur : val) : f == 1 ? (cur > val ? cur : val) : wrap_to(t, cur + val);
  }
  state[2 * a + 1] = out;
}

__global__ __launch_bounds__(kBlock) void k_fill_u64(uint64_t* __restrict__ p, uint64_t v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) p[i] = v;
}
// The Int32 shadow of an Int64 key column (dfx_key_shadow.hpp): 8 bytes read, 4 written per row -- a lane takes two keys (one
// 16-byte load, one 8-byte store); the upper halves it drops are ORed into one word: non-zero = some key has no 32-bit form.
__global__ __launch_bounds__(kBlock) void k_narrow_keys(const uint64_t* __restrict__ in, int64_t n, uint32_t* __restrict__ out, uint32_t* __restrict__ dropped) {
  typedef uint64_t u64x2v __attribute__((ext_vector_type(2)));
  typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
  uint32_t hi = 0;
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kBlock) {
    const u64x2v k = __builtin_nontemporal_load((const u64x2v*)in + i);
    hi |= (uint32_t)(k.x >> 32) | (uint32_t)(k.y >> 32);
    u32x2v w;
    w.x = (uint32_t)k.x;
    w.y = (uint32_t)k.y;
    ((u32x2v*)out)[i] = w;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t k = in[n - 1];
    hi |= (uint32_t)(k >> 32);
    out[n - 1] = (uint32_t)k;
  }
  if (hi != 0) atomicOr(dropped, hi);
}
// The Float32 shadow of a Float64 operand column (dfx_value_shadow.hpp), the same stream: two values per lane, the float of each
// stored, "some value is not exactly its float" (shadow_narrow: THE rule, next to the scanners' shadow_widen) ORed into one word.
__global__ __launch_bounds__(kBlock) void k_narrow_values(const uint64_t* __restrict__ in, int64_t n, uint32_t* __restrict__ out, uint32_t* __restrict__ inexact) {
  typedef uint64_t u64x2v __attribute__((ext_vector_type(2)));
  typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
  bool bad = false;
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kBlock) {
    const u64x2v v = __builtin_nontemporal_load((const u64x2v*)in + i);
    bool r0, r1;
    u32x2v w;
    w.x = shadow_narrow(v.x, &r0);
    w.y = shadow_narrow(v.y, &r1);
    bad = bad || r0 || r1;
    ((u32x2v*)out)[i] = w;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    bool r;
    out[n - 1] = shadow_narrow(in[n - 1], &r);
    bad = bad || r;
  }
  if (bad) atomicOr(inexact, 1u);
}
__global__ __launch_bounds__(kBlock) void k_fill_u32(uint32_t* __restrict__ p, uint32_t v, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) p[i] = v;
}

// dense u64 plane -> typed output column (keys: narrow; aggregates: undo the accumulator image)
__global__ __launch_bounds__(kBlock) void k_finalize(const uint64_t* __restrict__ in, int64_t n,
                                                     uint8_t out_dtype, uint8_t val_xform,
                                                     void* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    uint64_t v = in[i];
    if (val_xform == VT_F64_ORD_MIN || val_xform == VT_F64_ORD_MAX) {
      v = f64_bits(f64_from_ordered(v));
    } else if (val_xform == VT_F32_ORD_MIN || val_xform == VT_F32_ORD_MAX) {
      v = f32_bits((float)f64_from_ordered(v));
    }
    store_typed(out_dtype, out, i, v);
  }
}

// AVG = SUM / COUNT of the same argument (deviation D7: the reference's planner types AVG, its executor has none).
// sum: the SUM accumulator word, cnt: the COUNT word; result in the argument's type: IEEE division for floats,
// truncating division of the wrapped sum for integers; null when cnt == 0.  validity: Arrow bitmap words.
__host__ __device__ inline uint64_t avg_value(uint8_t t, uint64_t sum, uint64_t cnt) {
  union { uint64_t u; double d; } c64;
  union { uint32_t u; float f; } c32;
  if (t == T_F64) {
    c64.u = sum;
    c64.d = c64.d / (double)cnt;
    return c64.u;
  }
  if (t == T_F32) {
    c32.u = (uint32_t)sum;
    c32.f = c32.f / (float)cnt;
    return (uint64_t)c32.u;
  }
  // integers: the wrapped sum in the argument's width, truncating division
  int bits = 64;
  bool is_signed = false;
  switch (t) {
    case T_I8: bits = 8; is_signed = true; break;
    case T_I16: bits = 16; is_signed = true; break;
    case T_I32: bits = 32; is_signed = true; break;
    case T_I64: bits = 64; is_signed = true; break;
    case T_U8: bits = 8; break;
    case T_U16: bits = 16; break;
    case T_U32: bits = 32; break;
    default: break;
  }
  if (is_signed) {
    const int64_t x = bits == 64 ? (int64_t)sum : (int64_t)(sum << (64 - bits)) >> (64 - bits);
    return (uint64_t)(x / (int64_t)cnt);
  }
  const uint64_t x = bits == 64 ? sum : sum & ((1ull << bits) - 1ull);
  return x / cnt;
}
uint64_t host_avg_value(uint8_t t, uint64_t sum, uint64_t cnt) { return avg_value(t, sum, cnt); }

__global__ __launch_bounds__(kBlock) void k_finalize_avg(const uint64_t* __restrict__ sum, const uint64_t* __restrict__ cnt,
                                                         int64_t n, uint8_t out_dtype, void* __restrict__ out,
                                                         uint64_t* __restrict__ validity, uint64_t* __restrict__ null_count) {
  const int64_t n_pad = (n + 63) & ~63ll;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_pad; i += (int64_t)gridDim.x * kBlock) {
    const bool inb = i < n;
    const uint64_t c = inb ? cnt[i] : 0;
    const bool valid = inb && c != 0;
    if (inb) store_typed(out_dtype, out, i, valid ? avg_value(out_dtype, sum[i], c) : 0ull);
    const uint64_t vm = __ballot(valid), im = __ballot(inb);
    if (lane_id() == 0) {
      validity[i >> 6] = vm;
      const int nulls = __popcll(im & ~vm);
      if (nulls) atomicAdd((unsigned long long*)null_count, (unsigned long long)nulls);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// synthetic columns -- same definition as orc_synth_fill (oracle/dfx_oracle.c)
// ---------------------------------------------------------------------------------------------
DEV uint64_t synth_u64(uint64_t seed, int column_id, int64_t row) {
  const uint64_t s = seed ^ ((uint64_t)(uint32_t)column_id * 0xA0761D6478BD642Full);
  return mix64(s + ((uint64_t)row + 1ull) * 0x9E3779B97F4A7C15ull);
}

__global__ __launch_bounds__(kBlock) void k_synth(int kind, int column_id, double p0, double p1, uint64_t seed,
                                                  int64_t row_begin, int64_t n, void* __restrict__ out) {
  int zipf_bits = 0;
  const uint64_t G = (uint64_t)(int64_t)p0;
  const int exact_shift = 64 - (p0 > 0.0 ? (int)p0 : 20);
  const double exact_scale = __longlong_as_double((long long)(1023 - (p1 > 0.0 ? (int)p1 : 10)) << 52);  // 2^-S
  if (kind == 3) {
    while ((1ull << zipf_bits) < G && zipf_bits < 62) ++zipf_bits;
  }
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint64_t r = synth_u64(seed, column_id, row_begin + i);
    if (kind == 0) {
      const double u = (double)(r >> 11) * 0x1.0p-53;
      const double t = p1 * u;
      ((double*)out)[i] = p0 + t;
    } else if (kind == 1) {  // m * 2^-S, m below 2^B (B = p0 or 20, S = p1 or 10): exact products / sums within the bit budget
      ((double*)out)[i] = (double)(r >> exact_shift) * exact_scale;
    } else if (kind == 2) {
      ((int64_t*)out)[i] = (int64_t)__umul64hi(r, G);
    } else if (kind == 4) {
      ((int32_t*)out)[i] = (int32_t)__umul64hi(r, G);
    } else if (kind == 5) {  // DFX_SYNTH_I64_WIDE
      ((int64_t*)out)[i] = (int64_t)((__umul64hi(r, G) + 1ull) * 0x9E3779B97F4A7C15ull);
    } else {
      const uint64_t b = __umul64hi(r, (uint64_t)zipf_bits + 1ull);
      const uint64_t r2 = mix64(r ^ 0xD6E8FEB86659FD93ull);
      uint64_t k = (b == 0) ? 0 : ((1ull << (b - 1)) + __umul64hi(r2, 1ull << (b - 1)));
      if (k >= G) k = G - 1;
      ((int64_t*)out)[i] = (int64_t)k;
    }
  }
}

// validity bitmap of a synthetic column: row NULL with probability permille / 1000 (include/dfx.h: DFX_SYNTH_NULL_PERMILLE;
// same draw as orc_synth_validity).  One ballot word per 64 rows; nulls += the number of null rows.
__global__ __launch_bounds__(kBlock) void k_synth_validity(int column_id, uint32_t permille, uint64_t seed, int64_t row_begin,
                                                           int64_t n, uint64_t* __restrict__ words, unsigned long long* nulls) {
  const int64_t n_words = (n + 63) >> 6;
  const int lane = lane_id();
  unsigned long long mine = 0;
  for (int64_t w = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; w < n_words; w += ((int64_t)gridDim.x * kBlock) >> 6) {
    const int64_t i = w * 64 + lane;
    const bool inb = i < n;
    const bool valid = inb && __umul64hi(synth_u64(seed, column_id ^ kSynthNullStream, row_begin + i), 1000ull) >= (uint64_t)permille;
    const uint64_t m = __ballot(valid);
    if (lane == 0) {
      words[w] = m;
      const int64_t rows = n - w * 64 < 64 ? n - w * 64 : 64;
      mine += (unsigned long long)(rows - __popcll(m));
    }
  }
  if (lane == 0 && mine) atomicAdd(nulls, mine);
}

template <typename TIN, typename TOUT>
static hipError_t scan_impl(const TIN* in, TOUT* out, int64_t n, uint64_t* tmp, hipStream_t s) {
  Scope sc(KID_SCAN, s, 0);
  const int64_t nb = scan_blocks(n);  // tmp[nb]: the 64-bit grand total
  hipLaunchKernelGGL((k_scan_local<TIN>), dim3((unsigned)nb), dim3(kBlock), 0, s, in, n, tmp);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kBlock), 0, s, tmp, nb);
  hipLaunchKernelGGL((k_scan_apply<TIN, TOUT>), dim3((unsigned)nb), dim3(kBlock), 0, s, in, n, tmp, nb, out);
  return hipGetLastError();
}
hipError_t launch_scan_u32(const uint32_t* in, uint64_t* out, int64_t n, uint64_t* tmp, hipStream_t s) {
  return scan_impl<uint32_t, uint64_t>(in, out, n, tmp, s);
}
hipError_t launch_scan_i32(const int32_t* in, int32_t* out, int64_t n, uint64_t* tmp, hipStream_t s) {
  return scan_impl<int32_t, int32_t>(in, out, n, tmp, s);
}

hipError_t launch_utf8_lengths(const int32_t* offsets, int64_t n, int32_t* lengths, int32_t* starts, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_GATHER_UTF8, s, 0);
  const int grid = stream_grid((n + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_utf8_lengths, dim3(grid), dim3(kBlock), 0, s, offsets, n, lengths, starts);
  return hipGetLastError();
}
hipError_t launch_utf8_gather(const uint8_t* data, const int32_t* src_starts, const int32_t* dst_offsets,
                              int64_t m, uint8_t* out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  Scope sc(KID_GATHER_UTF8, s, 0);
  const int grid = stream_grid((m * 16 + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_utf8_gather, dim3(grid), dim3(kBlock), 0, s, data, src_starts, dst_offsets, m, out);
  return hipGetLastError();
}

hipError_t launch_project(const DevProgram& P, const DevColumns& C, const DevProjectPlan& plan, int64_t n,
                          uint32_t* ctrl, double algo_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_PROJECT, s, algo_bytes);
  const int grid = stream_grid((n + kBlock - 1) / kBlock, 8);
  auto run = [&](auto pol) {
    hipLaunchKernelGGL((k_project<typename decltype(pol)::type>), dim3(grid), dim3(kBlock), 0, s, P, C, plan, n, ctrl);
    return hipGetLastError();
  };
  const DevFastPlan no_fast = {};  // (a projection has no decoded shape)
  switch (choose_row_source(ScanKernel::project, P, no_fast, 0, 0, nullptr, nullptr, false, 0)) {
    case RowSource::interp_c2: return run(Policy<InterpPolicy<2, 8>>{});
    case RowSource::interp_c4: return run(Policy<InterpPolicy<4, 4>>{});
    case RowSource::interp_c8: return run(Policy<InterpPolicy<8, 2>>{});
    default: return hipErrorNotSupported;  // (no other source in this kernel's ladder)
  }
}

hipError_t launch_reduce_fold(const DevTable& T, const uint8_t* arg_dtype, const uint8_t* func,
                              uint64_t* partial, uint64_t* state, uint32_t* ctrl, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_fold, dim3(1), dim3(64), 0, s, T, arg_dtype, func, partial, state, ctrl);
  return hipGetLastError();
}


DFX_DECLARE_TABLE_KW(1)
DFX_DECLARE_TABLE_KW(2)
DFX_DECLARE_TABLE_KW(3)
DFX_DECLARE_TABLE_KW(4)
DFX_DECLARE_TABLE_KW(8)

#define DFX_KW_DISPATCH(kw, CALL)            \
  switch (kw) {                              \
    case 1: return CALL(1);                  \
    case 2: return CALL(2);                  \
    case 3: return CALL(3);                  \
    case 4: return CALL(4);                  \
    case 8: return CALL(8);                  \
    default: return hipErrorInvalidValue;    \
  }

hipError_t launch_hash_agg(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevAggPlan& plan,
                           const DevTable& T, const DevRows& spill, int64_t n, double algo_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_HASH_AGG, s, algo_bytes);
#define CALL(K) table_hash_agg<K>(P, fast, C, plan, T, spill, n, s)
  DFX_KW_DISPATCH(T.kw, CALL)
#undef CALL
}

hipError_t launch_merge_rows(const DevRows& rows, int64_t row_begin, int64_t n_rows, const DevTable& T,
                             const DevRows& spill, hipStream_t s) {
  if (n_rows <= 0) return hipSuccess;
  Scope sc(KID_MERGE_ROWS, s, 0);
#define CALL(K) table_merge_rows<K>(rows, row_begin, n_rows, T, spill, s)
  DFX_KW_DISPATCH(T.kw, CALL)
#undef CALL
}

hipError_t launch_merge_bucket(const uint64_t* bucket, uint64_t count, const DevTable& T, const DevRows& spill,
                               hipStream_t s) {
  DevRows rows;
  rows.words = const_cast<uint64_t*>(bucket);
  rows.capacity = count;
  return launch_merge_rows(rows, 0, (int64_t)count, T, spill, s);
}

hipError_t launch_rehash(const DevTable& from, const DevTable& to, const DevRows& spill, hipStream_t s) {
  Scope sc(KID_REHASH, s, 0);
#define CALL(K) table_rehash<K>(from, to, spill, s)
  DFX_KW_DISPATCH(from.kw, CALL)
#undef CALL
}

hipError_t launch_table_mask(const DevTable& T, uint64_t* mask_words, uint32_t* tile_counts, hipStream_t s) {
  Scope sc(KID_EMIT_MASK, s, 0);
#define CALL(K) table_mask<K>(T, mask_words, tile_counts, s)
  DFX_KW_DISPATCH(T.kw, CALL)
#undef CALL
}

hipError_t launch_partial_count(const DevTable& T, int world, uint64_t* counts, hipStream_t s) {
  Scope sc(KID_PARTIAL, s, 0);
#define CALL(K) table_partial_count<K>(T, world, counts, s)
  DFX_KW_DISPATCH(T.kw, CALL)
#undef CALL
}

hipError_t launch_partial_scatter(const DevTable& T, int world, const uint64_t* bucket_base,
                                  const uint64_t* bucket_count, uint64_t* cursors, uint64_t* dst, hipStream_t s) {
  Scope sc(KID_PARTIAL, s, 0);
#define CALL(K) table_partial_scatter<K>(T, world, bucket_base, bucket_count, cursors, dst, s)
  DFX_KW_DISPATCH(T.kw, CALL)
#undef CALL
}

// Result download by the shader: 16-byte loads from HBM, 16-byte stores to host-mapped pinned memory (the destination
// is hipHostMalloc'd, device-accessible).  The copy engines' path showed sporadic 6 - 150 ms stalls on these boxes for an
// 8 MB device-to-host copy (tools/d2h_probe.py: 1 in 300 with torch's own copy, too); a kernel on the query's stream has
// no such outliers and needs no engine hand-over.  `bytes` any value; src / dst 16-byte aligned (pool allocations are).
__global__ __launch_bounds__(256) void k_copy_to_host(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n16,
                                                      const uint8_t* __restrict__ src_tail, uint8_t* __restrict__ dst_tail, int tail) {
  // four 16-byte pieces per lane in flight (the PCIe writes are posted; the loads are what a lane waits for)
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const uint4 a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
    dst[i] = a;
    dst[i + stride] = b;
    dst[i + 2 * stride] = c;
    dst[i + 3 * stride] = d;
  }
  for (; i < n16; i += stride) dst[i] = src[i];
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}
hipError_t launch_copy_to_host(const void* src_device, void* dst_pinned, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  if ((((uintptr_t)src_device) | ((uintptr_t)dst_pinned)) & 15u) return hipMemcpyAsync(dst_pinned, src_device, bytes, hipMemcpyDeviceToHost, s);
  const int64_t n16 = (int64_t)(bytes / 16);
  const int tail = (int)(bytes % 16);
  const int grid = (int)std::min<int64_t>(512, std::max<int64_t>(1, (n16 + 1023) / 1024));
  hipLaunchKernelGGL(k_copy_to_host, dim3(grid), dim3(256), 0, s, (const uint4*)src_device, (uint4*)dst_pinned, n16,
                     (const uint8_t*)src_device + n16 * 16, (uint8_t*)dst_pinned + n16 * 16, tail);
  return hipGetLastError();
}

hipError_t launch_fill_u64(uint64_t* p, uint64_t v, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_FILL, s, 0);
  hipLaunchKernelGGL(k_fill_u64, dim3(stream_grid((n + kBlock - 1) / kBlock, 8)), dim3(kBlock), 0, s, p, v, n);
  return hipGetLastError();
}
hipError_t launch_narrow_keys(const uint64_t* in, int64_t n, uint32_t* out, uint32_t* dropped, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_FILL, s, 12.0 * (double)n);
  hipLaunchKernelGGL(k_narrow_keys, dim3(stream_grid((n / 2 + kBlock) / kBlock, 8)), dim3(kBlock), 0, s, in, n, out, dropped);
  return hipGetLastError();
}
hipError_t launch_narrow_values(const uint64_t* in, int64_t n, uint32_t* out, uint32_t* inexact, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_FILL, s, 12.0 * (double)n);
  hipLaunchKernelGGL(k_narrow_values, dim3(stream_grid((n / 2 + kBlock) / kBlock, 8)), dim3(kBlock), 0, s, in, n, out, inexact);
  return hipGetLastError();
}
hipError_t launch_fill_u32(uint32_t* p, uint32_t v, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_FILL, s, 0);
  hipLaunchKernelGGL(k_fill_u32, dim3(stream_grid((n + kBlock - 1) / kBlock, 8)), dim3(kBlock), 0, s, p, v, n);
  return hipGetLastError();
}

hipError_t launch_finalize(const uint64_t* in, int64_t n, uint8_t out_dtype, uint8_t val_xform, void* out,
                           hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_FINALIZE, s, 0);
  hipLaunchKernelGGL(k_finalize, dim3(stream_grid((n + kBlock - 1) / kBlock, 8)), dim3(kBlock), 0, s, in, n, out_dtype, val_xform, out);
  return hipGetLastError();
}

hipError_t launch_finalize_avg(const uint64_t* sum, const uint64_t* cnt, int64_t n, uint8_t out_dtype, void* out,
                               uint64_t* validity, uint64_t* null_count, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_FINALIZE, s, 0);
  hipLaunchKernelGGL(k_finalize_avg, dim3(stream_grid((n + kBlock - 1) / kBlock, 8)), dim3(kBlock), 0, s, sum, cnt, n, out_dtype, out,
                     validity, null_count);
  return hipGetLastError();
}

hipError_t launch_synth_validity(int column_id, uint32_t permille, uint64_t seed, int64_t row_begin, int64_t n, uint64_t* words,
                                 uint64_t* nulls, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_SYNTH, s, 0);
  hipLaunchKernelGGL(k_synth_validity, dim3(stream_grid((n + kBlock - 1) / kBlock, 16)), dim3(kBlock), 0, s, column_id, permille, seed, row_begin, n,
                     words, (unsigned long long*)nulls);
  return hipGetLastError();
}

hipError_t launch_synth(int kind, int column_id, double p0, double p1, uint64_t seed, int64_t row_begin, int64_t n,
                        void* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_SYNTH, s, 0);
  hipLaunchKernelGGL(k_synth, dim3(stream_grid((n + kBlock - 1) / kBlock, 16)), dim3(kBlock), 0, s, kind, column_id, p0, p1, seed, row_begin, n, out);
  return hipGetLastError();
}

}  // namespace dfx
