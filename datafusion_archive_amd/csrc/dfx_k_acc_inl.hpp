// dfx_k_acc_inl.hpp -- what an aggregate kernel does with a row once it has keys and values: the accumulator algebra (one 64-bit
// word per (group, aggregate): ordered float images, operand transforms, combine, hardware atomics) and the group table's
// find-or-insert with its spill list and statistics.
// Who includes it: the aggregate kernels -- dfx_k_core.hip, dfx_k_reduce.hip, dfx_k_fewgroup.hip, dfx_k_table_inl.hpp,
// dfx_k_distinct_inl.hpp, dfx_k_partition_inl.hpp (pass 1 and, through it, dfx_k_pass2.hip).
#pragma once
#include "dfx_k_base_inl.hpp"

namespace dfx {

// ---------------------------------------------------------------------------------------------
// accumulator algebra (one 64-bit word per (group, aggregate))
// ---------------------------------------------------------------------------------------------
// order-preserving u64 image of an f64; NaN is canonicalised so that MIN and MAX ignore it unless
// every value is NaN (f64::min / f64::max, aggregate.rs:136-141 / :205-210)
DEV uint64_t f64_ordered(double d, bool for_min) {
  uint64_t b = f64_bits(d);
  if (d != d) b = for_min ? 0x7FF8000000000000ull : 0xFFF8000000000000ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double f64_from_ordered(uint64_t u) {
  const uint64_t b = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
  union { uint64_t u; double d; } c;
  c.u = b;
  return c.d;
}

DEV uint64_t transform_value(uint8_t xf, uint64_t v, bool valid) {
  switch (xf) {
    case VT_F64_ORD_MIN: return f64_ordered(as_f64(v), true);
    case VT_F64_ORD_MAX: return f64_ordered(as_f64(v), false);
    case VT_F32_ORD_MIN: return f64_ordered((double)as_f32(v), true);
    case VT_F32_ORD_MAX: return f64_ordered((double)as_f32(v), false);
    case VT_COUNT_VALID: return valid ? 1ull : 0ull;
    default: return v;
  }
}

// non-atomic combine (thread-private / shuffle reductions)
DEV uint64_t acc_combine(uint8_t kind, uint64_t a, uint64_t b) {
  switch (kind) {
    case ACC_ADD_F64: return f64_bits(as_f64(a) + as_f64(b));
    case ACC_ADD_F32: return f32_bits(as_f32(a) + as_f32(b));
    case ACC_ADD_U64: return a + b;
    case ACC_MIN_S64: return (uint64_t)(((int64_t)a < (int64_t)b) ? (int64_t)a : (int64_t)b);
    case ACC_MAX_S64: return (uint64_t)(((int64_t)a > (int64_t)b) ? (int64_t)a : (int64_t)b);
    case ACC_MIN_U64: return a < b ? a : b;
    default: return a > b ? a : b;
  }
}

// one hardware atomic, result unused (no-return form); works on global and LDS addresses
DEV void acc_atomic(uint8_t kind, uint64_t* p, uint64_t v) {
  switch (kind) {
    case ACC_ADD_F64: unsafeAtomicAdd((double*)p, as_f64(v)); break;
    case ACC_ADD_F32: unsafeAtomicAdd((float*)p, as_f32(v)); break;
    case ACC_ADD_U64: atomicAdd((unsigned long long*)p, (unsigned long long)v); break;
    case ACC_MIN_S64: atomicMin((long long*)p, (long long)v); break;
    case ACC_MAX_S64: atomicMax((long long*)p, (long long)v); break;
    case ACC_MIN_U64: atomicMin((unsigned long long*)p, (unsigned long long)v); break;
    default: atomicMax((unsigned long long*)p, (unsigned long long)v); break;
  }
}

// ---------------------------------------------------------------------------------------------
// group table: find-or-insert + atomic update
// ---------------------------------------------------------------------------------------------
// returns false when the bounded probe sequence found neither the key nor a free slot
template <int KW>
DEV bool table_upsert_slot(const DevTable& T, const uint64_t (&key)[KW], uint64_t h, uint64_t& slot_out,
                           bool& inserted) {
  inserted = false;
  // The home slot is the base of the ALIGNED GROUP OF FOUR the hash points into (probing stays linear from there).
  // Pass 2 of the partitioned strategy examines a whole group per step (two 16-byte LDS reads) and a wave pays for its
  // slowest lane: with homes anywhere in the group a key often spills into the next group, with group-base homes a
  // 4-slot bucket at load <= 0.5 rarely overflows (measured: -10 % VALU, -6.5 % LDS instructions in pass 2).  The
  // global kernels pay ~1.5 more single-slot probes per lookup, which their atomic rate (24 G/s) hides.
  uint64_t slot = ((h >> T.shift) & T.mask) & ~3ull;
  if (KW == 1) {
    if (key[0] == kEmptyKey) {  // the one key that collides with the claim sentinel owns slot `cap`
      slot_out = T.mask + 1;
      if (__hip_atomic_load(&T.ctrl[CTRL_SENTINEL], RLX_AGENT) == 0u) {
        if (atomicExch(&T.ctrl[CTRL_SENTINEL], 1u) == 0u) inserted = true;
      }
      return true;
    }
    for (int p = 0; p < T.max_probe; ++p) {
      const uint64_t k = __hip_atomic_load(&T.keys[slot], RLX_AGENT);
      if (k == key[0]) {
        slot_out = slot;
        return true;
      }
      if (k == kEmptyKey) {
        const uint64_t old = atomicCAS((unsigned long long*)&T.keys[slot], (unsigned long long)kEmptyKey,
                                       (unsigned long long)key[0]);
        if (old == kEmptyKey) {
          inserted = true;
          slot_out = slot;
          return true;
        }
        if (old == key[0]) {
          slot_out = slot;
          return true;
        }
      }
      slot = (slot & ~(uint64_t)T.block_mask) | ((slot + 1) & (uint64_t)T.block_mask);
    }
    return false;
  } else {
    // multi-word keys: claim the slot's state word (0 empty -> 1 busy), publish the key words
    // write-through, drain, then state = 2.  A lane that meets a busy slot re-reads it on its next
    // loop trip (structured loop: the claimer never waits on anybody, so no SIMT deadlock).
    int spins = 0;
    for (int p = 0; p < T.max_probe;) {
      uint32_t st = __hip_atomic_load(&T.state[slot], RLX_AGENT);
      if (st == 0u) {
        const uint32_t old = atomicCAS(&T.state[slot], 0u, 1u);
        if (old == 0u) {
#pragma unroll
          for (int w = 0; w < KW; ++w) __hip_atomic_store(&T.keys[(uint64_t)w * T.stride + slot], key[w], RLX_AGENT);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(&T.state[slot], 2u, RLX_AGENT);
          inserted = true;
          slot_out = slot;
          return true;
        }
        st = old;
      }
      if (st == 1u) {
        if (++spins > (1 << 20)) return false;
        continue;
      }
      bool same = true;
#pragma unroll
      for (int w = 0; w < KW; ++w)
        same = same && (__hip_atomic_load(&T.keys[(uint64_t)w * T.stride + slot], RLX_AGENT) == key[w]);
      if (same) {
        slot_out = slot;
        return true;
      }
      slot = (slot & ~(uint64_t)T.block_mask) | ((slot + 1) & (uint64_t)T.block_mask);
      ++p;
    }
    return false;
  }
}

// append one row (keys + accumulator operands) to the spill list; wave-aggregated cursor bump
template <int KW>
DEV void spill_row(const DevTable& T, const DevRows& spill, bool do_spill, const uint64_t (&key)[KW],
                   const uint64_t (&val)[kMaxAggs]) {
  const uint64_t m = __ballot(do_spill);
  if (m == 0) return;
  const int lane = lane_id();
  const int leader = __ffsll((unsigned long long)m) - 1;
  uint64_t base = 0;
  if (lane == leader)
    base = atomicAdd((unsigned long long*)&T.ctrl[CTRL_SPILL_LO], (unsigned long long)__popcll(m));
  base = __shfl(base, leader, 64);
  if (do_spill) {
    const uint64_t pos = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < spill.capacity) {
#pragma unroll
      for (int w = 0; w < KW; ++w) spill.words[(uint64_t)w * spill.capacity + pos] = key[w];
#pragma unroll
      for (int a = 0; a < kMaxAggs; ++a)  // static indices: val[] must stay in registers
        if (a < T.na) spill.words[(uint64_t)(KW + a) * spill.capacity + pos] = val[a];
    }
  }
}

// statistics counter of this workgroup's stripe (see DevTable::stats)
DEV void stat_add(const DevTable& T, int which, uint64_t v) {
  if (T.stats && v) atomicAdd((unsigned long long*)&T.stats[(size_t)(blockIdx.x % kStatStripes) * STAT_WORDS + which], (unsigned long long)v);
}

// the group whose (single-word) key equals the claim sentinel lives in slot `cap`: the slice of table_apply<1>
// that such a row takes, as a small function of its own (the partition kernels call it from unrolled loops)
DEV void sentinel_apply(const DevTable& T, const uint64_t (&val)[kMaxAggs]) {
  bool inserted = false;
  if (__hip_atomic_load(&T.ctrl[CTRL_SENTINEL], RLX_AGENT) == 0u)
    inserted = atomicExch(&T.ctrl[CTRL_SENTINEL], 1u) == 0u;
  const uint64_t mi = __ballot(inserted);
  if (mi != 0 && lane_id() == __ffsll((unsigned long long)mi) - 1) atomicAdd(&T.ctrl[CTRL_OCCUPIED], (uint32_t)__popcll(mi));
  const uint64_t slot = T.mask + 1;
#pragma unroll
  for (int a = 0; a < kMaxAggs; ++a)
    if (a < T.na) acc_atomic(T.acc_kind[a], &T.accs[(uint64_t)a * T.stride + slot], val[a]);
}

template <int KW>
DEV bool table_apply(const DevTable& T, const uint64_t (&key)[KW], const uint64_t (&val)[kMaxAggs]) {
  uint64_t slot = 0;
  bool inserted = false;
  const bool ok = table_upsert_slot<KW>(T, key, hash_keys<KW>(key), slot, inserted);
  // new groups are counted ONCE PER WAVE: thousands of lanes bumping the same word serialise at
  // ~11 ns per atomic (MI355X_MICROARCH.md, fanin) -- 1 M inserts would cost 11 ms
  const uint64_t mi = __ballot(ok && inserted);
  if (mi != 0 && lane_id() == __ffsll((unsigned long long)mi) - 1) atomicAdd(&T.ctrl[CTRL_OCCUPIED], (uint32_t)__popcll(mi));
  if (!ok) return false;
#pragma unroll
  for (int a = 0; a < kMaxAggs; ++a)
    if (a < T.na) acc_atomic(T.acc_kind[a], &T.accs[(uint64_t)a * T.stride + slot], val[a]);
  return true;
}

}  // namespace dfx
