// dfx_k_distinct_inl.hpp -- COUNT(DISTINCT x) (deviation D8): the distinct-set kernels, templated on the tuple width KW.
// Instantiated once per KW in dfx_k_distinct{1,2,3,4,8}.hip so the variants build in parallel.
//
// A distinct set is a DevTable with na == 0 whose key is the TUPLE (group key words, zero padding, canonical argument image):
// width 1 ungrouped, kw_out + 1 grouped (five to seven keys padded to eight words, like the GROUP BY tables).  The insert, the
// spill list, the growth (k_rehash) and the spill replay (k_merge_rows) are the group table's own helpers; what is new here is
// the evaluation of the tuple, the skipping of null arguments, the float canonicalisation and the two emit kernels.
#pragma once
#include "dfx_k_acc_inl.hpp"
#include "dfx_k_plan_policy_inl.hpp"
#include "dfx_k_policy_inl.hpp"
#include "dfx_launch.hpp"

namespace dfx {

// one value per distinct float: -0.0 is +0.0, every NaN payload is the quiet NaN; integers as load_canonical reads them
DEV uint64_t distinct_image(uint8_t t, uint64_t v) {
  if (t == T_F64) {
    if ((v & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0x7FF8000000000000ull;
    return v == 0x8000000000000000ull ? 0ull : v;
  }
  if (t == T_F32) {
    const uint32_t x = (uint32_t)v;
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC00000ull;
    return x == 0x80000000u ? 0ull : (uint64_t)x;
  }
  return wrap_to(t, v);  // (narrow integers: the same image whichever loader widened them)
}

// Rows -> tuples -> set.  plan.key[0, kw_out) are the group keys, plan.arg[0] the argument (plan.arg_dtype[0] its type).
// A row whose argument is null is skipped.  The probe reads a slot with a plain load and CASes only an empty one
// (table_upsert_slot): once the set is warm most rows are duplicates and cost one load.  (A wave-level dedup -- a lane whose
// tuple equals its lower neighbour's leaving the insert to that lane -- lost tuples on the device and was taken out: DESIGN.md.)  Rows the set cannot take (past its
// load limit, probe sequence exhausted) go to the spill list, which the host sizes for the whole batch.
template <int KW, typename POL>
__global__ __launch_bounds__(kBlock) void k_distinct_insert(const DevProgram P, const DevFastPlan F, const DevColumns C,
                                                            const DevAggPlan plan, const int kw_out, const DevTable T,
                                                            const DevRows spill, const int64_t n) {
  typedef typename POL::COLV COLV;
  constexpr int U = POL::U;
  const int lane = lane_id();
  const int64_t n_words = (n + 63) >> 6;
  const int64_t wave_global = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
  uint32_t err = 0;
  int iter = 0;
  bool saturated = false;
  const uint64_t none[kMaxAggs] = {0, 0, 0, 0, 0, 0, 0, 0};
  typename POL::PREP prep;
  POL::prepare(P, F, prep);
  for (int64_t w0 = wave_global * U; w0 < n_words; w0 += n_waves * U, ++iter) {
    if ((iter & 7) == 0) {  // wave-uniform: has the set passed its load limit?
      saturated = __hip_atomic_load(&T.ctrl[CTRL_SATURATED], RLX_AGENT) != 0u;
      if (!saturated && (uint64_t)__hip_atomic_load(&T.ctrl[CTRL_OCCUPIED], RLX_AGENT) > T.load_limit) {
        saturated = true;
        if (lane == 0) __hip_atomic_store(&T.ctrl[CTRL_SATURATED], 1u, RLX_AGENT);
      }
    }
    COLV col[U];
    uint32_t cv[U];
    FOR_U {
      const int64_t row = (w0 + u) * 64 + lane;
      POL::load(P, C, row, row < n, col[u], cv[u]);
    }
#pragma nounroll
    for (int uu = 0; uu < U; ++uu) {
      COLV cur;
      uint32_t curv;
      DFX_SELECT_BANK(uu, col, cv, cur, curv)
      const int64_t row = (w0 + uu) * 64 + lane;
      const bool inb = row < n;
      u64x16 reg;
      uint32_t rv = 0;
      POL::eval(P, F, cur, curv, reg, rv, inb, err, prep);
      uint64_t tup[KW];
#pragma unroll
      for (int k = 0; k < KW - 1; ++k)  // key nulls are not checked (aggregate.rs:807-852), as in the GROUP BY
        tup[k] = k < kw_out ? wrap_to(plan.key_dtype[k], POL::key(P, F, plan.key[k], k, cur, curv, reg, rv)) : 0ull;
      uint64_t v;
      bool valid;
      POL::arg(P, F, plan.arg[0], 0, cur, curv, reg, rv, v, valid);
      tup[KW - 1] = distinct_image(plan.arg_dtype[0], v);
      bool todo = inb && valid;
      if (todo && !saturated) {
        if (table_apply<KW>(T, tup, none)) todo = false;
      }
      spill_row<KW>(T, spill, todo, tup, none);
    }
  }
  if (err) atomicOr(&T.ctrl[CTRL_ERROR], err);
}

template <int KW>
DEV bool distinct_slot_occupied(const DevTable& S, uint64_t slot) {
  if (slot == S.mask + 1) return KW == 1 && S.ctrl[CTRL_SENTINEL] != 0u;
  if (KW == 1) return S.keys[slot] != kEmptyKey;
  return S.state[slot] == 2u;
}

// One pass over the set's slots.  Ungrouped (KW == 1): wave-reduced count into total[0].  Grouped: +1 per tuple into the count
// table Cnt (same width, the argument word zeroed: the key prefix; one ACC_ADD_U64 accumulator).  Cnt is sized so that it never
// fills (load <= 1/2, probing over the whole table); an insert that fails anyway sets bit 8 of its CTRL_ERROR.
template <int KW>
__global__ __launch_bounds__(kBlock) void k_distinct_count(const DevTable S, const DevTable Cnt, uint64_t* total) {
  const int64_t n_slots = (int64_t)S.mask + 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t n_pad = (n_slots + 63) & ~63ll;
  uint64_t cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_pad; i += stride) {
    const bool occ = i < n_slots && distinct_slot_occupied<KW>(S, (uint64_t)i);
    if (KW == 1) {
      cnt += occ ? 1 : 0;
    } else if (occ) {
      uint64_t key[KW];
      const uint64_t one[kMaxAggs] = {1, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < KW - 1; ++k) key[k] = S.keys[(uint64_t)k * S.stride + i];
      key[KW - 1] = 0;
      if (!table_apply<KW>(Cnt, key, one)) atomicOr(&Cnt.ctrl[CTRL_ERROR], 0x100u);
    }
  }
  if (KW == 1) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += shfl_xor_u64(cnt, m);
    if (lane_id() == 0 && cnt) atomicAdd((unsigned long long*)total, (unsigned long long)cnt);
  }
}


// The emit-time tables (the count table here, the extrema table of dfx_k_utf8agg.hip) are keyed by the key prefix: row i of the
// emitted key columns as such a key, and its slot (table_upsert_slot's probe sequence).  The table is complete and quiescent:
// plain loads.  KW > 1: the emit-time table of a grouped query is at least two words wide.
template <int KW>
DEV void distinct_prefix_key(const DevDistinctKeys& K, int kw_out, int64_t i, uint64_t (&key)[KW]) {
#pragma unroll
  for (int k = 0; k < KW; ++k) key[k] = k < kw_out ? load_canonical(K.dtype[k], K.values[k], i, 0) : 0ull;
}
template <int KW>
DEV bool distinct_prefix_find(const DevTable& Cnt, const uint64_t (&key)[KW], uint64_t& slot_out) {
  uint64_t slot = ((hash_keys<KW>(key) >> Cnt.shift) & Cnt.mask) & ~3ull;
  for (int p = 0; p < Cnt.max_probe; ++p) {
    const uint32_t st = Cnt.state[slot];
    if (st == 0u) return false;
    bool eq = true;
#pragma unroll
    for (int k = 0; k < KW; ++k) eq = eq && Cnt.keys[(uint64_t)k * Cnt.stride + slot] == key[k];
    if (eq) {
      slot_out = slot;
      return true;
    }
    slot = (slot & ~(uint64_t)Cnt.block_mask) | ((slot + 1) & (uint64_t)Cnt.block_mask);
  }
  return false;
}

// emitted group keys -> their distinct counts (0: the group has no counted tuple)
template <int KW>
__global__ __launch_bounds__(kBlock) void k_distinct_lookup(const DevTable Cnt, const DevDistinctKeys K, const int kw_out,
                                                            const int64_t n, uint64_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    uint64_t key[KW];
    distinct_prefix_key<KW>(K, kw_out, i, key);
    uint64_t c = 0, slot = 0;
    if (KW > 1 && distinct_prefix_find<KW>(Cnt, key, slot)) c = Cnt.accs[slot];
    out[i] = c;
  }
}

// ---------------------------------------------------------------------------------------------
// host launchers (one instantiation per KW)
// ---------------------------------------------------------------------------------------------
template <int KW>
hipError_t distinct_insert(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevAggPlan& plan, int kw_out,
                           const DevTable& T, const DevRows& spill, int64_t n, bool* plan_kernel, hipStream_t s) {
  const int grid = stream_grid((n + kBlock - 1) / kBlock, 8);
  // plain columns (nulls and 4-byte columns included): the scan plan's loads; anything else: the SSA interpreter
  const uint8_t xf[kMaxAggs] = {VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW};
  const BoundRowSource b = bind_row_source(ScanKernel::distinct_insert, P, fast, C, kw_out, 1, xf, xf);
  *plan_kernel = is_plan(b.source);
  auto run = [&](auto pol) {
    hipLaunchKernelGGL((k_distinct_insert<KW, typename decltype(pol)::type>), dim3(grid), dim3(kBlock), 0, s, P, b.F(fast), b.C(C), plan, kw_out, T, spill, n);
    return hipGetLastError();
  };
  switch (b.source) {
    case RowSource::plan_c2: return run(Policy<PlanPolicyN<2, 4, kPlanW4 | kPlanNulls>>{});
    case RowSource::plan_c4: return run(Policy<PlanPolicyN<4, 2, kPlanW4 | kPlanNulls>>{});
    case RowSource::interp_c4: return run(Policy<InterpPolicy<4, 4>>{});
    case RowSource::interp_c8: return run(Policy<InterpPolicy<8, 2>>{});
    default: return hipErrorNotSupported;  // (no other source in this kernel's ladder)
  }
}

template <int KW>
hipError_t distinct_count(const DevTable& S, const DevTable& Cnt, uint64_t* total, hipStream_t s) {
  const int64_t n = (int64_t)S.mask + 2;
  const int grid = stream_grid((n + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_distinct_count<KW>, dim3(grid), dim3(kBlock), 0, s, S, Cnt, total);
  return hipGetLastError();
}

template <int KW>
hipError_t distinct_lookup(const DevTable& Cnt, const DevDistinctKeys& K, int kw_out, int64_t n, uint64_t* out, hipStream_t s) {
  const int grid = stream_grid((n + kBlock - 1) / kBlock, 8);
  hipLaunchKernelGGL(k_distinct_lookup<KW>, dim3(grid), dim3(kBlock), 0, s, Cnt, K, kw_out, n, out);
  return hipGetLastError();
}

#define DFX_INSTANTIATE_DISTINCT_KW(KW)                                                                                      \
  template hipError_t distinct_insert<KW>(const DevProgram&, const DevFastPlan&, const DevColumns&, const DevAggPlan&, int,   \
                                          const DevTable&, const DevRows&, int64_t, bool*, hipStream_t);                      \
  template hipError_t distinct_count<KW>(const DevTable&, const DevTable&, uint64_t*, hipStream_t);                           \
  template hipError_t distinct_lookup<KW>(const DevTable&, const DevDistinctKeys&, int, int64_t, uint64_t*, hipStream_t);

}  // namespace dfx
