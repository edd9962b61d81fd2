// dfx_k_plan_policy_inl.hpp -- PlanPolicy: the row source that evaluates a scan plan (DevScanPlan, built on the host by
// dfx_scan_plan.hpp) as data, its plan words kept in vector registers.  It fills in the contract written down at the top of
// dfx_k_policy_inl.hpp.
// Who includes it: the scan kernels that take RowSource::plan_* or a plan unit of pass 1 -- dfx_k_reduce.hip, dfx_k_fewgroup.hip,
// dfx_k_table_inl.hpp, dfx_k_distinct_inl.hpp, dfx_k_partition_inl.hpp.
#pragma once
#include "dfx_k_policy_inl.hpp"

namespace dfx {

// ---------------------------------------------------------------------------------------------
// scan plan (DevScanPlan): the run-time shape family evaluated as DATA -- see dfx_device.hpp
// ---------------------------------------------------------------------------------------------
// A wave-uniform plan word in a VECTOR register.  Plan words read from the kernel arguments are scalar values, and a
// loop that keeps thirty of them alive runs out of scalar registers (the run-time decoded kernels carried 230-300 SGPR
// spills: a v_readlane per use); the vector file has room (128 registers per lane at sixteen waves per CU, the scan
// loops use ~60).  volatile: the copy stays where PlanPolicy::prepare puts it, before the scan loop (a pure asm was
// re-executed inside the loop, with its scalar sources alive across it: nothing gained).
DEV uint32_t plan_word(uint32_t s) {
  uint32_t v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
  return v;
}
DEV uint64_t plan_word64(uint64_t s) { return (uint64_t)plan_word((uint32_t)s) | ((uint64_t)plan_word((uint32_t)(s >> 32)) << 32); }

template <int NCOL, bool NULLS>
struct PlanBank {
  uint64_t v[NCOL];               // the aligned 8 bytes that hold the row's element of every plan column
  uint32_t vb[NULLS ? NCOL : 1];  // NULLS: validity bytes -- the row's own byte (per-row loads), or lane j = byte j of the TRIP's
                                  // bitmap slice (trip loads: one load per column and trip, every row group picks its byte
                                  // with ds_bpermute)
  DEV uint64_t operator[](int c) const { return v[c]; }
};

template <int NCOL>
DEV uint64_t plan_sel(const u64x16& reg, uint32_t slot) {  // slot is wave-uniform: compare-and-select, no indexing
  uint64_t x = reg[0];
  if (NCOL > 1) x = slot == 1u ? reg[1] : x;
  if (NCOL > 2) x = slot == 2u ? reg[2] : x;
  if (NCOL > 3) x = slot == 3u ? reg[3] : x;
  return x;
}

// NCOL: plan column slots loaded per row (slots past the plan's n_cols repeat slot 0: a cache hit, no branch around a load);
// GENK bit 0 (W4): 4-byte columns (read as the aligned 8 bytes that hold the element, widened afterwards), bit 1 (NULLS):
// validity bitmaps (without either every column is 8 bytes wide and null-free: no widening, no validity loads);
// FIXED: one key in slot 0, one routed argument in slot 1 (the partitioned GROUP BY's one-value kernels).
// bit 2 (KEY4: the FIXED kernels, and the pair scan's slot look-ups over a key shadow -- PlanPolicyN<3, 3, 4> / <4, 2, 4>, whose
// binding puts the key in slot 0): slot 0 -- the key -- is a 4-byte integer column and every other slot is 8 bytes wide: the
// key is read with a real 4-byte load (half the bytes of the aligned-pair form, no lane select) and extended in one operation.
// The reference's own GROUP BY fixtures have Int32 keys (aggregate.rs:1033-1127).
constexpr int kPlanW4 = 1, kPlanNulls = 2, kPlanKey4 = 4;
template <int NCOL, int U_, int GENK, bool FIXED>
struct PlanPolicy : PolicyDefaults<PlanPolicy<NCOL, U_, GENK, FIXED>, PlanBank<NCOL, (GENK & kPlanNulls) != 0>, U_> {
  static constexpr bool W4 = (GENK & kPlanW4) != 0, NULLS = (GENK & kPlanNulls) != 0, KEY4 = (GENK & kPlanKey4) != 0;
  static_assert(!(W4 && KEY4), "KEY4 is the special case of W4");
  static constexpr bool kHasTripLoad = true;
  static constexpr int U = U_;
  static constexpr int kStaticNa = FIXED ? 1 : 0;
  static_assert(!NULLS || U_ * 8 + 1 <= 64, "one lane per validity byte of a trip");
  typedef PlanBank<NCOL, NULLS> COLV;
  // The terms' plan words, one copy per lane (see plan_word): everything a term needs is a vector operand, the predicate is
  // evaluated without one scalar instruction besides the `t < np` guards.  Five registers per term: the range, and one word
  // of flags that v_bfe takes apart per use (a register per flag cost the ring kernels their 128-register budget):
  //   bit 0  image: negative values are complemented (f64)       bit 1  image: the sign bit is flipped (f64, i64)
  //   bit 2  complement the range test (NotEq, impossible terms) bit 3, 4  the term's column slot
  //   bit 5  the term's value for a null column value
  // ... and what the columns need, as per-LANE constants (the row groups of a trip start at multiples of 64 rows, so a lane's
  // half of an aligned pair, its validity bit and its byte of the trip's bitmap slice never change): widening and validity are
  // vector selects, no column word is decoded inside the loop.
  struct PREP {
    uint64_t nlo[kPlanTerms];   // -lo
    uint64_t span[kPlanTerms];
    uint32_t flags[kPlanTerms];
    uint32_t key_sext;                // KEY4: all ones: the key is a signed integer (sign-extended), else zero-extended
    uint32_t hi_half[W4 ? NCOL : 1];  // W4: all ones where this lane's 4-byte element is the HIGH word of its aligned pair
    uint32_t is4[W4 ? NCOL : 1];      //     all ones: a 4-byte column
    uint32_t sext[W4 ? NCOL : 1];     //     all ones: ... of signed integers
    uint32_t vshift[NULLS ? NCOL : 1];  // NULLS: (lane + bit_offset) & 7: the row's bit inside its validity byte
    uint32_t vlane[NULLS ? NCOL : 1];   //        ((lane + bit_offset) >> 3) * 4: ds_bpermute address of the row's byte in group 0 of a trip
  };
  static DEV void prepare(const DevProgram&, const DevFastPlan& F, PREP& W) {
#pragma unroll
    for (int t = 0; t < kPlanTerms; ++t) {
      const DevPlanTerm& T = F.scan.term[t];
      W.nlo[t] = plan_word64(0ull - T.lo);
      W.span[t] = plan_word64(T.span);
      W.flags[t] = plan_word((T.a != 0ull ? 1u : 0u) | ((T.b >> 63) ? 2u : 0u) | (T.inv ? 4u : 0u) | ((T.col & 3u) << 3) | (T.if_null ? 32u : 0u));
    }
    const uint32_t lane = (uint32_t)lane_id();
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      const uint32_t meta = F.scan.col_meta[c];
      if constexpr (W4) {
        const bool four = (meta & 15u) == 2u;
        W.is4[c] = plan_word(four ? 0xFFFFFFFFu : 0u);
        W.sext[c] = plan_word((four && ((meta >> 8) & 3u) == PX_SEXT32) ? 0xFFFFFFFFu : 0u);
        W.hi_half[c] = (four && ((lane + ((meta >> 4) & 1u)) & 1u)) ? 0xFFFFFFFFu : 0u;
      }
      if constexpr (NULLS) {
        const uint32_t at = lane + ((meta >> 16) & 7u);
        W.vshift[c] = at & 7u;
        W.vlane[c] = (at >> 3) << 2;
      }
    }
    W.key_sext = KEY4 ? plan_word(((F.scan.col_meta[0] >> 8) & 3u) == PX_SEXT32 ? 0xFFFFFFFFu : 0u) : 0u;
    if constexpr (!W4) W.hi_half[0] = W.is4[0] = W.sext[0] = 0;
    if constexpr (!NULLS) W.vshift[0] = W.vlane[0] = 0;
  }
  static DEV int na(const DevTable& T) { return FIXED ? 1 : T.na; }

  // C is the plan's own binding (bind_scan_plan): values = the column base rounded down to 8 bytes, validity = the byte
  // that holds row 0's bit (or the block of 0xFF bytes), bit_offset = the column word (plan_col_meta)
  static DEV void load(const DevProgram&, const DevColumns& C, int64_t row, bool inb, COLV& col, uint32_t& cv) {
    cv = 0xFFFFFFFFu;  // (vb holds every row's own byte)
    const uint64_t r = inb ? (uint64_t)row : 0ull;
    if constexpr (!NULLS) col.vb[0] = 0;
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      const uint32_t meta = (uint32_t)C.c[c].bit_offset;
      if constexpr (W4) {
        const uint64_t off = ((r + ((meta >> 4) & 1u)) << (meta & 15u)) & ~7ull;
        col.v[c] = __builtin_nontemporal_load((const uint64_t*)((const uint8_t*)C.c[c].values + off));
      } else if constexpr (KEY4) {
        if (c == 0)  // (values = the column base rounded down to 8 bytes; bit 4 of the column word: row 0 is the pair's second element)
          col.v[c] = (uint64_t)__builtin_nontemporal_load((const uint32_t*)C.c[c].values + ((meta >> 4) & 1u) + r);
        else
          col.v[c] = __builtin_nontemporal_load((const uint64_t*)C.c[c].values + r);
      } else {
        col.v[c] = __builtin_nontemporal_load((const uint64_t*)C.c[c].values + r);
      }
      if constexpr (NULLS) col.vb[c] = (uint32_t)C.c[c].validity[((r + ((meta >> 16) & 7u)) >> 3) & (0ull - (uint64_t)((meta >> 20) & 1u))];
    }
  }
  // one trip of U row groups from group w0: a scalar base per column, 32-bit lane offsets clamped to the batch's last row
  // (StaticPolicy::load_trip), every load unconditional.  Validity: ONE byte load per column and trip -- lane j takes byte j
  // of the trip's slice of the bitmap (U x 8 + 1 bytes at most) -- instead of one per row group: vector-memory instructions,
  // not bytes, are what a second load per group costs.  cv[u] = u tells eval which rows of the slice are its own.
  static DEV void load_trip(const DevColumns& C, int64_t w0, bool active, int64_t n, int lane, COLV (&col)[U], uint32_t (&cv)[U]) {
    const int64_t r0 = active ? w0 * 64 : 0;
    const int64_t left = n - r0;
    const bool none = !active || left <= 0;
    const uint32_t last = none ? 0u : (uint32_t)((left < (int64_t)U * 64 ? left : (int64_t)U * 64) - 1);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cv[u] = (uint32_t)u;
      if constexpr (!NULLS) col[u].vb[0] = 0;
    }
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      const uint32_t meta = (uint32_t)C.c[c].bit_offset;
      if constexpr (W4) {
        const uint32_t shift = meta & 15u, delta = (meta >> 4) & 1u;
        const uint8_t* p = (const uint8_t*)C.c[c].values + (none ? 0ull : ((uint64_t)r0 << shift));  // r0 is a multiple of 64: still 8-byte aligned
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (uint32_t)(u * 64 + lane);
          const uint32_t ic = i < last ? i : last;
          col[u].v[c] = __builtin_nontemporal_load((const uint64_t*)(p + (((ic + delta) << shift) & ~7u)));
        }
      } else if (KEY4 && c == 0) {
        const uint32_t* p = (const uint32_t*)C.c[c].values + ((meta >> 4) & 1u) + (none ? 0 : r0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (uint32_t)(u * 64 + lane);
          col[u].v[c] = (uint64_t)__builtin_nontemporal_load(p + (i < last ? i : last));
        }
      } else {
        const uint64_t* p = (const uint64_t*)C.c[c].values + (none ? 0 : r0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (uint32_t)(u * 64 + lane);
          col[u].v[c] = __builtin_nontemporal_load(p + (i < last ? i : last));
        }
      }
      if constexpr (NULLS) {
        const uint32_t vbit0 = (meta >> 16) & 7u;
        const uint32_t vmask = 0u - ((meta >> 20) & 1u);  // no bitmap: byte 0 of the ones block for every lane
        const uint8_t* pv = C.c[c].validity + ((none || vmask == 0u) ? 0ull : ((uint64_t)r0 >> 3));
        const uint32_t last_byte = (last + vbit0) >> 3;
        const uint32_t j = (uint32_t)lane < last_byte ? (uint32_t)lane : last_byte;
        const uint32_t bytes = (uint32_t)pv[j & vmask];
#pragma unroll
        for (int u = 0; u < U; ++u) col[u].vb[c] = bytes;
      }
    }
  }
  // widened values into reg[0 .. NCOL), validity bits into rv (bit c = slot c).  curv: the row group's index inside its trip
  // (load_trip), or ~0 (per-row loads).  Kernels that prepare() pass W; without it (never in the scan loops) the column words
  // are decoded here.
  static DEV void eval(const DevProgram& P, const DevFastPlan& F, const COLV& cur, uint32_t curv, u64x16& reg, uint32_t& rv, bool inb,
                       uint32_t& err) {
    PREP W;
    prepare(P, F, W);
    eval(P, F, cur, curv, reg, rv, inb, err, W);
  }
  static DEV void eval(const DevProgram&, const DevFastPlan& F, const COLV& cur, uint32_t curv, u64x16& reg, uint32_t& rv, bool,
                       uint32_t&, const PREP& W) {
    rv = 0xFFFFFFFFu;
    uint32_t valid = 0;
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      uint64_t x = cur.v[c];
      if constexpr (W4) {
        const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
        const uint32_t w = (hi & W.hi_half[c]) | (lo & ~W.hi_half[c]);  // (an 8-byte column: hi_half = 0, w = lo)
        const uint32_t xh = (hi & ~W.is4[c]) | ((uint32_t)((int32_t)w >> 31) & W.sext[c]);
        x = ((uint64_t)xh << 32) | w;
        if (((F.scan.col_meta[c] >> 8) & 3u) == PX_F32) x = f64_bits((double)__uint_as_float(w));  // (wave-uniform, rare; exact)
      }
      if constexpr (KEY4) {
        if (c == 0) x = ((uint64_t)((uint32_t)((int32_t)(uint32_t)x >> 31) & W.key_sext) << 32) | (uint32_t)x;
      }
      if constexpr (NULLS) {
        uint32_t byte = cur.vb[c];
        if (curv != 0xFFFFFFFFu)  // the trip's slice: this row's byte sits in lane (group x 64 + lane + bit_offset) / 8
          byte = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(W.vlane[c] + (curv << 5)), (int)byte);
        valid |= ((byte >> W.vshift[c]) & 1u) << c;
      }
      reg[c] = x;
    }
    if constexpr (NULLS) rv = valid;
  }
  // value of the term's column: a bitwise select by the slot's bits (vector masks: no scalar compare, no SGPR pair per term)
  static DEV uint64_t term_value(const u64x16& reg, uint32_t flags) {
    const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)flags, 3, 1);  // all ones: slot bit 0
    const uint64_t M0 = ((uint64_t)m0 << 32) | m0;
    if constexpr (NCOL <= 2) {
      return reg[0] ^ ((reg[0] ^ reg[NCOL > 1 ? 1 : 0]) & M0);
    } else {
      const uint32_t m1 = (uint32_t)__builtin_amdgcn_sbfe((int)flags, 4, 1);
      const uint64_t M1 = ((uint64_t)m1 << 32) | m1;
      const uint64_t y0 = reg[0] ^ ((reg[0] ^ reg[1]) & M0);
      const uint64_t y1 = reg[2] ^ ((reg[2] ^ reg[NCOL > 3 ? 3 : 2]) & M0);
      return y0 ^ ((y0 ^ y1) & M1);
    }
  }
  // (the host restates the five lines from `hi` to `r`, for the CPU tests of the planner: plan_term_passes, dfx_scan_plan.hpp)
  static DEV bool pass(const DevProgram&, const DevFastPlan& F, uint8_t, const COLV&, uint32_t, const u64x16& reg, uint32_t rv,
                       const PREP& W) {
    uint32_t ok = 1u;
#pragma unroll
    for (int t = 0; t < kPlanTerms; ++t) {
      if (t < F.scan.np) {  // (wave-uniform; nothing but vector arithmetic inside)
        const uint32_t f = W.flags[t];
        const uint64_t x = term_value(reg, f);
        const uint32_t hi = (uint32_t)(x >> 32);
        const uint32_t neg = (uint32_t)((int32_t)hi >> 31) & (uint32_t)__builtin_amdgcn_sbfe((int)f, 0, 1);  // all ones: a negative f64
        const uint32_t img_hi = hi ^ (neg & 0x7FFFFFFFu) ^ ((f << 30) & 0x80000000u);
        const uint64_t img = ((uint64_t)img_hi << 32) | ((uint32_t)x ^ neg);
        uint32_t r = ((img + W.nlo[t]) <= W.span[t] ? 1u : 0u) ^ ((f >> 2) & 1u);
        if constexpr (NULLS) r = ((rv >> ((f >> 3) & 3u)) & 1u) ? r : ((f >> 5) & 1u);
        ok &= r;
      }
    }
    return ok != 0u;
  }
  static DEV uint64_t key(const DevProgram&, const DevFastPlan& F, uint8_t, int k, const COLV&, uint32_t, const u64x16& reg, uint32_t) {
    if constexpr (FIXED) return reg[0];
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < kMaxKeys; ++j)  // k is a compile-time constant after unrolling at the call site
      if (j == k) v = plan_sel<NCOL>(reg, F.scan.keyslot[j]);
    return v;
  }
  static DEV void arg(const DevProgram&, const DevFastPlan& F, uint8_t, int a, const COLV&, uint32_t, const u64x16& reg, uint32_t rv,
                      uint64_t& v, bool& valid) {
    if constexpr (FIXED) {
      v = reg[NCOL > 1 ? 1 : 0];
      valid = (NULLS && F.scan.count_valid) ? ((rv >> 1) & 1u) != 0u : true;
    } else {
      v = 0;
      valid = true;
#pragma unroll
      for (int j = 0; j < kMaxAggs; ++j) {
        if (j == a) {
          const uint32_t slot = F.scan.argslot[j];
          v = plan_sel<NCOL>(reg, slot);
          if (NULLS && F.scan.count_valid) valid = ((rv >> slot) & 1u) != 0u;
        }
      }
    }
  }
  // the argument in plan column `slot` (wave-uniform, run-time: the pair scan's second operand, DevPartition::pair_slot1)
  static DEV void arg_slot(const DevFastPlan& F, uint32_t slot, const u64x16& reg, uint32_t rv, uint64_t& v, bool& valid) {
    v = plan_sel<NCOL>(reg, slot);
    valid = (NULLS && F.scan.count_valid) ? ((rv >> slot) & 1u) != 0u : true;
  }
};
template <int NCOL, int U, int GENK> using PlanPolicyN = PlanPolicy<NCOL, U, GENK, false>;  // any keys / arguments
template <int NCOL, int U, int GENK> using PlanPolicy1 = PlanPolicy<NCOL, U, GENK, true>;   // key in slot 0, one routed value in slot 1

}  // namespace dfx
