// dfx_k_policy_inl.hpp -- the row-source policies of the scan kernels: how one 64-row group turns into (pass, keys, aggregate
// arguments).  Here: the contract, its defaults (PolicyDefaults), the interpreter as a policy (InterpPolicy), the decoded shape
// (FastPolicy), the compile-time signatures (StaticPolicy over dfx_sigs.hpp) and their forms over the column shadows (StaticKey4*).
// The scan plan's policy has a header of its own (dfx_k_plan_policy_inl.hpp).  Which policy a launch takes is chosen on the host:
// dfx_row_source.hpp, dfx_pass1_units.hpp.
// Who includes it: the scan kernels -- dfx_k_core.hip (k_project), dfx_k_filter.hip, and through dfx_k_plan_policy_inl.hpp
// dfx_k_reduce.hip, dfx_k_fewgroup.hip, dfx_k_table_inl.hpp, dfx_k_distinct_inl.hpp, dfx_k_partition_inl.hpp.
//
// THE CONTRACT.  A scan kernel is a template over POL and may ask it for the members below; after each, the kernels that read it.
// (k_partition* = k_partition, k_partition_sorted, k_partition_ring of dfx_k_partition_inl.hpp; "pass 1" = those and
// k_partition_ws; "the launchers" = host code of the same files.)
//   types and constants
//     COLV            one row's column values as a vector VALUE (the bank); every scan kernel
//     U               row groups a wave loads per trip; every scan kernel
//     PREP            per-wave state made once before the scan loop (PlanPolicy: its plan words in vector registers; else
//                     empty); k_reduce, k_fewgroup_agg, k_hash_agg, k_distinct_insert, pass 1
//     kIsStatic       a compile-time signature, so the comparison FORMs exist; k_reduce, k_filter_fused(_dense) and their
//                     launchers, launch_partition_ws
//     kHasTripLoad    load_trip is the policy's own (else: U calls of load); the free load_trip<POL> below
//     kPredTerms      predicate terms known at compile time, 0: none, -1: run-time; launch_partition_ws
//     kStaticNa       aggregates known at compile time, 0: run-time; k_reduce, k_filter_fused (launch bounds), k_partition_ring
//     kRow8, kRowPairs, kKeyPairs   the forms over the column shadows (below); k_partition_ws
//   before the loop
//     prepare(P, F, prep)                                   fills PREP; the kernels that read PREP
//     form_of(F)                                            the comparison FORM a plan matches, 0: run-time masks; the launchers
//                                                           of k_reduce, k_filter_fused(_dense) and k_partition_ws
//   loading
//     load(P, C, row, inb, col, cv)                         one row's columns; k_project, k_predicate_mask, k_hash_agg,
//                                                           k_distinct_insert, k_partition, k_partition_sorted, load_trip<POL>
//     load_trip(C, w0, active, n, lane, col[U], cv[U])      the U row groups of a trip (kHasTripLoad only); load_trip<POL>, which
//                                                           k_reduce, k_fewgroup_agg, k_filter_fused, k_partition_ring and
//                                                           k_partition_ws call
//   per row group
//     eval(P, F, cur, curv, reg, rv, inb, err[, prep])      computes what pass / key / arg read; every scan kernel
//     pass(P, F, pred, cur, curv, reg, rv[, prep])          the predicate; k_predicate_mask, k_fewgroup_agg, k_hash_agg, k_partition*
//     pass_form<FORM>(same)                                 ... its operators compile-time constants; k_reduce, k_filter_fused(_dense)
//     pass_mask<FORM>(same)                                 ... as the wave's lane mask; k_partition_ws
//     key(P, F, opnd, k, cur, curv, reg, rv)                key word k; k_fewgroup_agg, k_hash_agg, k_distinct_insert, pass 1
//     arg(P, F, opnd, a, cur, curv, reg, rv, v, valid)      aggregate argument a; k_reduce and the same
//     na(T), acc_kind(T, a), xform(T, a)                    the aggregates, run-time or the signature's; every aggregate scan kernel
//   optional, k_partition_ws alone, behind the flag named
//     kKeyPairs: pair_key(pairs, b, lane)                   two keys per lane (StaticKey4Policy)
//     kRowPairs: pair_row(pairs, b), trip_row(u, lane)      two rows per lane (StaticKey4Val4Policy)
//     kRow8:     pair_raw(pairs, b)                         the operand's shadow word for 8-byte routed rows (StaticKey4Val4Row8Policy)
//     arg_slot(F, slot, reg, rv, v, valid)                  PlanPolicyN: the pair scan's second operand (NV == 2)
#pragma once
#include "dfx_k_interp_inl.hpp"
#include "dfx_sigs.hpp"

namespace dfx {

// ---------------------------------------------------------------------------------------------
// row-source policies: how one 64-row group turns into (pass, keys, aggregate arguments)
// ---------------------------------------------------------------------------------------------
// Kernels are templated on a policy.  All state lives in kernel-local variables (vector VALUES,
// see the note in dfx_k_interp_inl.hpp); a policy is a bag of static inline functions.  Each kernel contains ONE
// copy of the evaluation code: the U prefetched row-groups are visited by a run-time loop that
// re-selects the group's column bank through a wave-uniform switch.
#define FOR_U _Pragma("unroll") for (int u = 0; u < U; ++u)
#define DFX_SELECT_BANK(uu, col, cv, cur, curv)                     \
  switch (uu) {                                                      \
    case 0: cur = col[0]; curv = cv[0]; break;                       \
    case 1: cur = col[U > 1 ? 1 : 0]; curv = cv[U > 1 ? 1 : 0]; break; \
    case 2: cur = col[U > 2 ? 2 : 0]; curv = cv[U > 2 ? 2 : 0]; break; \
    case 3: cur = col[U > 3 ? 3 : 0]; curv = cv[U > 3 ? 3 : 0]; break; \
    case 4: cur = col[U > 4 ? 4 : 0]; curv = cv[U > 4 ? 4 : 0]; break; \
    case 5: cur = col[U > 5 ? 5 : 0]; curv = cv[U > 5 ? 5 : 0]; break; \
    case 6: cur = col[U > 6 ? 6 : 0]; curv = cv[U > 6 ? 6 : 0]; break; \
    default: cur = col[U > 7 ? 7 : 0]; curv = cv[U > 7 ? 7 : 0]; break; \
  }

// The defaults of the contract: a run-time policy that loads row by row and knows nothing at compile time.  POL is the policy
// that derives from it (pass_form and pass_mask forward to POL::pass); a policy restates only what it specialises.
template <typename POL, typename COLV_, int U_>
struct PolicyDefaults {
  static constexpr bool kIsStatic = false;
  static constexpr bool kHasTripLoad = false;
  static constexpr bool kRow8 = false, kRowPairs = false, kKeyPairs = false;
  struct PREP {};  // per-wave state prepared before the scan loop (PlanPolicy: the plan words in vector registers)
  static DEV void prepare(const DevProgram&, const DevFastPlan&, PREP&) {}
  static constexpr int kPredTerms = -1;  // (run-time)
  static constexpr int U = U_;
  static constexpr int kStaticNa = 0;  // aggregates known at compile time (0: run-time)
  typedef COLV_ COLV;
  static DEV void load(const DevProgram& P, const DevColumns& C, int64_t row, bool inb, COLV& col, uint32_t& cv) {
    load_columns(P, C, row, inb, col, cv);
  }
  static DEV void load_trip(const DevColumns&, int64_t, bool, int64_t, int, COLV (&)[U_], uint32_t (&)[U_]) {}  // (kHasTripLoad only)
  static DEV int na(const DevTable& T) { return T.na; }
  static DEV uint8_t acc_kind(const DevTable& T, int a) { return T.acc_kind[a]; }
  static DEV uint8_t xform(const DevTable& T, int a) { return T.val_xform[a]; }
  static DEV int form_of(const DevFastPlan&) { return 0; }
  // (W: the policy's own PREP, which this base cannot name)
  template <int FORM, typename W = PREP>
  static DEV bool pass_form(const DevProgram& P, const DevFastPlan& F, uint8_t pred, const COLV& cur, uint32_t cv, const u64x16& reg, uint32_t rv, const W& prep = W()) {
    return POL::pass(P, F, pred, cur, cv, reg, rv, prep);
  }
  // the wave's lane mask of pass_form (scalar): what the scan loops that keep their predicates in masks call
  template <int FORM, typename W = PREP>
  static DEV uint64_t pass_mask(const DevProgram& P, const DevFastPlan& F, uint8_t pred, const COLV& cur, uint32_t cv, const u64x16& reg, uint32_t rv, const W& prep = W()) {
    return __ballot(POL::pass(P, F, pred, cur, cv, reg, rv, prep));
  }
};

// generic: the SSA register program (any expression the compiler accepts, nulls included)
template <int BANK, int U_>
struct InterpPolicy : PolicyDefaults<InterpPolicy<BANK, U_>, typename Bank<BANK>::type, U_> {
  typedef PolicyDefaults<InterpPolicy<BANK, U_>, typename Bank<BANK>::type, U_> Base;
  typedef typename Base::COLV COLV;
  typedef typename Base::PREP PREP;
  static DEV void eval(const DevProgram& P, const DevFastPlan&, const COLV& cur, uint32_t curv, u64x16& reg,
                       uint32_t& rv, bool inb, uint32_t& err, const PREP& = PREP()) {
    COLV c = cur;
    uint32_t cvv = curv;
    run_program(P, c, reg, cvv, rv, inb, err);
  }
  static DEV bool pass(const DevProgram& P, const DevFastPlan&, uint8_t pred, const COLV& cur, uint32_t curv,
                       const u64x16& reg, uint32_t rv, const PREP& = PREP()) {
    return eval_predicate(P, cur, reg, curv, rv, pred);
  }
  static DEV uint64_t key(const DevProgram& P, const DevFastPlan&, uint8_t opnd, int, const COLV& cur, uint32_t curv,
                          const u64x16& reg, uint32_t rv) {
    uint64_t v;
    bool valid;
    fetch(P, cur, reg, curv, rv, opnd, v, valid);
    return v;
  }
  static DEV void arg(const DevProgram& P, const DevFastPlan&, uint8_t opnd, int, const COLV& cur, uint32_t curv,
                      const u64x16& reg, uint32_t rv, uint64_t& v, bool& valid) {
    fetch(P, cur, reg, curv, rv, opnd, v, valid);
  }
};

// the interpreter for kernels that route ONE value per row (the narrow-row flavours of the partitioned pass 1): as FastPolicy1 --
// with the aggregate count a compile-time 1 the eight-wide value arrays of the routing code (16 VGPRs per row group, twice) drop
// out.  Round 5: the narrow ring kernel ran the interpreter at 128 VGPRs with 12 of them spilled to scratch -- and every scratch
// reload waits for the column loads in flight as well (one in-order counter)
template <int BANK, int U_>
struct InterpPolicy1 : InterpPolicy<BANK, U_> {
  static constexpr int kStaticNa = 1;
  static DEV int na(const DevTable&) { return 1; }
};

// three-way compare code of two canonical values of dtype t: 1 less, 2 equal, 4 greater, 0 unordered
DEV uint32_t cmp3(uint8_t t, uint64_t x, uint64_t y) {
  if (t == T_F64) {
    const double a = as_f64(x), b = as_f64(y);
    return (a < b ? 1u : 0u) | (a == b ? 2u : 0u) | (a > b ? 4u : 0u);
  }
  if (t == T_F32) {
    const float a = as_f32(x), b = as_f32(y);
    return (a < b ? 1u : 0u) | (a == b ? 2u : 0u) | (a > b ? 4u : 0u);
  }
  if (t == T_U64) return (x < y ? 1u : 0u) | (x == y ? 2u : 0u) | (x > y ? 4u : 0u);
  const int64_t a = (int64_t)x, b = (int64_t)y;
  return (a < b ? 1u : 0u) | (a == b ? 2u : 0u) | (a > b ? 4u : 0u);
}

// Wave-level comparison: the lane mask of `(cmp3(t, x, y) & m) != 0` for a wave-uniform m (it comes from the
// kernarg segment).  The three v_cmp write SGPR pairs and the selection by m runs on the scalar unit -- no
// per-lane select / or, no branch; the caller turns the final mask back into a per-lane predicate with
// inverse_ballot (a copy into VCC).  Bits of inactive lanes are meaningless.
template <typename TT>
DEV uint64_t cmp_mask_by(TT a, TT b, uint32_t m) {
  const uint64_t lt = __ballot(a < b), eq = __ballot(a == b), gt = __ballot(a > b);
  return ((m & 1u) ? lt : 0ull) | ((m & 2u) ? eq : 0ull) | ((m & 4u) ? gt : 0ull);
}
DEV uint64_t cmp_mask(uint8_t t, uint64_t x, uint64_t y, uint32_t m) {
  if (t == T_F64) return cmp_mask_by<double>(as_f64(x), as_f64(y), m);
  if (t == T_F32) return cmp_mask_by<float>(as_f32(x), as_f32(y), m);
  if (t == T_U64) return cmp_mask_by<uint64_t>(x, y, m);
  return cmp_mask_by<int64_t>((int64_t)x, (int64_t)y, m);
}
DEV bool lane_of_mask(uint64_t mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }

// shape-specialised (DevFastPlan): conjunction of `column <op> literal`, plain-column keys, column /
// short-product arguments; no nulls.  Straight-line code, the only scalar work is reading the plan.
template <int BANK, int U_>
struct FastPolicy : PolicyDefaults<FastPolicy<BANK, U_>, typename Bank<BANK>::type, U_> {
  typedef PolicyDefaults<FastPolicy<BANK, U_>, typename Bank<BANK>::type, U_> Base;
  typedef typename Base::COLV COLV;
  typedef typename Base::PREP PREP;
  static DEV void eval(const DevProgram&, const DevFastPlan&, const COLV&, uint32_t, u64x16&, uint32_t&, bool,
                       uint32_t&, const PREP& = PREP()) {}
  static DEV bool pass(const DevProgram&, const DevFastPlan& F, uint8_t, const COLV& cur, uint32_t, const u64x16&,
                       uint32_t, const PREP& = PREP()) {
    uint64_t ok = ~0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < F.np) {
        const DevFastTerm t = F.term[i];
        ok &= cmp_mask(t.dtype, cur[t.col & (BANK - 1)], F.term_imm[i], (uint32_t)t.m) ^ (t.inv ? ~0ull : 0ull);
      }
    }
    return lane_of_mask(ok);
  }
  static DEV uint64_t key(const DevProgram&, const DevFastPlan& F, uint8_t, int k, const COLV& cur, uint32_t,
                          const u64x16&, uint32_t) {
    return cur[F.keycol[k] & (BANK - 1)];
  }
  static DEV double factor(const DevFastPlan& F, int a, int j, const COLV& cur) {
    const DevFastFactor f = F.arg[a].f[j];
    const double x = as_f64(cur[f.col & (BANK - 1)]);
    const double imm = as_f64(F.arg_imm[a][j]);
    switch (f.kind) {
      case FF_IMM_MINUS_COL: return imm - x;
      case FF_COL_PLUS_IMM: return x + imm;
      case FF_COL_MINUS_IMM: return x - imm;
      case FF_COL_TIMES_IMM: return x * imm;
      default: return x;
    }
  }
  static DEV void arg(const DevProgram&, const DevFastPlan& F, uint8_t, int a, const COLV& cur, uint32_t,
                      const u64x16&, uint32_t, uint64_t& v, bool& valid) {
    valid = true;
    const DevFastArg A = F.arg[a];
    if (A.nf == 1 && A.f[0].kind == FF_COL) {
      v = cur[A.f[0].col & (BANK - 1)];
      return;
    }
    double acc = factor(F, a, 0, cur);
    if (A.nf > 1) acc = acc * factor(F, a, 1, cur);
    if (A.nf > 2) acc = acc * factor(F, a, 2, cur);
    v = f64_bits(acc);
  }
};

// FastPolicy for scans that route ONE value per row (one aggregate, or PTF_SHARED's common operand): the per-aggregate
// loops and their plan words (8 aggregates x 3 factors) drop out of the kernel
template <int BANK, int U_>
struct FastPolicy1 : FastPolicy<BANK, U_> {
  static constexpr int kStaticNa = 1;
  static DEV int na(const DevTable&) { return 1; }
};

// compile-time shape signature (dfx_sigs.hpp): column slots, term types, accumulator kinds and
// operand transforms are constants, every referenced column is 8 bytes wide, no nulls.  The only
// run-time inputs are the comparison masks and the literals.
template <int BANK, int U_, typename SIG>
struct StaticPolicy : PolicyDefaults<StaticPolicy<BANK, U_, SIG>, typename Bank<BANK>::type, U_> {
  typedef PolicyDefaults<StaticPolicy<BANK, U_, SIG>, typename Bank<BANK>::type, U_> Base;
  typedef typename Base::COLV COLV;
  typedef typename Base::PREP PREP;
  static constexpr int U = U_;
  static constexpr bool kIsStatic = true;
  static constexpr bool kHasTripLoad = true;
  static constexpr int kPredTerms = SIG::NP;  // 0: the signature has no predicate (every in-range row passes)
  static constexpr int kStaticNa = SIG::NA;
  static DEV void load(const DevProgram&, const DevColumns& C, int64_t row, bool inb, COLV& col, uint32_t& cv) {
    cv = 0xFFFFFFFFu;
#pragma unroll
    for (int c = 0; c < BANK; ++c)
      if (c < SIG::NCOL)  // streamed once: non-temporal, so the table blocks / open region lines keep the L2.
        // Out-of-range lanes re-read row 0 (no branch around the load: the compiler can then count the
        // loads in flight and software-pipelined kernels wait with vmcnt(N) instead of vmcnt(0)).
#ifdef DFX_COND_LOAD
        col[c] = inb ? __builtin_nontemporal_load((const uint64_t*)C.c[c].values + row) : 0ull;
#else
        col[c] = __builtin_nontemporal_load((const uint64_t*)C.c[c].values + (inb ? row : 0));
#endif
  }
  // The U row groups of one trip, starting at group w0 (wave-uniform): ONE scalar base per column and a 32-bit lane index
  // clamped to the last row of the batch (v_min_u32 + shift per load; the per-row form clamps a 64-bit index: six vector
  // instructions per load).  Lanes past the end re-read the last row (their rows are masked out by `row < n` later); an
  // inactive trip (w0 past the end: the software pipeline's last prefetch) reads row 0.  Unconditional loads: the compiler
  // can count them (vmcnt(N), not vmcnt(0)).
  static DEV void load_trip(const DevColumns& C, int64_t w0, bool active, int64_t n, int lane, COLV (&col)[U], uint32_t (&cv)[U]) {
    const int64_t r0 = active ? w0 * 64 : 0;
    const int64_t left = n - r0;
    const uint32_t last = (!active || left <= 0) ? 0u : (uint32_t)((left < (int64_t)U * 64 ? left : (int64_t)U * 64) - 1);
#pragma unroll
    for (int u = 0; u < U; ++u) cv[u] = 0xFFFFFFFFu;
#pragma unroll
    for (int c = 0; c < BANK; ++c) {
      if (c < SIG::NCOL) {
        const uint64_t* p = (const uint64_t*)C.c[c].values + ((!active || left <= 0) ? 0 : r0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t i = (uint32_t)(u * 64 + lane);
          col[u][c] = __builtin_nontemporal_load(p + (i < last ? i : last));
        }
      }
    }
  }
  static DEV int na(const DevTable&) { return SIG::NA; }
  static DEV uint8_t acc_kind(const DevTable&, int a) { return SIG::acc(a); }
  static DEV uint8_t xform(const DevTable&, int a) { return SIG::xf(a); }
  static DEV void eval(const DevProgram&, const DevFastPlan&, const COLV&, uint32_t, u64x16&, uint32_t&, bool,
                       uint32_t&, const PREP& = PREP()) {}
  static DEV bool pass(const DevProgram&, const DevFastPlan& F, uint8_t, const COLV& cur, uint32_t, const u64x16&,
                       uint32_t, const PREP& = PREP()) {
    uint64_t ok = ~0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < SIG::NP)
        ok &= cmp_mask(SIG::term_cls(i), cur[SIG::term_col(i)], F.term_imm[i], (uint32_t)F.term[i].m) ^
              (F.term[i].inv ? ~0ull : 0ull);
    }
    return lane_of_mask(ok);
  }
  // Comparison operators as COMPILE-TIME constants.  With run-time masks a term costs three v_cmp (less / equal / greater)
  // and a dozen scalar selects per row group; the operators of a query do not change while it runs, so the scan kernels
  // pick one of a few loop bodies once per wave: FORM = m0 | m1 << 3 | ... (three-way masks of the terms, none inverted),
  // 0 = the run-time form above.  form_of() names the FORM a plan matches (0 if none is instantiated).
  static __host__ __device__ inline int form_of(const DevFastPlan& F) {
    int form = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < SIG::NP) {
        if (F.term[i].inv || F.term[i].m < 1 || F.term[i].m > 6) return 0;
        form |= (int)F.term[i].m << (3 * i);
      }
    return form;
  }
  template <int M, typename TT>
  static DEV bool cmp_ct(TT a, TT b) {
    if constexpr (M == 1) return a < b;
    else if constexpr (M == 2) return a == b;
    else if constexpr (M == 3) return a <= b;
    else if constexpr (M == 4) return a > b;
    else if constexpr (M == 5) return a < b || a > b;
    else return a >= b;
  }
  template <int M>
  static DEV bool term_ct(uint8_t t, uint64_t x, uint64_t y) {
    if (t == T_F64) return cmp_ct<M, double>(as_f64(x), as_f64(y));
    if (t == T_F32) return cmp_ct<M, float>(as_f32(x), as_f32(y));
    if (t == T_U64) return cmp_ct<M, uint64_t>(x, y);
    return cmp_ct<M, int64_t>((int64_t)x, (int64_t)y);
  }
  template <int FORM>
  static DEV bool pass_form(const DevProgram& P, const DevFastPlan& F, uint8_t pred, const COLV& cur, uint32_t cv, const u64x16& reg, uint32_t rv, const PREP& = PREP()) {
    if constexpr (FORM == 0) {
      return pass(P, F, pred, cur, cv, reg, rv);
    } else {
      bool ok = true;
      if constexpr (SIG::NP > 0) ok = ok && term_ct<((FORM >> 0) & 7) ? ((FORM >> 0) & 7) : 1>(SIG::term_cls(0), cur[SIG::term_col(0)], F.term_imm[0]);
      if constexpr (SIG::NP > 1) ok = ok && term_ct<((FORM >> 3) & 7) ? ((FORM >> 3) & 7) : 1>(SIG::term_cls(1), cur[SIG::term_col(1)], F.term_imm[1]);
      if constexpr (SIG::NP > 2) ok = ok && term_ct<((FORM >> 6) & 7) ? ((FORM >> 6) & 7) : 1>(SIG::term_cls(2), cur[SIG::term_col(2)], F.term_imm[2]);
      if constexpr (SIG::NP > 3) ok = ok && term_ct<((FORM >> 9) & 7) ? ((FORM >> 9) & 7) : 1>(SIG::term_cls(3), cur[SIG::term_col(3)], F.term_imm[3]);
      return ok;
    }
  }
  // ... as the wave's lane mask: one ballot per TERM, the conjunction on the scalar unit.  (The ballot of `a && b` is lowered as
  // v_cndmask + v_cmp_ne on top of the two compares: each compare can write its SGPR pair directly.)
  template <int FORM>
  static DEV uint64_t pass_mask(const DevProgram& P, const DevFastPlan& F, uint8_t pred, const COLV& cur, uint32_t cv, const u64x16& reg, uint32_t rv, const PREP& = PREP()) {
    if constexpr (FORM == 0) {
      return __ballot(pass(P, F, pred, cur, cv, reg, rv));
    } else {
      uint64_t ok = ~0ull;
      if constexpr (SIG::NP > 0) ok &= __ballot(term_ct<((FORM >> 0) & 7) ? ((FORM >> 0) & 7) : 1>(SIG::term_cls(0), cur[SIG::term_col(0)], F.term_imm[0]));
      if constexpr (SIG::NP > 1) ok &= __ballot(term_ct<((FORM >> 3) & 7) ? ((FORM >> 3) & 7) : 1>(SIG::term_cls(1), cur[SIG::term_col(1)], F.term_imm[1]));
      if constexpr (SIG::NP > 2) ok &= __ballot(term_ct<((FORM >> 6) & 7) ? ((FORM >> 6) & 7) : 1>(SIG::term_cls(2), cur[SIG::term_col(2)], F.term_imm[2]));
      if constexpr (SIG::NP > 3) ok &= __ballot(term_ct<((FORM >> 9) & 7) ? ((FORM >> 9) & 7) : 1>(SIG::term_cls(3), cur[SIG::term_col(3)], F.term_imm[3]));
      return ok;
    }
  }
  static DEV uint64_t key(const DevProgram&, const DevFastPlan&, uint8_t, int k, const COLV& cur, uint32_t,
                          const u64x16&, uint32_t) {
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < kMaxKeys; ++j)  // k is a compile-time constant after unrolling at the call site
      if (j < SIG::KW && j == k) v = cur[SIG::key_col(j)];
    return v;
  }
  // factor j of aggregate argument a: kind and column are compile-time constants after unrolling
  static DEV double sfactor(const DevFastPlan& F, int a, int j, const COLV& cur) {
    const double x = as_f64(cur[SIG::fc(a, j) & (BANK - 1)]);
    const double imm = as_f64(F.arg_imm[a][j]);
    switch (SIG::fk(a, j)) {
      case FF_RT:  // the operator is the plan's: wave-uniform, read from the kernel arguments
        switch (F.arg[a].f[j].kind) {
          case FF_IMM_MINUS_COL: return imm - x;
          case FF_COL_PLUS_IMM: return x + imm;
          case FF_COL_MINUS_IMM: return x - imm;
          default: return x * imm;
        }
      case FF_IMM_MINUS_COL: return imm - x;
      case FF_COL_PLUS_IMM: return x + imm;
      case FF_COL_MINUS_IMM: return x - imm;
      case FF_COL_TIMES_IMM: return x * imm;
      default: return x;
    }
  }
  static DEV void arg(const DevProgram&, const DevFastPlan& F, uint8_t, int a, const COLV& cur, uint32_t,
                      const u64x16&, uint32_t, uint64_t& v, bool& valid) {
    valid = true;
    v = 0;
#pragma unroll
    for (int j = 0; j < kMaxAggs; ++j) {
      if (j < SIG::NA && j == a) {
        if (SIG::arg_dyn(j)) {  // product of signature-defined factors, multiplied left to right
          double acc = sfactor(F, j, 0, cur);
          if (SIG::nf(j) > 1) acc = acc * sfactor(F, j, 1, cur);
          if (SIG::nf(j) > 2) acc = acc * sfactor(F, j, 2, cur);
          v = f64_bits(acc);
        } else {
          v = cur[SIG::arg_col(j)];
        }
      }
    }
  }
};

// A two-column signature whose KEY column is bound as 4-byte words: the Int32 shadow of a resident Int64 key column whose keys
// are all below 2^32.  The scanner waves of k_partition_ws load two keys per lane: one 8-byte load per
// lane covers the keys of TWO row groups (128 rows), next to the two 8-byte operand loads of those rows -- every column load
// stays a 512-byte wave instruction, 12 bytes per row.  Row L of group 2j + b finds its key in lane 32 b + L / 2, half L & 1,
// of pair word j (pair_key: two ds_bpermute and a select).  Trips start on even groups (U is even, row0 a multiple of 64 and
// the binding 8-byte aligned), so a pair never straddles two trips.  Only the wave-specialised kernel knows this form.
template <int U_, typename SIG>
struct StaticKey4Policy : StaticPolicy<2, U_, SIG> {
  typedef StaticPolicy<2, U_, SIG> Base;
  typedef typename Base::COLV COLV;
  static constexpr int U = U_;
  static constexpr bool kKeyPairs = true;
  static constexpr int KC = SIG::key_col(0);
  static_assert(SIG::NCOL == 2 && SIG::KW == 1 && U_ % 2 == 0, "one operand column beside the key; whole pairs of row groups per trip");
  static DEV void load(const DevProgram&, const DevColumns& C, int64_t row, bool inb, COLV& col, uint32_t& cv) {  // (one row: its own key, zero-extended)
    cv = 0xFFFFFFFFu;
    col[1 - KC] = __builtin_nontemporal_load((const uint64_t*)C.c[1 - KC].values + (inb ? row : 0));
    col[KC] = (uint64_t)__builtin_nontemporal_load((const uint32_t*)C.c[KC].values + (inb ? row : 0));
  }
  // as StaticPolicy::load_trip; the key column: U / 2 pair words, col[2j][KC] = the keys of rows 128 j + 2 lane and + 1 of the trip.
  // The pair index is clamped to the pair that holds the batch's last row: an odd batch reads four bytes past its last key (the
  // next batch's first key, or the padding the shadow is allocated with).
  static DEV void load_trip(const DevColumns& C, int64_t w0, bool active, int64_t n, int lane, COLV (&col)[U], uint32_t (&cv)[U]) {
    const int64_t r0 = active ? w0 * 64 : 0;
    const int64_t left = n - r0;
    const bool none = !active || left <= 0;
    const uint32_t last = none ? 0u : (uint32_t)((left < (int64_t)U * 64 ? left : (int64_t)U * 64) - 1);
    const uint64_t* pv = (const uint64_t*)C.c[1 - KC].values + (none ? 0 : r0);
    const uint64_t* pk = (const uint64_t*)((const uint32_t*)C.c[KC].values + (none ? 0 : r0));
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cv[u] = 0xFFFFFFFFu;
      const uint32_t i = (uint32_t)(u * 64 + lane);
      col[u][1 - KC] = __builtin_nontemporal_load(pv + (i < last ? i : last));
      col[u][KC] = 0;
    }
    const uint32_t lastp = last >> 1;
#pragma unroll
    for (int j = 0; j < U / 2; ++j) {
      const uint32_t i = (uint32_t)(j * 64 + lane);
      col[2 * j][KC] = __builtin_nontemporal_load(pk + (i < lastp ? i : lastp));
    }
  }
  // the key of this lane's row in group 2j + b of the trip, from pair word j (every lane of the wave takes part)
  static DEV uint64_t pair_key(const COLV& pairs, int b, int lane) {
    const uint64_t w = pairs[KC];
    const int src = (b * 32 + (lane >> 1)) << 2;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)w);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(w >> 32));
    return (uint64_t)((lane & 1) ? hi : lo);
  }
};
// ... and whose OPERAND column is bound as 4-byte words too: the Float32 shadow of a resident Float64 column whose every value is
// exactly its float (dfx_value_shadow.hpp).  Both columns then have the same layout, and both are loaded as pair words: one
// 8-byte load per lane and column covers two row groups -- 512-byte wave instructions, 8 bytes per row.  Lane L owns rows 2 L and
// 2 L + 1 of the pair, so a row's key and operand sit in the same lane: "group" 2j of the trip is the pair's even rows, 2j + 1 its
// odd rows, no ds_bpermute and no select.  (Row order inside a trip does not matter to what is routed; the bounds test of the
// ragged last trip does, and uses trip_row.)  pair_row rebuilds the row as the 8-byte binding has it -- the key zero-extended,
// the operand widened by shadow_widen, the conversion the build checked --, and everything after it (predicate terms, FORM
// specialisations, the routed value) is StaticPolicy's own code over those 8-byte values.
template <int U_, typename SIG>
struct StaticKey4Val4Policy : StaticPolicy<2, U_, SIG> {
  typedef StaticPolicy<2, U_, SIG> Base;
  typedef typename Base::COLV COLV;
  static constexpr int U = U_;
  static constexpr bool kRowPairs = true;
  static constexpr int KC = SIG::key_col(0);
  static_assert(SIG::NCOL == 2 && SIG::KW == 1 && U_ % 2 == 0, "one operand column beside the key; whole pairs of row groups per trip");
  static DEV void load(const DevProgram&, const DevColumns& C, int64_t row, bool inb, COLV& col, uint32_t& cv) {  // (one row, as the 8-byte binding has it)
    cv = 0xFFFFFFFFu;
    col[1 - KC] = shadow_widen(__builtin_nontemporal_load((const uint32_t*)C.c[1 - KC].values + (inb ? row : 0)));
    col[KC] = (uint64_t)__builtin_nontemporal_load((const uint32_t*)C.c[KC].values + (inb ? row : 0));
  }
  // U / 2 pair words per column: col[2j][c] = the elements of rows 128 j + 2 lane and + 1 of the trip (col[2j + 1] is not used).
  // The pair index is clamped to the pair that holds the batch's last row: an odd batch reads four bytes past its last element
  // (the next batch's first, or the padding the shadows are allocated with).  (The opening is StaticKey4Policy::load_trip's, restated:
  // taken from one helper that returns r0 / last / lastp, all 36 kernels of the two key4 units came out with other registers.)
  static DEV void load_trip(const DevColumns& C, int64_t w0, bool active, int64_t n, int lane, COLV (&col)[U], uint32_t (&cv)[U]) {
    const int64_t r0 = active ? w0 * 64 : 0;
    const int64_t left = n - r0;
    const bool none = !active || left <= 0;
    const uint32_t last = none ? 0u : (uint32_t)((left < (int64_t)U * 64 ? left : (int64_t)U * 64) - 1);
    const uint32_t lastp = last >> 1;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cv[u] = 0xFFFFFFFFu;
      col[u][0] = 0;
      col[u][1] = 0;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint64_t* p = (const uint64_t*)((const uint32_t*)C.c[c].values + (none ? 0 : r0));
#pragma unroll
      for (int j = 0; j < U / 2; ++j) {
        const uint32_t i = (uint32_t)(j * 64 + lane);
        col[2 * j][c] = __builtin_nontemporal_load(p + (i < lastp ? i : lastp));
      }
    }
  }
  // the row of the trip that this lane holds in "group" u (group 2j + b: row b of the lane's pair in pair word j)
  static DEV int64_t trip_row(int u, int lane) { return (int64_t)(u >> 1) * 128 + 2 * lane + (u & 1); }
  static DEV COLV pair_row(const COLV& pairs, int b) {
    COLV row;
    const uint32_t k = b ? (uint32_t)(pairs[KC] >> 32) : (uint32_t)pairs[KC];
    const uint32_t w = b ? (uint32_t)(pairs[1 - KC] >> 32) : (uint32_t)pairs[1 - KC];
    row[KC] = (uint64_t)k;
    row[1 - KC] = shadow_widen(w);
    return row;
  }
};
// ... for regions of 8-byte rows (PTF_ROW8: every launch of the window binds both shadows).  The same loads, the same predicate
// over the widened operand; what the scanner hands the router is the operand's shadow word itself (pair_raw) -- the aggregate is
// SUM of the plain operand column, so the widened word is the routed value and pass 2 does that widening (shadow_widen).
template <int U_, typename SIG>
struct StaticKey4Val4Row8Policy : StaticKey4Val4Policy<U_, SIG> {
  typedef typename StaticKey4Val4Policy<U_, SIG>::COLV COLV;
  static constexpr bool kRow8 = true;
  static constexpr int KC = SIG::key_col(0);
  static_assert(SIG::NA == 1 && !SIG::arg_dyn(0) && SIG::arg_col(0) == 1 - KC && SIG::xf(0) == VT_RAW, "the routed value is the operand column itself");
  static DEV uint32_t pair_raw(const COLV& pairs, int b) { return b ? (uint32_t)(pairs[1 - KC] >> 32) : (uint32_t)pairs[1 - KC]; }
};

// the column loads of one trip of U row groups starting at group w0 (wave-uniform); `active` false: nothing is needed (the
// software pipeline's prefetch past the end), the loads still happen (row 0) so that their count stays fixed
template <typename POL>
DEV void load_trip(const DevProgram& P, const DevColumns& C, int64_t w0, bool active, int64_t n, int lane,
                   typename POL::COLV (&col)[POL::U], uint32_t (&cv)[POL::U]) {
  if constexpr (POL::kHasTripLoad) {
    POL::load_trip(C, w0, active, n, lane, col, cv);
  } else {
#pragma unroll
    for (int u = 0; u < POL::U; ++u) {
      const int64_t row = (w0 + u) * 64 + lane;
      POL::load(P, C, row, active && row < n, col[u], cv[u]);
    }
  }
}

// signature list: index == sig id handed to the launchers; -1: none
template <int BANK, int U> using PolPred2F64 = StaticPolicy<BANK, U, SigPred2F64>;

}  // namespace dfx
