// dfx_scan_plan.hpp -- what a FastPolicy / PlanPolicy kernel reads, built on the host: arithmetic over the structs of
// dfx_device.hpp and nothing else.
//   recogniser: the SSA program of an operator (DevProgram) -> its decoded shape (DevFastPlan), once per operator;
//   planner:    the decoded shape + the columns of one batch -> the scan plan (DevFastPlan::scan, the plan-order DevColumns),
//               once per launch: column slots, the gen flavour bits, range images, neutral terms, count_valid.
// Host only and free of HIP; the one thing the planner needs of the runtime, the device's block of 0xFF bytes, is an argument.
// The names the library calls (ProgramBuilder::build_fast, scan_plan_shape_ok, bind_scan_plan: dfx_host.hpp, dfx_kernels.hpp)
// are one-line wrappers in dfx_expr_program.cpp.  tests/native/scan_plan_check.cpp holds every function here against the
// comparison it restates and against the code it was taken from.
#pragma once
#include <string.h>

#include "dfx_device.hpp"

namespace dfx {
namespace host_plan {

// -------------------------------------------------------------------------------------------------
// recogniser: DevProgram -> DevFastPlan
// -------------------------------------------------------------------------------------------------
inline bool fast_factor(const DevProgram& P, uint8_t opnd, DevFastFactor* f, uint64_t* imm) {
  const int kind = opnd >> 6, idx = opnd & 63;
  *imm = 0;
  if (kind == OPK_COL) {
    if (P.col_dtype[idx] != T_F64) return false;
    f->kind = FF_COL;
    f->col = (uint8_t)idx;
    return true;
  }
  if (kind != OPK_REG) return false;
  const DevIns& in = P.ins[idx];
  if (in.t != T_F64 || in.op < DOP_ADD || in.op > DOP_MUL) return false;
  const int ka = in.a >> 6, kb = in.b >> 6;
  const bool col_imm = ka == OPK_COL && kb == OPK_IMM, imm_col = ka == OPK_IMM && kb == OPK_COL;
  if (!col_imm && !imm_col) return false;
  f->col = (uint8_t)((col_imm ? in.a : in.b) & 63);
  *imm = P.imm[(col_imm ? in.b : in.a) & 63];
  if (in.op == DOP_ADD) f->kind = FF_COL_PLUS_IMM;        // f64 addition commutes bit for bit
  else if (in.op == DOP_MUL) f->kind = FF_COL_TIMES_IMM;  // so does multiplication
  else f->kind = col_imm ? FF_COL_MINUS_IMM : FF_IMM_MINUS_COL;
  return true;
}

// left-nested product ((f0 * f1) * f2) of factors, evaluated in the tree's own association
inline bool fast_product(const DevProgram& P, uint8_t opnd, DevFastArg* A, uint64_t* imms) {
  DevFastFactor f;
  uint64_t imm;
  if (fast_factor(P, opnd, &f, &imm)) {
    A->nf = 1;
    A->f[0] = f;
    imms[0] = imm;
    return true;
  }
  if ((opnd >> 6) != OPK_REG) return false;
  const DevIns& in = P.ins[opnd & 63];
  if (in.op != DOP_MUL || in.t != T_F64) return false;
  if (!fast_product(P, in.a, A, imms)) return false;
  if (A->nf >= 3) return false;
  if (!fast_factor(P, in.b, &f, &imm)) return false;
  A->f[A->nf] = f;
  imms[A->nf] = imm;
  A->nf++;
  return true;
}

inline bool fast_terms(const DevProgram& P, uint8_t opnd, DevFastPlan* F) {
  if ((opnd >> 6) != OPK_REG) return false;
  const DevIns& in = P.ins[opnd & 63];
  if (in.op == DOP_AND) return fast_terms(P, in.a, F) && fast_terms(P, in.b, F);
  if (in.op > DOP_GE) return false;
  const int ka = in.a >> 6, kb = in.b >> 6;
  const bool col_imm = ka == OPK_COL && kb == OPK_IMM, imm_col = ka == OPK_IMM && kb == OPK_COL;
  if ((!col_imm && !imm_col) || F->np >= 4) return false;
  int op = in.op;
  if (imm_col) {  // literal on the left: mirror the operator
    op = op == DOP_LT ? DOP_GT : op == DOP_LE ? DOP_GE : op == DOP_GT ? DOP_LT : op == DOP_GE ? DOP_LE : op;
  }
  DevFastTerm& t = F->term[F->np];
  t.col = (uint8_t)((col_imm ? in.a : in.b) & 63);
  t.dtype = in.t;
  t.m = op == DOP_EQ || op == DOP_NE ? 2 : op == DOP_LT ? 1 : op == DOP_LE ? 3 : op == DOP_GT ? 4 : 6;
  t.inv = op == DOP_NE ? 1 : 0;
  F->term_imm[F->np] = P.imm[(col_imm ? in.b : in.a) & 63];
  F->np++;
  return true;
}

// The decoded shape of a program (ProgramBuilder::build_fast): pred is a conjunction of `column <op> literal`, keys are plain
// columns, arguments are a column or a product of up to three (column | literal +- column | column * literal) factors.
// F->valid = 0 otherwise.
inline void build_fast_plan(const DevProgram& P, uint8_t pred, const uint8_t* keys, int kw, const uint8_t* args, int na, DevFastPlan* F) {
  memset(F, 0, sizeof(*F));
  if (pred != kNoOperand && !fast_terms(P, pred, F)) return;
  // One ordered Float64 comparison becomes the two-sided range the compile-time signatures are written for (dfx_sigs.hpp:
  // "WHERE c <op> lit AND c <op> lit"): `v < x` is `v >= -inf AND v < x`, `v > x` is `v > x AND v <= +inf`.  The added term
  // is true for every value the original term can pass (NaN fails both, as it fails the original), so the rows selected are
  // the same; lower bound first, so that the pair lands on one of the instantiated comparison forms (GT|GE, LT|LE).
  // Only where a signature can match afterwards (they read one or two columns): a run-time decoded plan of three or more
  // columns would merely pay for a second term.
  if (F->np == 1 && P.n_cols <= 2 && F->term[0].dtype == T_F64 && !F->term[0].inv && F->term[0].m != 2) {
    const bool upper = F->term[0].m == 1 || F->term[0].m == 3;
    const double inf = upper ? -__builtin_inf() : __builtin_inf();
    uint64_t bits;
    memcpy(&bits, &inf, 8);
    if (upper) {
      F->term[1] = F->term[0];
      F->term_imm[1] = F->term_imm[0];
      F->term[0].m = 6;  // >= -inf
      F->term_imm[0] = bits;
      F->synth = 1;
    } else {
      F->term[1] = F->term[0];
      F->term[1].m = 3;  // <= +inf
      F->term_imm[1] = bits;
      F->synth = 2;
    }
    F->np = 2;
  }
  for (int k = 0; k < kw; ++k) {
    if ((keys[k] >> 6) != OPK_COL) return;
    F->keycol[k] = (uint8_t)(keys[k] & 63);
  }
  for (int a = 0; a < na; ++a) {
    if ((args[a] >> 6) == OPK_COL) {  // plain column of any type
      F->arg[a].nf = 1;
      F->arg[a].f[0].kind = FF_COL;
      F->arg[a].f[0].col = (uint8_t)(args[a] & 63);
      continue;
    }
    if (!fast_product(P, args[a], &F->arg[a], F->arg_imm[a])) return;
  }
  F->valid = 1;
}

// -------------------------------------------------------------------------------------------------
// planner: scan plans (dfx_device.hpp: DevScanPlan), the shape family of DevFastPlan as data
// -------------------------------------------------------------------------------------------------
enum PlanClass { PC_NONE = 0, PC_F = 1, PC_I = 2, PC_U = 3 };
inline PlanClass plan_class(uint8_t t) {
  switch (t) {
    case T_F64: case T_F32: return PC_F;
    case T_I64: case T_I32: return PC_I;
    case T_U64: case T_U32: return PC_U;
    default: return PC_NONE;  // 1- and 2-byte columns, Boolean: other kernels
  }
}
inline bool plan_width4(uint8_t t) { return t == T_I32 || t == T_U32 || t == T_F32; }
inline uint64_t image_of(PlanClass c, uint64_t x) {
  if (c == PC_F) return (x >> 63) ? ~x : (x | 0x8000000000000000ull);
  if (c == PC_I) return x ^ 0x8000000000000000ull;
  return x;
}

// `value <op> literal` as an inclusive range of images (+ complement flag).  m: three-way mask of the operator (1 less, 2
// equal, 4 greater), ne: NotEq.  imm: the literal's canonical 64-bit form in the COLUMN's type.
inline void plan_term_range(uint8_t dtype, uint8_t m, bool ne, uint64_t imm, DevPlanTerm* T) {
  const PlanClass c = plan_class(dtype);
  T->a = c == PC_F ? 0x7FFFFFFFFFFFFFFFull : 0ull;
  T->b = c == PC_U ? 0ull : 0x8000000000000000ull;
  uint64_t LO = 0, HI = ~0ull, p, q;
  bool never = false;  // the comparison is false for every value (an unordered literal)
  if (c == PC_F) {
    double d;
    if (dtype == T_F32) {
      float f;
      const uint32_t b32 = (uint32_t)imm;
      memcpy(&f, &b32, 4);
      d = (double)f;  // exact: the kernels widen Float32 values the same way
    } else {
      memcpy(&d, &imm, 8);
    }
    const double ninf = -__builtin_inf(), pinf = __builtin_inf(), nz = -0.0, pz = 0.0;
    uint64_t bits;
    memcpy(&bits, &ninf, 8); LO = image_of(PC_F, bits);
    memcpy(&bits, &pinf, 8); HI = image_of(PC_F, bits);
    if (d != d) {
      never = true;
      p = q = 0;
    } else if (d == 0.0) {  // -0.0 == +0.0: the two images are neighbours
      memcpy(&bits, &nz, 8); p = image_of(PC_F, bits);
      memcpy(&bits, &pz, 8); q = image_of(PC_F, bits);
    } else {
      memcpy(&bits, &d, 8);
      p = q = image_of(PC_F, bits);
    }
  } else {
    p = q = image_of(c, imm);
  }
  uint64_t lo = 1, hi = 0;  // (empty)
  if (!never) {
    switch (m) {
      case 1: if (p > LO) { lo = LO; hi = p - 1; } break;        // <
      case 3: lo = LO; hi = q; break;                            // <=
      case 4: if (q < HI) { lo = q + 1; hi = HI; } break;        // >
      case 6: lo = p; hi = HI; break;                            // >=
      default: lo = p; hi = q; break;                            // == (and != as its complement)
    }
  }
  bool inv = ne;
  if (lo > hi) {  // no value passes: the complement of everything
    lo = 0;
    hi = ~0ull;
    inv = !inv;
  }
  T->lo = lo;
  T->span = hi - lo;
  T->inv = inv ? 1u : 0u;
  // arrow 0.12 bool_op compares Option<T>: None sorts below every value, the result is never null (expression.rs:171-210
  // -> array_ops; restated in run_program, dfx_k_interp_inl.hpp).  For `null <op> literal`:
  T->if_null = ne ? 1u : (m == 1 || m == 3) ? 1u : 0u;
}

// What a lane makes of a non-null value under a term: PlanPolicy::pass (dfx_k_plan_policy_inl.hpp, the five lines from `hi` to `r`)
// restated word for word, with the three flag bits of PlanPolicy::prepare it reads (bit 0: T.a != 0, bit 1: T.b >> 63, bit 2:
// T.inv) taken from the term itself.  x: the value widened to 64 bits, as PlanPolicy::eval leaves it in the row's register.
// The kernel's form is tuned (flag word, sbfe) and stays its own; tests/native/scan_plan_check.cpp and
// tests/test_scan_plan_host.py (through dfx_debug_plan_term) hold this one against the comparison operators.
inline bool plan_term_passes(const DevPlanTerm& T, uint64_t x) {
  const uint32_t hi = (uint32_t)(x >> 32);
  const uint32_t neg = (uint32_t)((int32_t)hi >> 31) & (T.a != 0ull ? 0xFFFFFFFFu : 0u);
  const uint32_t img_hi = hi ^ (neg & 0x7FFFFFFFu) ^ ((T.b >> 63) ? 0x80000000u : 0u);
  const uint64_t img = ((uint64_t)img_hi << 32) | ((uint32_t)x ^ neg);
  const uint64_t nlo = 0ull - T.lo;
  return (((img + nlo) <= T.span ? 1u : 0u) ^ (T.inv ? 1u : 0u)) != 0u;
}

// Shape check at operator-creation time (no batch needed): <= 4 columns of 4 / 8-byte numeric types, a conjunction of
// `column <op> literal` terms, plain-column keys, plain-column arguments.
inline bool scan_plan_shape_ok(const DevProgram& P, const DevFastPlan& F, int kw, int na, const uint8_t* val_xform) {
  if (!F.valid || P.n_cols < 1 || P.n_cols > kPlanCols || kw > kMaxKeys || na > kMaxAggs) return false;
  for (int c = 0; c < P.n_cols; ++c)
    if (plan_class(P.col_dtype[c]) == PC_NONE) return false;
  for (int k = 0; k < kw; ++k)
    if (plan_class(P.col_dtype[F.keycol[k]]) == PC_F) return false;  // (float keys are rejected long before, aggregate.rs:848-850)
  for (int a = 0; a < na; ++a) {
    if (F.arg[a].nf != 1 || F.arg[a].f[0].kind != FF_COL) return false;  // products stay with the decoded shapes
    const uint8_t t = P.col_dtype[F.arg[a].f[0].col];
    // the accumulators take the argument's own bits: a 4-byte argument is widened by the plan (Int32 as i64, Float32 as f64),
    // which only COUNT does not mind
    if (t != T_I64 && t != T_U64 && t != T_F64 && val_xform[a] != VT_COUNT_VALID) return false;
  }
  // the one-key kernels bind the key to slot 0 and the first argument to slot 1 even when they are the same column
  if (kw == 1 && na >= 1 && F.keycol[0] == F.arg[0].f[0].col && P.n_cols >= kPlanCols) return false;
  return true;
}

// ---- bind_scan_plan, step by step ----
struct PlanSlots {
  int n;                       // slots in use
  int src_of[kPlanCols + 2];   // slot -> program column
  int slot_of[kMaxCols];       // program column -> its (first) slot, -1: none
};

// Step 1, the slots: FIXED kernels find the key in slot 0 and the routed argument in slot 1; then the program's other columns.
// False: more than kPlanCols slots (scan_plan_shape_ok leaves no such shape: the check stays beside the array it guards).
inline bool assign_plan_slots(const DevProgram& P, const DevFastPlan& F, int kw, bool fixed, bool key4_slots, PlanSlots* L) {
  for (int c = 0; c < kMaxCols; ++c) L->slot_of[c] = -1;
  int n = 0;
  if (fixed) {
    L->src_of[n] = F.keycol[0];
    L->slot_of[F.keycol[0]] = n++;
    const int ac = F.arg[0].f[0].col;
    L->src_of[n] = ac;  // (the key column again when the aggregate is over the key: read twice, a cache hit)
    if (L->slot_of[ac] < 0) L->slot_of[ac] = n;
    ++n;
  } else if (key4_slots && kw == 1) {  // (slot look-ups: any order is right; the 4-byte-key kernels load slot 0 as the key)
    L->src_of[n] = F.keycol[0];
    L->slot_of[F.keycol[0]] = n++;
  }
  for (int c = 0; c < P.n_cols; ++c) {
    if (L->slot_of[c] >= 0) continue;
    if (n >= kPlanCols) return false;
    L->src_of[n] = c;
    L->slot_of[c] = n++;
  }
  L->n = n;
  return true;
}

// Step 2, one slot's column: the aligned 8 bytes that hold element 0, the byte that holds its validity bit (a column without a
// bitmap: the block of 0xFF bytes) and the column word.  in_use: the slot is one of the plan's (an unused slot is loaded too,
// but asks nothing of the kernels); *gen gains bit 0 for a 4-byte column in use, bit 1 for a bitmap in use.
// False: buffers the plan's loads cannot take.
inline bool bind_plan_column(uint8_t t, const DevColumn& col, const uint8_t* ones, bool in_use, DevColumn* out, uint32_t* meta, int* gen) {
  const bool w4 = plan_width4(t);
  const uintptr_t base = (uintptr_t)col.values;
  if ((base & (w4 ? 3u : 7u)) != 0) return false;  // (Arrow buffers are at least value-aligned; anything else: other kernels)
  const uint32_t ext = t == T_I32 ? PX_SEXT32 : t == T_U32 ? PX_ZEXT32 : t == T_F32 ? PX_F32 : PX_NONE;
  uint32_t vbit0 = 0;
  const uint8_t* vb = ones;
  if (col.validity) {
    if (col.bit_offset < 0) return false;
    vb = col.validity + (col.bit_offset >> 3);
    vbit0 = (uint32_t)(col.bit_offset & 7);
    if (in_use) *gen |= 2;
  }
  if (w4 && in_use) *gen |= 1;
  *meta = plan_col_meta(w4 ? 2u : 3u, w4 ? (uint32_t)((base & 7u) >> 2) : 0u, ext, vbit0, col.validity != nullptr);
  out->values = (const void*)(base & ~(uintptr_t)7);
  out->validity = vb;
  out->bit_offset = (int64_t)*meta;
  return true;
}

// Step 3, the terms (the open side build_fast_plan added to a one-sided range is left out: see DevFastPlan::synth), then
// neutral ones: every value passes.  False: more than kPlanTerms terms of the query's own.
inline bool plan_terms_of(const DevFastPlan& F, const int* slot_of, DevScanPlan* S) {
  int np = 0;
  for (int i = 0; i < F.np; ++i) {
    if ((F.synth >> i) & 1) continue;
    if (np >= kPlanTerms) return false;
    DevPlanTerm& T = S->term[np++];
    T.col = (uint32_t)slot_of[F.term[i].col];
    plan_term_range(F.term[i].dtype, F.term[i].m, F.term[i].inv != 0, F.term_imm[i], &T);
  }
  for (int i = np; i < kPlanTerms; ++i) {
    S->term[i].col = 0;
    S->term[i].lo = 0;
    S->term[i].span = ~0ull;
    S->term[i].if_null = 1;
  }
  S->np = np;
  return true;
}

// Step 4, "only the key is narrow": slot 0 holds an Int32 / UInt32 column and no other slot in use is 4 bytes wide.  Such a
// binding has a flavour of its own, a real 4-byte load of the key: gen bit 2 INSTEAD of bit 0.
inline bool only_key_is_narrow(const DevProgram& P, const PlanSlots& L) {
  if (P.col_dtype[L.src_of[0]] != T_I32 && P.col_dtype[L.src_of[0]] != T_U32) return false;
  for (int sl = 1; sl < L.n; ++sl)
    if (plan_width4(P.col_dtype[L.src_of[sl]])) return false;
  return true;
}
inline int key4_flavour(int gen, int n, DevColumns* Cout, DevScanPlan* S) {
  for (int sl = n; sl < kPlanCols; ++sl) {  // unused slots are read 8 bytes wide here: repeat slot 1, never the 4-byte key
    Cout->c[sl] = Cout->c[1];
    S->col_meta[sl] = S->col_meta[1];
  }
  return (gen & ~1) | 4;
}

// Per launch: the plan-order column binding (Cout) and the plan itself (Fout->scan) for the bound batch.  fixed: one key in
// slot 0 and the (first) argument in slot 1 (PlanPolicy1).  key4_slots: the caller has slot look-up kernels for "the key in
// slot 0 is the only 4-byte column".  ones: the device's block of 0xFF bytes (device_ones_block()).
// False: the shape or this batch's buffers are not covered.
inline bool bind_scan_plan(const DevProgram& P, const DevFastPlan& F, const DevColumns& C, int kw, int na, const uint8_t* val_xform,
                           bool fixed, DevFastPlan* Fout, DevColumns* Cout, bool key4_slots, const uint8_t* ones) {
  // (qualified: argument-dependent look-up would add the library's entry point of the same name, dfx_kernels.hpp)
  if ((F.plan_mode & 3) == 0 || !host_plan::scan_plan_shape_ok(P, F, kw, na, val_xform)) return false;
  if (fixed && (kw != 1 || na < 1)) return false;
  if (!ones) return false;
  *Fout = F;
  DevScanPlan& S = Fout->scan;
  memset(&S, 0, sizeof(S));
  memset(Cout, 0, sizeof(*Cout));
  PlanSlots L;
  if (!assign_plan_slots(P, F, kw, fixed, key4_slots, &L)) return false;
  S.n_cols = L.n;
  int gen = 0;
  for (int sl = 0; sl < kPlanCols; ++sl) {
    const int c = sl < L.n ? L.src_of[sl] : L.src_of[0];  // unused slots repeat slot 0 (loads are unconditional)
    if (!bind_plan_column(P.col_dtype[c], C.c[c], ones, sl < L.n, &Cout->c[sl], &S.col_meta[sl], &gen)) return false;
  }
  if (!plan_terms_of(F, L.slot_of, &S)) return false;
  for (int k = 0; k < kw; ++k) S.keyslot[k] = (uint8_t)L.slot_of[F.keycol[k]];
  for (int a = 0; a < na; ++a) S.argslot[a] = (uint8_t)L.slot_of[F.arg[a].f[0].col];
  if (fixed) S.argslot[0] = 1;
  // COUNT(x) looks at x's validity only when no Filter sits below: fn filter emits all-valid arrays (filter.rs:83-92), so
  // under an absorbed predicate every surviving slot counts (and every other aggregate reads value(row) regardless,
  // aggregate.rs:561-603)
  S.count_valid = F.np == 0 ? 1 : 0;
  // The key-4 flavour: of a one-key kernel (fixed; its test of the key's class is implied by only_key_is_narrow: kept as
  // found), and of a slot look-up binding whose caller has kernels for it (key4_slots: the pair scan over the key's Int32
  // shadow) and whose key did land in slot 0 with a slot 1 behind it.
  const bool key4_asked = fixed ? plan_class(P.col_dtype[L.src_of[0]]) != PC_F
                                : key4_slots && kw == 1 && L.n >= 2 && L.slot_of[F.keycol[0]] == 0;
  if ((gen & 1) && key4_asked && only_key_is_narrow(P, L)) gen = key4_flavour(gen, L.n, Cout, &S);
  S.gen = gen;
  S.valid = 1;
  return true;
}

}  // namespace host_plan
}  // namespace dfx
