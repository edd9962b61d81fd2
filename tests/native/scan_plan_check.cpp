// scan_plan_check.cpp -- the host side of the FastPolicy / PlanPolicy kernels (csrc/dfx_scan_plan.hpp) as a stand-alone program:
//   (a) plan_term_range + plan_term_passes against the C++ comparison of the typed values, every operator over NaN of both signs,
//       +-0, +-inf, subnormals, the integer extremes and random bit patterns, six column types; if_null against arrow 0.12's table;
//   (b) bind_scan_plan against the function it was taken apart from (former_bind_scan_plan, below, with former_scan_plan_shape_ok),
//       return value and on success DevFastPlan::scan and the plan-order DevColumns byte for byte, with counters that hold the
//       space to what it is meant to reach: every refusal site, every gen value, the key-4 rule through both of its doors;
//   (c) build_fast_plan against the former fast_factor / fast_product / fast_terms / ProgramBuilder::build_fast over hand-built
//       programs, DevFastPlan byte for byte.
// The former functions are the library's text before the header existed, verbatim but for: the ones block and the program are
// parameters (they were device_ones_block() and prog_), and every `return false` of the two planner functions is REFUSE(site),
// which counts the site.  tests/test_scan_plan.py builds this plain and with -fsanitize=address,undefined.
#include <initializer_list>
#include <stdio.h>
#include <string.h>

#include "../../datafusion_archive_amd/csrc/dfx_scan_plan.hpp"

using namespace dfx;
using namespace dfx::host_plan;

static int failures = 0;
#define CHECK(cond)                                    \
  do {                                                 \
    if (!(cond)) {                                     \
      if (failures < 40) printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++failures;                                      \
    }                                                  \
  } while (0)

static uint64_t rng_state = 0x20261020ull;  // (fixed seed: splitmix64)
static uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

// ---- the former functions ---------------------------------------------------------------------------------------------
enum { DFX_FLOAT64 = T_F64 };  // (the former recogniser named the type by include/dfx.h's code: the same number)
enum Site {
  // former_bind_scan_plan
  S_MODE_OR_SHAPE, S_FIXED_COUNTS, S_NO_ONES, S_TOO_MANY_SLOTS, S_MISALIGNED, S_NEGATIVE_BIT_OFFSET, S_TOO_MANY_TERMS,
  // former_scan_plan_shape_ok
  S_NOT_VALID_OR_COUNTS, S_UNCOVERED_TYPE, S_FLOAT_KEY, S_PRODUCT_ARG, S_NARROW_ARG, S_KEY_IS_ARG_AND_FULL,
  S_COUNT_
};
static const char* kSiteName[S_COUNT_] = {"mode_or_shape", "fixed_counts", "no_ones", "too_many_slots", "misaligned", "negative_bit_offset",
                                          "too_many_terms", "not_valid_or_counts", "uncovered_type", "float_key", "product_arg",
                                          "narrow_arg", "key_is_arg_and_full"};
static long site_hits[S_COUNT_];
#define REFUSE(site) return (++site_hits[site], false)

namespace former {
bool fast_factor(const DevProgram& P, uint8_t opnd, DevFastFactor* f, uint64_t* imm) {
  const int kind = opnd >> 6, idx = opnd & 63;
  *imm = 0;
  if (kind == OPK_COL) {
    if (P.col_dtype[idx] != DFX_FLOAT64) return false;
    f->kind = FF_COL;
    f->col = (uint8_t)idx;
    return true;
  }
  if (kind != OPK_REG) return false;
  const DevIns& in = P.ins[idx];
  if (in.t != DFX_FLOAT64 || in.op < DOP_ADD || in.op > DOP_MUL) return false;
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
bool fast_product(const DevProgram& P, uint8_t opnd, DevFastArg* A, uint64_t* imms) {
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
  if (in.op != DOP_MUL || in.t != DFX_FLOAT64) return false;
  if (!fast_product(P, in.a, A, imms)) return false;
  if (A->nf >= 3) return false;
  if (!fast_factor(P, in.b, &f, &imm)) return false;
  A->f[A->nf] = f;
  imms[A->nf] = imm;
  A->nf++;
  return true;
}

bool fast_terms(const DevProgram& P, uint8_t opnd, DevFastPlan* F) {
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

void build_fast(const DevProgram& prog_, uint8_t pred, const uint8_t* keys, int kw, const uint8_t* args, int na,
                DevFastPlan* F) {
  memset(F, 0, sizeof(*F));
  if (pred != kNoOperand && !fast_terms(prog_, pred, F)) return;
  if (F->np == 1 && prog_.n_cols <= 2 && F->term[0].dtype == T_F64 && !F->term[0].inv && F->term[0].m != 2) {
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
    if (!fast_product(prog_, args[a], &F->arg[a], F->arg_imm[a])) return;
  }
  F->valid = 1;
}

bool former_scan_plan_shape_ok(const DevProgram& P, const DevFastPlan& F, int kw, int na, const uint8_t* val_xform) {
  if (!F.valid || P.n_cols < 1 || P.n_cols > kPlanCols || kw > kMaxKeys || na > kMaxAggs) REFUSE(S_NOT_VALID_OR_COUNTS);
  for (int c = 0; c < P.n_cols; ++c)
    if (plan_class(P.col_dtype[c]) == PC_NONE) REFUSE(S_UNCOVERED_TYPE);
  for (int k = 0; k < kw; ++k)
    if (plan_class(P.col_dtype[F.keycol[k]]) == PC_F) REFUSE(S_FLOAT_KEY);  // (float keys are rejected long before, aggregate.rs:848-850)
  for (int a = 0; a < na; ++a) {
    if (F.arg[a].nf != 1 || F.arg[a].f[0].kind != FF_COL) REFUSE(S_PRODUCT_ARG);  // products stay with the decoded shapes
    const uint8_t t = P.col_dtype[F.arg[a].f[0].col];
    if (t != T_I64 && t != T_U64 && t != T_F64 && val_xform[a] != VT_COUNT_VALID) REFUSE(S_NARROW_ARG);
  }
  if (kw == 1 && na >= 1 && F.keycol[0] == F.arg[0].f[0].col && P.n_cols >= kPlanCols) REFUSE(S_KEY_IS_ARG_AND_FULL);
  return true;
}

bool former_bind_scan_plan(const DevProgram& P, const DevFastPlan& F, const DevColumns& C, int kw, int na, const uint8_t* val_xform,
                           bool fixed, DevFastPlan* Fout, DevColumns* Cout, bool key4_slots, const uint8_t* ones) {
  if ((F.plan_mode & 3) == 0 || !former_scan_plan_shape_ok(P, F, kw, na, val_xform)) REFUSE(S_MODE_OR_SHAPE);
  if (fixed && (kw != 1 || na < 1)) REFUSE(S_FIXED_COUNTS);
  if (!ones) REFUSE(S_NO_ONES);
  *Fout = F;
  DevScanPlan& S = Fout->scan;
  memset(&S, 0, sizeof(S));
  memset(Cout, 0, sizeof(*Cout));
  // plan slots: FIXED kernels find the key in slot 0 and the routed argument in slot 1; then the program's other columns
  int slot_of[kMaxCols];
  for (int c = 0; c < kMaxCols; ++c) slot_of[c] = -1;
  int src_of[kPlanCols + 2];
  int n = 0;
  if (fixed) {
    src_of[n] = F.keycol[0];
    slot_of[F.keycol[0]] = n++;
    const int ac = F.arg[0].f[0].col;
    src_of[n] = ac;  // (the key column again when the aggregate is over the key: read twice, a cache hit)
    if (slot_of[ac] < 0) slot_of[ac] = n;
    ++n;
  } else if (key4_slots && kw == 1) {  // (slot look-ups: any order is right; the 4-byte-key kernels load slot 0 as the key)
    src_of[n] = F.keycol[0];
    slot_of[F.keycol[0]] = n++;
  }
  for (int c = 0; c < P.n_cols; ++c) {
    if (slot_of[c] >= 0) continue;
    if (n >= kPlanCols) REFUSE(S_TOO_MANY_SLOTS);
    src_of[n] = c;
    slot_of[c] = n++;
  }
  S.n_cols = n;
  int gen = 0;
  for (int sl = 0; sl < kPlanCols; ++sl) {
    const int c = sl < n ? src_of[sl] : src_of[0];  // unused slots repeat slot 0 (loads are unconditional)
    const uint8_t t = P.col_dtype[c];
    const bool w4 = t == T_I32 || t == T_U32 || t == T_F32;
    const uintptr_t base = (uintptr_t)C.c[c].values;
    if ((base & (w4 ? 3u : 7u)) != 0) REFUSE(S_MISALIGNED);  // (Arrow buffers are at least value-aligned; anything else: other kernels)
    const uint32_t ext = t == T_I32 ? PX_SEXT32 : t == T_U32 ? PX_ZEXT32 : t == T_F32 ? PX_F32 : PX_NONE;
    uint32_t vbit0 = 0;
    const uint8_t* vb = ones;
    if (C.c[c].validity) {
      if (C.c[c].bit_offset < 0) REFUSE(S_NEGATIVE_BIT_OFFSET);
      vb = C.c[c].validity + (C.c[c].bit_offset >> 3);
      vbit0 = (uint32_t)(C.c[c].bit_offset & 7);
      if (sl < n) gen |= 2;
    }
    if (w4 && sl < n) gen |= 1;
    const uint32_t meta = plan_col_meta(w4 ? 2u : 3u, w4 ? (uint32_t)((base & 7u) >> 2) : 0u, ext, vbit0, C.c[c].validity != nullptr);
    Cout->c[sl].values = (const void*)(base & ~(uintptr_t)7);
    Cout->c[sl].validity = vb;
    Cout->c[sl].bit_offset = (int64_t)meta;
    S.col_meta[sl] = meta;
  }
  // terms (the open side build_fast added to a one-sided range is left out: see DevFastPlan::synth)
  int np = 0;
  for (int i = 0; i < F.np; ++i) {
    if ((F.synth >> i) & 1) continue;
    if (np >= kPlanTerms) REFUSE(S_TOO_MANY_TERMS);
    DevPlanTerm& T = S.term[np++];
    T.col = (uint32_t)slot_of[F.term[i].col];
    plan_term_range(F.term[i].dtype, F.term[i].m, F.term[i].inv != 0, F.term_imm[i], &T);
  }
  for (int i = np; i < kPlanTerms; ++i) {  // neutral: every value passes
    S.term[i].col = 0;
    S.term[i].lo = 0;
    S.term[i].span = ~0ull;
    S.term[i].if_null = 1;
  }
  S.np = np;
  for (int k = 0; k < kw; ++k) S.keyslot[k] = (uint8_t)slot_of[F.keycol[k]];
  for (int a = 0; a < na; ++a) S.argslot[a] = (uint8_t)slot_of[F.arg[a].f[0].col];
  if (fixed) S.argslot[0] = 1;
  S.count_valid = F.np == 0 ? 1 : 0;
  // the Int32 / UInt32 key of a one-key kernel with nothing else to widen: its own flavour (a real 4-byte load of the key)
  if (fixed && (gen & 1)) {
    bool only_key = plan_class(P.col_dtype[src_of[0]]) != PC_F && (P.col_dtype[src_of[0]] == T_I32 || P.col_dtype[src_of[0]] == T_U32);
    for (int sl = 1; sl < n && only_key; ++sl) {
      const uint8_t t = P.col_dtype[src_of[sl]];
      if (t == T_I32 || t == T_U32 || t == T_F32) only_key = false;
    }
    if (only_key) {
      gen = (gen & ~1) | 4;
      for (int sl = n; sl < kPlanCols; ++sl) {  // unused slots are read 8 bytes wide here: repeat slot 1, never the 4-byte key
        Cout->c[sl] = Cout->c[1];
        S.col_meta[sl] = S.col_meta[1];
      }
    }
  }
  // ... and of a slot look-up binding whose caller has kernels for it (key4_slots: the pair scan over the key's Int32 shadow)
  if (!fixed && key4_slots && (gen & 1) && kw == 1 && n >= 2 && slot_of[F.keycol[0]] == 0) {
    bool only_key = P.col_dtype[src_of[0]] == T_I32 || P.col_dtype[src_of[0]] == T_U32;
    for (int sl = 1; sl < n && only_key; ++sl) {
      const uint8_t t = P.col_dtype[src_of[sl]];
      if (t == T_I32 || t == T_U32 || t == T_F32) only_key = false;
    }
    if (only_key) {
      gen = (gen & ~1) | 4;
      for (int sl = n; sl < kPlanCols; ++sl) {
        Cout->c[sl] = Cout->c[1];
        S.col_meta[sl] = S.col_meta[1];
      }
    }
  }
  S.gen = gen;
  S.valid = 1;
  return true;
}
}  // namespace former

// ---- (a) terms against the comparison they restate ---------------------------------------------------------------------
static uint64_t f64_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static double bits_f64(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static float bits_f32(uint64_t b) { const uint32_t w = (uint32_t)b; float f; memcpy(&f, &w, 4); return f; }
static uint64_t f32_bits(float f) { uint32_t w; memcpy(&w, &f, 4); return w; }

template <typename T>
static bool compare(int op, T a, T b) {  // dfx_operator 0..5: Eq NotEq Lt LtEq Gt GtEq
  switch (op) {
    case 0: return a == b;
    case 1: return a != b;
    case 2: return a < b;
    case 3: return a <= b;
    case 4: return a > b;
    default: return a >= b;
  }
}
// `value <op> literal` of the column's type, both in canonical 64-bit form (signed: sign-extended, Float32: bits in the low word)
static bool typed_compare(uint8_t t, int op, uint64_t value, uint64_t literal) {
  switch (t) {
    case T_I32: return compare<int32_t>(op, (int32_t)(uint32_t)value, (int32_t)(uint32_t)literal);
    case T_U32: return compare<uint32_t>(op, (uint32_t)value, (uint32_t)literal);
    case T_F32: return compare<float>(op, bits_f32(value), bits_f32(literal));
    case T_I64: return compare<int64_t>(op, (int64_t)value, (int64_t)literal);
    case T_U64: return compare<uint64_t>(op, value, literal);
    default: return compare<double>(op, bits_f64(value), bits_f64(literal));
  }
}
// a bit pattern as a canonical value of the type
static uint64_t canon(uint8_t t, uint64_t bits) {
  switch (t) {
    case T_I32: return (uint64_t)(int64_t)(int32_t)(uint32_t)bits;
    case T_U32: case T_F32: return (uint64_t)(uint32_t)bits;
    default: return bits;
  }
}
// what PlanPolicy::eval leaves in the row's register: the value widened to 64 bits (Float32 -> Float64 is exact)
static uint64_t widened(uint8_t t, uint64_t value) { return t == T_F32 ? f64_bits((double)bits_f32(value)) : value; }

static const uint8_t kThreeWay[6] = {2, 2, 1, 3, 4, 6};  // Eq NotEq Lt LtEq Gt GtEq (fast_terms)
static long term_cells = 0;

static void check_terms_of(uint8_t t, const uint64_t* vals, int n) {
  static const uint32_t if_null[6] = {0, 1, 1, 1, 0, 0};  // arrow 0.12 bool_op over Option<T>: None sorts below every value
  for (int l = 0; l < n; ++l)
    for (int op = 0; op < 6; ++op) {
      DevPlanTerm T;
      memset(&T, 0, sizeof(T));
      plan_term_range(t, kThreeWay[op], op == 1, vals[l], &T);
      CHECK(T.if_null == if_null[op]);
      for (int v = 0; v < n; ++v) {
        const bool got = plan_term_passes(T, widened(t, vals[v])), want = typed_compare(t, op, vals[v], vals[l]);
        if (got != want && failures < 40)
          printf("term: dtype %d op %d value %016llx literal %016llx: plan %d, comparison %d\n", (int)t, op, (unsigned long long)vals[v],
                 (unsigned long long)vals[l], (int)got, (int)want);
        CHECK(got == want);
        ++term_cells;
      }
    }
}

static void check_terms() {
  const double inf = __builtin_inf();
  const uint64_t f64_edges[] = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, f64_bits(inf), f64_bits(-inf), f64_bits(0.0),
                                f64_bits(-0.0), 1ull, 0x8000000000000001ull, f64_bits(2.2250738585072014e-308), f64_bits(1.0), f64_bits(-1.0),
                                f64_bits(1.0000000000000002), f64_bits(0.9999999999999999), f64_bits(204.8), f64_bits(409.6),
                                f64_bits(1.7976931348623157e308), f64_bits(-1.7976931348623157e308), f64_bits(3.5), f64_bits(-3.5)};
  const uint64_t f32_edges[] = {0x7FC00000ull, 0xFFC00000ull, 0x7F800001ull, f32_bits((float)inf), f32_bits((float)-inf), f32_bits(0.0f), f32_bits(-0.0f),
                                1ull, 0x80000001ull, 0x00800000ull, f32_bits(1.0f), f32_bits(-1.0f), f32_bits(1.0000001f), f32_bits(3.4028235e38f),
                                f32_bits(-3.4028235e38f), f32_bits(16777216.0f)};
  const int64_t i64_edges[] = {0, 1, -1, 2, -2, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MIN + 1, 1ll << 31, -(1ll << 31), 1ll << 32, 12345, -12345};
  const int32_t i32_edges[] = {0, 1, -1, INT32_MAX, INT32_MIN, INT32_MAX - 1, INT32_MIN + 1, 65536, -65536, 7};
  const uint64_t u64_edges[] = {0, 1, 2, 1ull << 63, (1ull << 63) - 1, UINT64_MAX, UINT64_MAX - 1, 1ull << 32, (1ull << 32) - 1};
  const uint64_t u32_edges[] = {0, 1, 2, 1ull << 31, (1ull << 31) - 1, UINT32_MAX, UINT32_MAX - 1};
  const uint8_t types[6] = {T_I32, T_U32, T_F32, T_I64, T_U64, T_F64};
  for (uint8_t t : types) {
    uint64_t vals[96];
    int n = 0;
    switch (t) {
      case T_F64: for (uint64_t b : f64_edges) vals[n++] = b; break;
      case T_F32: for (uint64_t b : f32_edges) vals[n++] = b; break;
      case T_I64: for (int64_t x : i64_edges) vals[n++] = (uint64_t)x; break;
      case T_I32: for (int32_t x : i32_edges) vals[n++] = (uint64_t)(int64_t)x; break;
      case T_U64: for (uint64_t x : u64_edges) vals[n++] = x; break;
      default: for (uint64_t x : u32_edges) vals[n++] = x; break;
    }
    // the edge values against each other, then with random bit patterns mixed in (every pair of the list, both ways round)
    check_terms_of(t, vals, n);
    for (int round = 0; round < 40; ++round) {
      const int keep = 8;  // a few edges stay in every round, so that random values meet them
      uint64_t mix[96];
      int m = 0;
      for (int i = 0; i < keep; ++i) mix[m++] = vals[below(n)];
      while (m < 40) {
        uint64_t b = rnd();
        if (below(4) == 0) b = (b & 0x800FFFFFFFFFFFFFull) | ((uint64_t)(below(2) ? 0x7FF : below(0x7FF)) << 52);  // Float64: more NaN, inf, subnormals
        if (below(4) == 0) b = (b & ~0x7F800000ull) | ((uint64_t)(below(2) ? 0xFF : below(0xFF)) << 23);            // Float32: the same
        mix[m++] = canon(t, b);
      }
      check_terms_of(t, mix, m);
    }
  }
}

// ---- (b) bind_scan_plan against the former function --------------------------------------------------------------------
static uint64_t column_bytes[kMaxCols][4];  // real buffers: the planner computes addresses inside them and never reads them
static uint8_t validity_bytes[kMaxCols][8];
static uint8_t ones_block[256];

static long bind_cells = 0, bind_bound = 0, gen_seen[8], key4_by_fixed = 0, key4_by_slots = 0;

static void check_bind_case(int n_cols, int kw, int na, bool fixed, bool key4_slots, int plan_mode, int np, int synth) {
  static const uint8_t types[7] = {T_I32, T_U32, T_F32, T_I64, T_U64, T_F64, T_I16};  // (Int16: a type no plan covers)
  static const int64_t bit_offsets[4] = {0, 3, 13, -1};
  DevProgram P;
  DevFastPlan F;
  DevColumns C;
  memset(&P, 0, sizeof(P));
  memset(&F, 0, sizeof(F));
  memset(&C, 0, sizeof(C));
  P.n_cols = n_cols;
  // the draws lean towards bindings that succeed (8-byte integers, aligned buffers), so that the success paths get their share
  const int narrow_key = below(3);  // 1: make the key a 4-byte integer and keep the rest wide (the key-4 flavour)
  for (int c = 0; c < n_cols; ++c) {
    P.col_dtype[c] = below(12) == 0 ? types[6] : below(3) == 0 ? types[below(6)] : types[below(2) ? 3 : 5];
    C.c[c].values = (const char*)column_bytes[c] + (below(8) == 0 ? 4 : 0);
    if (below(3) == 0) {
      C.c[c].validity = validity_bytes[c];
      C.c[c].bit_offset = bit_offsets[below(16) == 0 ? 3 : below(3)];
    }
  }
  for (int k = 0; k < kw; ++k) {
    F.keycol[k] = (uint8_t)below(n_cols);
    if (below(4) != 0 && P.col_dtype[F.keycol[k]] == T_F64) P.col_dtype[F.keycol[k]] = T_U64;
  }
  if (kw >= 1 && narrow_key == 1) {
    for (int c = 0; c < n_cols; ++c)
      if (P.col_dtype[c] == T_I32 || P.col_dtype[c] == T_U32 || P.col_dtype[c] == T_F32) P.col_dtype[c] = T_I64;
    P.col_dtype[F.keycol[0]] = below(2) ? T_I32 : T_U32;
  }
  uint8_t val_xform[kMaxAggs];
  memset(val_xform, 0, sizeof(val_xform));
  for (int a = 0; a < na; ++a) {
    F.arg[a].nf = below(24) == 0 ? 2 : 1;
    F.arg[a].f[0].kind = below(24) == 0 ? FF_COL_PLUS_IMM : FF_COL;
    F.arg[a].f[0].col = (uint8_t)(kw >= 1 && below(4) == 0 ? F.keycol[0] : below(n_cols));  // (key == argument: its own draw)
    val_xform[a] = below(2) ? VT_COUNT_VALID : VT_RAW;
  }
  F.valid = below(24) == 0 ? 0 : 1;
  F.plan_mode = plan_mode | (below(2) ? 4 : 0);
  F.np = np;
  F.synth = synth;
  for (int i = 0; i < np && i < 4; ++i) {
    static const uint8_t masks[5] = {1, 2, 3, 4, 6};
    F.term[i].col = (uint8_t)below(n_cols);
    F.term[i].dtype = P.col_dtype[F.term[i].col];
    F.term[i].m = masks[below(5)];
    F.term[i].inv = F.term[i].m == 2 ? (uint8_t)below(2) : 0;
    F.term_imm[i] = below(4) == 0 ? f64_bits(below(2) ? 0.0 : __builtin_nan("")) : rnd();
  }
  const uint8_t* ones = below(40) == 0 ? nullptr : ones_block;

  DevFastPlan Fa, Fb;
  DevColumns Ca, Cb;
  memset(&Fa, 0, sizeof(Fa));
  memset(&Fb, 0, sizeof(Fb));
  memset(&Ca, 0, sizeof(Ca));
  memset(&Cb, 0, sizeof(Cb));
  const bool was = former::former_bind_scan_plan(P, F, C, kw, na, val_xform, fixed, &Fa, &Ca, key4_slots, ones);
  const bool now = bind_scan_plan(P, F, C, kw, na, val_xform, fixed, &Fb, &Cb, key4_slots, ones);
  long keep[S_COUNT_];  // (the shape check on its own, asked the same question: its hits are not counted twice)
  memcpy(keep, site_hits, sizeof(keep));
  const bool shape_was = former::former_scan_plan_shape_ok(P, F, kw, na, val_xform);
  memcpy(site_hits, keep, sizeof(keep));
  CHECK(scan_plan_shape_ok(P, F, kw, na, val_xform) == shape_was);
  CHECK(was == now);
  ++bind_cells;
  if (!was || !now) return;
  ++bind_bound;
  const bool same = memcmp(&Fa.scan, &Fb.scan, sizeof(Fa.scan)) == 0 && memcmp(&Ca, &Cb, sizeof(Ca)) == 0;
  if (!same && failures < 40)
    printf("bind: n_cols %d kw %d na %d fixed %d key4_slots %d plan_mode %d np %d synth %d: gen %d / %d, n_cols %d / %d\n", n_cols, kw, na,
           (int)fixed, (int)key4_slots, plan_mode, np, synth, Fa.scan.gen, Fb.scan.gen, Fa.scan.n_cols, Fb.scan.n_cols);
  CHECK(same);
  CHECK(memcmp(&Fa, &Fb, sizeof(Fa)) == 0);  // (and the copy of the decoded shape around the plan)
  if (Fa.scan.gen >= 0 && Fa.scan.gen < 8) ++gen_seen[Fa.scan.gen];
  if (Fa.scan.gen & 4) ++(fixed ? key4_by_fixed : key4_by_slots);
}

static void check_bind() {
  memset(ones_block, 0xFF, sizeof(ones_block));
  // the small axes exhaustively, the others (types, validity, bit offsets, alignment, which columns, transforms, literals,
  // F.valid, the ones block) drawn kDraws times per point
  const int kDraws = 16;
  for (int n_cols = 1; n_cols <= 5; ++n_cols)
    for (int kw = 0; kw <= 2; ++kw)
      for (int na = 0; na <= 2; ++na)
        for (int fixed = 0; fixed <= 1; ++fixed)
          for (int key4_slots = 0; key4_slots <= 1; ++key4_slots)
            for (int plan_mode = 0; plan_mode <= 2; ++plan_mode)
              for (int np = 0; np <= 5; ++np)
                for (int synth = 0; synth <= 2; ++synth) {
                  // five terms of which one is dropped: the former function reads DevFastPlan::term[4], past the array, before
                  // it can refuse (fast_terms never builds more than four): left out, by name
                  if (np == 5 && synth != 0) continue;
                  for (int d = 0; d < kDraws; ++d) check_bind_case(n_cols, kw, na, fixed != 0, key4_slots != 0, plan_mode, np, synth);
                }
  for (int s = 0; s < S_COUNT_; ++s) {
    // too_many_slots cannot be reached: the slots are the program's columns, plus one when a fixed binding's key is also its
    // argument -- and that shape passes the shape check with at most kPlanCols - 1 columns (key_is_arg_and_full)
    if (s == S_TOO_MANY_SLOTS) CHECK(site_hits[s] == 0);
    else CHECK(site_hits[s] > 0);
  }
  for (int g : {0, 1, 2, 3, 4, 6}) CHECK(gen_seen[g] > 0);
  CHECK(gen_seen[5] == 0 && gen_seen[7] == 0);  // bit 2 stands INSTEAD of bit 0
  CHECK(key4_by_fixed > 0 && key4_by_slots > 0);
  CHECK(bind_cells >= 100000);
}

// ---- (c) the recogniser against the former one -------------------------------------------------------------------------
struct Builder {
  DevProgram P;
  Builder() { memset(&P, 0, sizeof(P)); }
  uint8_t col(uint8_t dtype) {
    P.col_dtype[P.n_cols] = dtype;
    return make_operand(OPK_COL, P.n_cols++);
  }
  uint8_t imm(uint64_t bits) {
    P.imm[P.n_imm] = bits;
    return make_operand(OPK_IMM, P.n_imm++);
  }
  uint8_t ins(uint8_t op, uint8_t t, uint8_t a, uint8_t b) {
    P.ins[P.n_ins] = DevIns{op, t, a, b};
    return make_operand(OPK_REG, P.n_ins++);
  }
};

static long fast_cells = 0, fast_valid = 0, fast_refused = 0, fast_synth[3];

static void check_fast(const DevProgram& P, uint8_t pred, const uint8_t* keys, int kw, const uint8_t* args, int na, int want_valid) {
  DevFastPlan Fa, Fb;
  memset(&Fa, 0x5A, sizeof(Fa));  // (both functions clear the whole plan themselves)
  memset(&Fb, 0xA5, sizeof(Fb));
  former::build_fast(P, pred, keys, kw, args, na, &Fa);
  build_fast_plan(P, pred, keys, kw, args, na, &Fb);
  CHECK(memcmp(&Fa, &Fb, sizeof(Fa)) == 0);
  if (want_valid >= 0) CHECK(Fa.valid == want_valid);
  ++fast_cells;
  ++(Fa.valid ? fast_valid : fast_refused);
  if (Fa.synth >= 0 && Fa.synth <= 2) ++fast_synth[Fa.synth];
}

static void check_recogniser() {
  static const uint8_t cmp_types[6] = {T_I32, T_U32, T_F32, T_I64, T_U64, T_F64};
  // conjunctions of 0..5 terms (5 refuses), the literal on either side, every operator
  for (int nt = 0; nt <= 5; ++nt)
    for (int op0 = DOP_EQ; op0 <= DOP_GE; ++op0)
      for (int side0 = 0; side0 <= 1; ++side0)
        for (int draw = 0; draw < 6; ++draw) {
          Builder B;
          const int n_cols = 1 + below(4);
          uint8_t cols[4];
          for (int c = 0; c < n_cols; ++c) cols[c] = B.col(cmp_types[below(6)]);
          uint8_t pred = kNoOperand;
          for (int i = 0; i < nt; ++i) {
            const uint8_t c = cols[below(n_cols)], lit = B.imm(rnd());
            const int op = i == 0 ? op0 : DOP_EQ + below(6);
            const bool lit_left = i == 0 ? side0 != 0 : below(2) != 0;
            const uint8_t term = B.ins((uint8_t)op, B.P.col_dtype[c & 63], lit_left ? lit : c, lit_left ? c : lit);
            pred = i == 0 ? term : below(2) ? B.ins(DOP_AND, T_BOOL, pred, term) : B.ins(DOP_AND, T_BOOL, term, pred);  // (either nesting)
          }
          const uint8_t key = make_operand(OPK_COL, below(n_cols)), arg = make_operand(OPK_COL, below(n_cols));
          check_fast(B.P, pred, &key, 1, &arg, 1, nt <= 4 ? 1 : 0);
        }
  // something that is not a term under the conjunction: an OR, a comparison of two columns, of a computed value
  {
    Builder B;
    const uint8_t c0 = B.col(T_F64), c1 = B.col(T_F64), l = B.imm(f64_bits(1.5));
    const uint8_t t0 = B.ins(DOP_LT, T_F64, c0, l), t1 = B.ins(DOP_GT, T_F64, c1, l);
    check_fast(B.P, B.ins(DOP_OR, T_BOOL, t0, t1), nullptr, 0, nullptr, 0, 0);
    check_fast(B.P, B.ins(DOP_LT, T_F64, c0, c1), nullptr, 0, nullptr, 0, 0);
    check_fast(B.P, B.ins(DOP_LT, T_F64, B.ins(DOP_ADD, T_F64, c0, l), l), nullptr, 0, nullptr, 0, 0);
    check_fast(B.P, c0, nullptr, 0, nullptr, 0, 0);  // (a bare column as the predicate)
  }
  // arguments: a plain column of any type; col + imm, imm + col, col - imm, imm - col, col * imm, imm * col; left-nested products of
  // 1..4 factors (4 refuses); a factor that is not Float64 (refuses); a key that is not a column (valid stays 0)
  for (uint8_t t = T_BOOL; t <= T_UTF8; ++t) {
    Builder B;
    const uint8_t k = B.col(T_I64), a = B.col(t);
    check_fast(B.P, kNoOperand, &k, 1, &a, 1, 1);
  }
  for (int nf = 1; nf <= 4; ++nf)
    for (int draw = 0; draw < 200; ++draw) {
      Builder B;
      const uint8_t k = B.col(T_I64);
      const int bad = draw % 8 == 7 ? below(nf) : -1;  // this factor is an Int64 one
      uint8_t prod = 0;
      for (int f = 0; f < nf; ++f) {
        const uint8_t t = f == bad ? T_I64 : T_F64;
        const uint8_t c = B.col(t);
        uint8_t fac = c;
        const int form = below(7);
        if (form > 0) {
          const uint8_t l = B.imm(rnd());
          const uint8_t op = form <= 2 ? DOP_ADD : form <= 4 ? DOP_SUB : DOP_MUL;
          fac = (form & 1) ? B.ins(op, t, c, l) : B.ins(op, t, l, c);
        }
        prod = f == 0 ? fac : B.ins(DOP_MUL, T_F64, prod, fac);
      }
      // (a lone Int64 column IS an argument -- "plain column of any type" -- unless it is a factor of a product)
      const bool plain_col = nf == 1 && (prod >> 6) == OPK_COL;
      check_fast(B.P, kNoOperand, &k, 1, &prod, 1, nf <= 3 && (bad < 0 || plain_col) ? 1 : 0);
      const uint8_t two[2] = {make_operand(OPK_COL, 1), prod};  // (behind a plain column as the first argument)
      check_fast(B.P, kNoOperand, &k, 1, two, 2, -1);
    }
  {
    Builder B;  // a right-nested product, a division, a key that is computed
    const uint8_t k = B.col(T_I64), x = B.col(T_F64), y = B.col(T_F64), z = B.col(T_F64), l = B.imm(f64_bits(2.0));
    const uint8_t right = B.ins(DOP_MUL, T_F64, x, B.ins(DOP_MUL, T_F64, y, z));
    check_fast(B.P, kNoOperand, &k, 1, &right, 1, 0);
    const uint8_t div = B.ins(DOP_DIV, T_F64, x, l);
    check_fast(B.P, kNoOperand, &k, 1, &div, 1, 0);
    const uint8_t computed_key = B.ins(DOP_ADD, T_I64, k, l);
    check_fast(B.P, kNoOperand, &computed_key, 1, &x, 1, 0);
    const uint8_t keys2[2] = {k, computed_key};
    check_fast(B.P, kNoOperand, keys2, 2, &x, 1, 0);
  }
  // the synthesised open side of a one-sided Float64 range: <, <=, >, >= with 1, 2 and 3 columns (3: none), the literal on either
  // side; and what gets none: Eq, NotEq, another type
  for (int n_cols = 1; n_cols <= 3; ++n_cols)
    for (int op = DOP_EQ; op <= DOP_GE; ++op)
      for (int lit_left = 0; lit_left <= 1; ++lit_left)
        for (uint8_t t : {T_F64, T_F32, T_I64}) {
          Builder B;
          uint8_t c = 0;
          for (int i = 0; i < n_cols; ++i) c = B.col(i == n_cols - 1 ? t : (uint8_t)T_F64);
          const uint8_t l = B.imm(f64_bits(204.8));
          const uint8_t pred = lit_left ? B.ins((uint8_t)op, t, l, c) : B.ins((uint8_t)op, t, c, l);
          DevFastPlan F;
          build_fast_plan(B.P, pred, nullptr, 0, nullptr, 0, &F);
          const bool ordered = op >= DOP_LT, wants = ordered && t == T_F64 && n_cols <= 2;
          const bool upper = (op == DOP_LT || op == DOP_LE) != (lit_left != 0);  // as the column sees it
          CHECK(F.valid == 1 && F.np == (wants ? 2 : 1) && F.synth == (wants ? (upper ? 1 : 2) : 0));
          check_fast(B.P, pred, nullptr, 0, nullptr, 0, 1);
        }
  CHECK(fast_valid > 0 && fast_refused > 0 && fast_synth[0] > 0 && fast_synth[1] > 0 && fast_synth[2] > 0);
}

int main() {
  check_terms();
  check_bind();
  check_recogniser();
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("ok: %ld cells (bind_scan_plan: %ld compared, %ld bound; terms: %ld; recogniser: %ld, %ld valid, %ld refused, synth 0/1/2 %ld/%ld/%ld)\n",
         bind_cells + term_cells + fast_cells, bind_cells, bind_bound, term_cells, fast_cells, fast_valid, fast_refused, fast_synth[0], fast_synth[1],
         fast_synth[2]);
  printf("refusal sites:");
  for (int s = 0; s < S_COUNT_; ++s) printf(" %s %ld", kSiteName[s], site_hits[s]);
  printf("\ngen:");
  for (int g = 0; g < 8; ++g) printf(" %d: %ld", g, gen_seen[g]);
  printf("\nkey-4 rule: through fixed %ld, through key4_slots %ld\n", key4_by_fixed, key4_by_slots);
  return 0;
}
