// dfx_k_interp_inl.hpp -- the per-row expression interpreter: the SSA register program of a DevProgram run for one row
// (load_columns, run_program, eval_predicate, fetch), and the two functions its loop calls out of line (cast_value_call,
// int_divide: every unit that includes this header emits a copy of them).
// Who includes it: dfx_k_policy_inl.hpp (InterpPolicy is this interpreter as a row source; the other policies share its column
// bank) and, through it, the scan kernels.  The units that scan no rows by a policy stay on dfx_k_base_inl.hpp.
#pragma once
#include "dfx_k_base_inl.hpp"

namespace dfx {

// cast_value out of line (the projection kernels inline cast_value; the interpreter's loop calls it)
__device__ __attribute__((noinline)) uint64_t cast_value_call(uint8_t from, uint8_t to, uint64_t v) { return cast_value(from, to, v); }

// integer Divide of the interpreter (arrow 0.12 array_ops::divide: DivideByZero; Rust's `/`: overflow panic).  Out of line: 64-bit
// integer division expands to ~150 instructions and a dozen live registers, which the interpreter's loop would carry in every path
struct IntDivResult {
  uint64_t value;
  uint32_t err;  // error bits to OR into the kernel's (returned by value: an `err` passed by reference would live in scratch memory)
};
__device__ __attribute__((noinline)) IntDivResult int_divide(uint8_t t, uint64_t x, uint64_t y, bool report) {
  IntDivResult r = {0, 0};
  if (y == 0) {
    if (report) r.err = 1u;
    return r;
  }
  if (is_signed_int(t)) {
    const uint64_t mn = wrap_to(t, 1ull << (t == T_I8 ? 7 : t == T_I16 ? 15 : t == T_I32 ? 31 : 63));
    if ((int64_t)y == -1 && x == mn) {
      if (report) r.err = 2u;
      r.value = x;
      return r;
    }
    r.value = (uint64_t)((int64_t)x / (int64_t)y);
    return r;
  }
  r.value = x / y;
  return r;
}

// ---------------------------------------------------------------------------------------------
// the per-row expression interpreter
// ---------------------------------------------------------------------------------------------
// NOTE: the register files are separate local vector VALUES (never members of a struct that is
// passed by reference): that is what lets SROA keep them in VGPRs and lower the wave-uniform
// dynamic indices to s_set_gpr_idx instead of scratch memory.
//
// Memory-level parallelism: a wave owns U consecutive 64-row groups per trip.  It first issues the
// column loads of ALL U groups (U x n_cols independent 512-byte requests in flight), then
// interprets the groups one after the other.  The column bank (values loaded per row) is sized to
// the program: BANK in {2,4,8} columns, U chosen so that BANK * U <= 16 values (32 VGPRs).
template <int BANK> struct Bank;
template <> struct Bank<2> { typedef u64x2 type; };
template <> struct Bank<4> { typedef u64x4 type; };
template <> struct Bank<8> { typedef u64x8 type; };

#define ROWSTATE_ARGS(s) s##_col, s##_reg, s##_colvalid, s##_regvalid
#define ROWSTATE_PARAMS COLV& s_col, u64x16& s_reg, uint32_t& s_colvalid, uint32_t& s_regvalid
#define ROWSTATE_CPARAMS const COLV& s_col, const u64x16& s_reg, const uint32_t& s_colvalid, const uint32_t& s_regvalid

// issue every column load of this row back to back (independent loads, all in flight together)
template <typename COLV>
DEV void load_columns(const DevProgram& P, const DevColumns& C, int64_t row, bool inb, COLV& s_col,
                      uint32_t& s_colvalid) {
  constexpr int BANK = (int)(sizeof(COLV) / 8);
  s_colvalid = 0xFFFFFFFFu;
  if (P.wide8) {  // wave-uniform.  8-byte columns without nulls: one unconditional load per bank slot (a slot past n_cols
                  // re-reads column 0 -- a cache hit), nothing between the loads, so all of them are in flight together.
                  // The dtype switch below waits for each load on its own (sub-word loads are widened at once): a
                  // wave then has ONE load in flight, and pass 1 of the partitioned GROUP BY ran at 1.7 TB/s.
#pragma unroll
    for (int c = 0; c < BANK; ++c) {
      const uint64_t* base = (const uint64_t*)C.c[c < P.n_cols ? c : 0].values;
      s_col[c] = __builtin_nontemporal_load(base + (inb ? row : 0));
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < BANK; ++c) {
    if (c < P.n_cols) {
      uint64_t v = 0;
      if (inb) v = load_canonical(P.col_dtype[c], C.c[c].values, row, C.c[c].bit_offset);
      s_col[c] = v;
      if (P.has_nulls) {  // wave-uniform branch
        if (C.c[c].validity != nullptr) {
          const bool ok = inb ? get_bit(C.c[c].validity, C.c[c].bit_offset + row) : false;
          if (!ok) s_colvalid &= ~(1u << c);
        }
      }
    }
  }
}

// (Round 5 also tried the program itself in vector registers -- lane j holding SSA instruction j and literal j, decoded with
// v_readlane instead of scalar loads from the kernel arguments: 1.74 ms per 2^27-row launch of the headline through the interpreter
// against 1.63 without; the three registers it takes push the ring kernel's allocation over its 128, and the scalar loads were not
// what the waves waited for.  profiles/r05_interpreter_counters.txt)
// NULLS == false: the batch's referenced columns carry no nulls (DevProgram::has_nulls, decided at bind time) -- every operand is
// valid, and `valid` is a compile-time constant for the code around the call
template <typename COLV, bool NULLS = true>
DEV void fetch(const DevProgram& P, ROWSTATE_CPARAMS, uint8_t opnd, uint64_t& v, bool& valid) {
  const int idx = opnd & 63;
  const int kind = opnd >> 6;
  if (kind == OPK_REG) {
    v = s_reg[idx];
    valid = NULLS ? ((s_regvalid >> idx) & 1) : true;
  } else if (kind == OPK_COL) {
    v = s_col[idx & (int)(sizeof(COLV) / 8 - 1)];
    valid = NULLS ? ((s_colvalid >> idx) & 1) : true;
  } else {
    v = P.imm[idx & (kMaxImm - 1)];
    valid = true;
  }
}

// Executes the SSA program for one row.  Semantics per op are arrow 0.12 array_ops, the same
// table the oracle restates (oracle/dfx_oracle.c: compare_arrays / boolean_arrays / math_arrays).
// NULLS == false (round 5): with every operand valid the per-lane validity booleans -- and the divergent control flow the compiler
// builds around `if (vx && vy)` for arrow's null rules, lane masks saved and restored per SSA instruction -- fold away.
template <typename COLV, bool NULLS>
DEV void run_program_impl(const DevProgram& P, ROWSTATE_PARAMS, bool active, uint32_t& err) {
  s_regvalid = NULLS ? 0u : 0xFFFFFFFFu;
  for (int pc = 0; pc < P.n_ins; ++pc) {
    const DevIns in = P.ins[pc];
    const uint8_t t = in.t;
    uint64_t x, y = 0;
    bool vx, vy = true;
    fetch<COLV, NULLS>(P, ROWSTATE_ARGS(s), in.a, x, vx);
    if (in.op != DOP_CAST) fetch<COLV, NULLS>(P, ROWSTATE_ARGS(s), in.b, y, vy);
    uint64_t res = 0;
    bool v = vx && vy;
    if (in.op <= DOP_GE) {
      bool lt, eq, gt;
      if (t == T_F64) {
        const double a = as_f64(x), b = as_f64(y);
        lt = a < b; eq = a == b; gt = a > b;
      } else if (t == T_F32) {
        const float a = as_f32(x), b = as_f32(y);
        lt = a < b; eq = a == b; gt = a > b;
      } else if (t == T_U64) {
        lt = x < y; eq = x == y; gt = x > y;
      } else {
        const int64_t a = (int64_t)x, b = (int64_t)y;
        lt = a < b; eq = a == b; gt = a > b;
      }
      bool r;
      if (vx && vy) {
        switch (in.op) {
          case DOP_EQ: r = eq; break;
          case DOP_NE: r = !eq; break;
          case DOP_LT: r = lt; break;
          case DOP_LE: r = lt || eq; break;
          case DOP_GT: r = gt; break;
          default: r = gt || eq; break;
        }
      } else {  // arrow 0.12 bool_op over Option<T>: never null; None sorts below every value
        switch (in.op) {
          case DOP_EQ: r = (!vx && !vy); break;
          case DOP_NE: r = (vx != vy); break;
          case DOP_LT: r = (!vx && vy); break;
          case DOP_LE: r = !vx; break;
          case DOP_GT: r = (vx && !vy); break;
          default: r = !vy; break;
        }
      }
      res = r ? 1 : 0;
      v = true;
    } else if (in.op == DOP_AND) {
      res = x & y & 1;
    } else if (in.op == DOP_OR) {
      res = (x | y) & 1;
    } else if (in.op == DOP_CAST) {
      res = cast_value_call(t, in.b, x);
      v = vx;
    } else if (t == T_F64) {
      const double a = as_f64(x), b = as_f64(y);
      double o;
      switch (in.op) {
        case DOP_ADD: o = a + b; break;
        case DOP_SUB: o = a - b; break;
        case DOP_MUL: o = a * b; break;
        default:
          if (v && active && b == 0.0) err |= 1u;
          o = a / b;
          break;
      }
      res = f64_bits(o);
    } else if (t == T_F32) {
      const float a = as_f32(x), b = as_f32(y);
      float o;
      switch (in.op) {
        case DOP_ADD: o = a + b; break;
        case DOP_SUB: o = a - b; break;
        case DOP_MUL: o = a * b; break;
        default:
          if (v && active && b == 0.0f) err |= 1u;
          o = a / b;
          break;
      }
      res = f32_bits(o);
    } else {
      uint64_t o;
      switch (in.op) {
        case DOP_ADD: o = x + y; break;
        case DOP_SUB: o = x - y; break;
        case DOP_MUL: o = x * y; break;
        default: {
          const IntDivResult dr = int_divide(t, x, y, v && active);
          o = dr.value;
          err |= dr.err;
          break;
        }
      }
      res = wrap_to(t, o);
    }
    // a null result slot holds zero: arrow 0.12's builders append_null() over zero-initialised buffers, and the grouped
    // aggregates read value(row) of their argument WITHOUT a null check (aggregate.rs:561-603), so the slot's content
    // is observable (MAX(x + x) over a null x sees 0, not raw + raw)
    s_reg[pc] = (!NULLS || v) ? res : 0ull;
    if (NULLS) s_regvalid |= (v ? 1u : 0u) << pc;
  }
}

template <typename COLV>
DEV void run_program(const DevProgram& P, ROWSTATE_PARAMS, bool active, uint32_t& err) {
  if (P.has_nulls) run_program_impl<COLV, true>(P, ROWSTATE_ARGS(s), active, err);  // (wave-uniform: a property of the batch)
  else run_program_impl<COLV, false>(P, ROWSTATE_ARGS(s), active, err);
}

template <typename COLV>
DEV bool eval_predicate(const DevProgram& P, ROWSTATE_CPARAMS, uint8_t pred) {
  if (pred == kNoOperand) return true;
  uint64_t v;
  bool valid;
  fetch(P, ROWSTATE_ARGS(s), pred, v, valid);
  // FilterRelation reads filter.value(i): the raw value bit; a null slot holds false (filter.rs:86)
  return valid && (v & 1);
}

}  // namespace dfx
