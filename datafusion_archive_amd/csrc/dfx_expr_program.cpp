// dfx_expr_program.cpp -- ProgramBuilder: lowers validated Expr trees (dfx_expr.cpp) to the fused device program
// (dfx_device.hpp: DevProgram), with common-subexpression elimination, and binds a batch's buffers to it.  What the kernels read
// besides the program -- the decoded shape and the scan plan -- is built in dfx_scan_plan.hpp (HIP-free, checked on the CPU):
// build_fast, scan_plan_shape_ok, bind_scan_plan and dfx_debug_plan_term here are that header's entry points into the library.
#include <string.h>

#include "dfx_host.hpp"
#include "dfx_kernels.hpp"
#include "dfx_scan_plan.hpp"

namespace dfx {

ProgramBuilder::ProgramBuilder(const SchemaInfo& schema) : schema_(schema) {
  memset(&prog_, 0, sizeof(prog_));
}

Status ProgramBuilder::add(const dfx_runtime_expr& e, int32_t root, uint8_t* operand, int* dtype) {
  return emit(e, root, operand, dtype);
}

Status ProgramBuilder::emit(const dfx_runtime_expr& e, int32_t idx, uint8_t* operand, int* dtype) {
  const dfx_expr_node& n = e.nodes[idx];
  switch (n.kind) {
    case DFX_EXPR_COLUMN: {
      const int dt = schema_.fields[n.column].dtype;
      if (dt == DFX_UTF8)
        return Status::Err(DFX_NOT_IMPLEMENTED, "Utf8 columns cannot be used in device expressions");
      int slot = -1;
      for (size_t i = 0; i < cols_.size(); ++i)
        if (cols_[i] == n.column) slot = (int)i;
      if (slot < 0) {
        if ((int)cols_.size() >= kMaxCols)
          return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("fused expression reads more than %d columns", kMaxCols));
        slot = (int)cols_.size();
        cols_.push_back(n.column);
        prog_.col_dtype[slot] = (uint8_t)dt;
        prog_.n_cols = (int32_t)cols_.size();
      }
      *operand = make_operand(OPK_COL, slot);
      *dtype = dt;
      return Status::OK();
    }
    case DFX_EXPR_LITERAL: {
      uint64_t bits = 0;
      switch (n.dtype) {
        case DFX_FLOAT64: memcpy(&bits, &n.lit.f64, 8); break;
        case DFX_FLOAT32: { uint32_t b; memcpy(&b, &n.lit.f32, 4); bits = b; break; }
        case DFX_INT8: case DFX_INT16: case DFX_INT32: case DFX_INT64: bits = (uint64_t)n.lit.i64; break;
        default: bits = n.lit.u64; break;
      }
      int slot = -1;
      for (int i = 0; i < prog_.n_imm; ++i)
        if (prog_.imm[i] == bits) slot = i;
      if (slot < 0) {
        if (prog_.n_imm >= kMaxImm)
          return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("fused expression uses more than %d literals", kMaxImm));
        slot = prog_.n_imm++;
        prog_.imm[slot] = bits;
      }
      *operand = make_operand(OPK_IMM, slot);
      *dtype = n.dtype;
      return Status::OK();
    }
    case DFX_EXPR_CAST:
    case DFX_EXPR_BINARY: {
      DevIns ins;
      memset(&ins, 0, sizeof(ins));
      uint8_t a = 0, b = 0;
      int ta = 0, tb = 0;
      DFX_RETURN_IF_ERROR(emit(e, n.left, &a, &ta));
      if (n.kind == DFX_EXPR_CAST) {
        // `as` to the same type is the identity -- for a computed value or a literal.  A COLUMN keeps its instruction:
        // cast_column! builds a NEW array (expression.rs:246-270), whose null slots hold zero, and the grouped aggregates
        // read value(row) of their argument without a null check (aggregate.rs:561-603), so MAX(CAST(c AS its own type))
        // over a null slot sees 0, not the column's raw content (found by tests/test_gpu_fuzz.py)
        if (ta == n.dtype && (a >> 6) != OPK_COL) {
          *operand = a;
          *dtype = ta;
          return Status::OK();
        }
        if ((a >> 6) == OPK_IMM) {  // CAST(literal): folded at compile time (no per-row work at all)
          const uint64_t bits = host_cast_value(ta, n.dtype, prog_.imm[a & 63]);
          int slot = -1;
          for (int i = 0; i < prog_.n_imm; ++i)
            if (prog_.imm[i] == bits) slot = i;
          if (slot < 0) {
            if (prog_.n_imm >= kMaxImm)
              return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("fused expression uses more than %d literals", kMaxImm));
            slot = prog_.n_imm++;
            prog_.imm[slot] = bits;
          }
          *operand = make_operand(OPK_IMM, slot);
          *dtype = n.dtype;
          return Status::OK();
        }
        ins.op = DOP_CAST;
        ins.t = (uint8_t)ta;
        ins.a = a;
        ins.b = (uint8_t)n.dtype;
        *dtype = n.dtype;
      } else {
        DFX_RETURN_IF_ERROR(emit(e, n.right, &b, &tb));
        if (n.op == DFX_OP_AND || n.op == DFX_OP_OR) {
          if (ta != DFX_BOOLEAN || tb != DFX_BOOLEAN)  // downcast_ref::<BooleanArray>().unwrap() (expression.rs:217-221)
            return Status::Err(DFX_INTERNAL_ERROR, "called `Option::unwrap()` on a `None` value (boolean_ops operand is not a BooleanArray)");
          ins.op = n.op == DFX_OP_AND ? DOP_AND : DOP_OR;
          *dtype = DFX_BOOLEAN;
        } else if (n.op <= DFX_OP_GT_EQ) {
          if (ta != tb || !dtype_is_numeric(ta))  // expression.rs:207
            return Status::Err(DFX_EXECUTION_ERROR, "comparison_ops");
          ins.op = (uint8_t)n.op;
          *dtype = DFX_BOOLEAN;
        } else {
          if (ta != tb || !dtype_is_numeric(ta))  // expression.rs:166
            return Status::Err(DFX_EXECUTION_ERROR, "math_ops");
          ins.op = (uint8_t)(DOP_ADD + (n.op - DFX_OP_PLUS));
          *dtype = ta;
        }
        ins.t = (uint8_t)ta;
        ins.a = a;
        ins.b = b;
      }
      for (int i = 0; i < prog_.n_ins; ++i) {  // common subexpression: identical instruction
        const DevIns& o = prog_.ins[i];
        if (o.op == ins.op && o.t == ins.t && o.a == ins.a && o.b == ins.b) {
          *operand = make_operand(OPK_REG, i);
          return Status::OK();
        }
      }
      if (prog_.n_ins >= kMaxRegs)
        return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("fused expression needs more than %d computed values", kMaxRegs));
      prog_.ins[prog_.n_ins] = ins;
      *operand = make_operand(OPK_REG, prog_.n_ins);
      prog_.n_ins++;
      return Status::OK();
    }
    default:
      return Status::Err(DFX_EXECUTION_ERROR, "expression " + expr_debug(e.nodes, idx));
  }
}

Status ProgramBuilder::bind(const DeviceBatch& batch, DevProgram* prog, DevColumns* cols) const {
  *prog = prog_;
  memset(cols, 0, sizeof(*cols));
  prog->has_nulls = 0;
  prog->wide8 = 0;
  for (size_t i = 0; i < cols_.size(); ++i) {
    const int ci = cols_[i];
    if (ci >= (int)batch.columns.size())
      return Status::Err(DFX_INTERNAL_ERROR, strfmt("batch has %zu columns, expression reads column %d", batch.columns.size(), ci));
    const DeviceColumn& c = batch.columns[ci];
    if (c.dtype != prog_.col_dtype[i])  // downcast_ref::<T>() of a column whose array has another type
      return Status::Err(DFX_INTERNAL_ERROR, strfmt("Column at index %d is not of expected type", ci));
    cols->c[i].values = c.values;
    cols->c[i].validity = c.null_count != 0 ? c.validity : nullptr;
    cols->c[i].bit_offset = c.bit_offset;
    if (cols->c[i].validity) prog->has_nulls = 1;
  }
  prog->wide8 = !prog->has_nulls && !cols_.empty();
  for (size_t i = 0; i < cols_.size(); ++i) {
    const uint8_t t = prog_.col_dtype[i];
    if (t != T_I64 && t != T_U64 && t != T_F64) prog->wide8 = 0;
  }
  return Status::OK();
}

// ---- dfx_scan_plan.hpp's entry points ----
static_assert(T_F64 == DFX_FLOAT64, "the header names dtypes by dfx_device.hpp's codes, the trees by include/dfx.h's");
void ProgramBuilder::build_fast(uint8_t pred, const uint8_t* keys, int kw, const uint8_t* args, int na, DevFastPlan* F) const {
  host_plan::build_fast_plan(prog_, pred, keys, kw, args, na, F);
}

bool scan_plan_shape_ok(const DevProgram& P, const DevFastPlan& F, int kw, int na, const uint8_t* val_xform) {
  return host_plan::scan_plan_shape_ok(P, F, kw, na, val_xform);
}

bool bind_scan_plan(const DevProgram& P, const DevFastPlan& F, const DevColumns& C, int kw, int na, const uint8_t* val_xform,
                    bool fixed, DevFastPlan* Fout, DevColumns* Cout, bool key4_slots) {
  return host_plan::bind_scan_plan(P, F, C, kw, na, val_xform, fixed, Fout, Cout, key4_slots, device_ones_block());
}

}  // namespace dfx

// one term on the host: the planner's range and the kernels' test of a value against it (include/dfx.h)
extern "C" int32_t dfx_debug_plan_term(int32_t dtype, int32_t op, uint64_t literal, uint64_t value, int32_t is_null) {
  using namespace dfx;
  if (op < 0 || op > 5) return -1;
  const uint8_t t = (uint8_t)dtype;
  if (t != T_I32 && t != T_U32 && t != T_F32 && t != T_I64 && t != T_U64 && t != T_F64) return -1;
  static const uint8_t three_way[6] = {2, 2, 1, 3, 4, 6};  // Eq NotEq Lt LtEq Gt GtEq (fast_terms)
  DevPlanTerm T;
  memset(&T, 0, sizeof(T));
  host_plan::plan_term_range(t, three_way[op], op == DFX_OP_NOT_EQ, literal, &T);
  if (is_null) return (int32_t)T.if_null;
  uint64_t x = value;  // what PlanPolicy::eval leaves in the row's register: the value widened to 64 bits
  if (t == T_F32) {
    float f;
    const uint32_t b32 = (uint32_t)value;
    memcpy(&f, &b32, 4);
    const double d = (double)f;
    memcpy(&x, &d, 8);
  }
  return host_plan::plan_term_passes(T, x) ? 1 : 0;
}
