// dfx_expr.cpp -- the expression compiler.
//   dfx_compile_scalar_expr  <->  compile_scalar_expr (src/execution/expression.rs:283-505)
//   dfx_compile_expr         <->  compile_expr        (src/execution/expression.rs:80-121)
//   The fused device program these trees are lowered to: dfx_expr_program.cpp (ProgramBuilder), dfx_scan_plan.hpp (what the
//   kernels read besides it); the Utf8 string terms of D9: dfx_expr_utf8.cpp.
//
// Deviations from the reference (each is a place where the reference panics / is unimplemented):
//   D1  numeric->numeric CAST of any scalar expression is implemented (Rust `as`); the reference
//       implements column->Int16/Int32 and literal Int64->Float64 only (expression.rs:272-280,
//       :345-368), `unimplemented!()` / NotImplemented / General otherwise.
//   D8  COUNT_DISTINCT (AggregateType::CountDistinct, expression.rs:37, has no executor in the reference): the number of
//       distinct non-null argument values, UInt64; -0.0 and +0.0 are one value, every NaN payload is one value; never null
//       when grouped (0 for a group of null arguments), ungrouped over nothing counted what COUNT(x) gives (dfx_distinct.cpp).
//   D6  RuntimeExpr type of a column cast is the TARGET type; the reference reports the source
//       column's type (expression.rs:324, a bug: the array it builds has the target type).
//   D9  Utf8 string terms (the planner's own example, `#4 Eq Utf8("CO")`, sqlplanner.rs:570, and Operator::Like / NotLike, :277-278, have no
//       evaluator in the reference: the literal is rejected, expression.rs:306-309): a BinaryExpr of a bare Utf8 column and a Utf8 literal,
//       Eq NotEq Lt LtEq Gt GtEq with the literal on either side (a literal on the left mirrors the operator) or column LIKE / NOT LIKE
//       pattern; type Boolean, name the Debug form.  Ordering is Rust `str` ordering (unsigned byte-wise lexicographic, a proper prefix
//       first), equality is byte equality (no collation, case folding or normalisation).  LIKE: `%` any run of bytes (also none), `_`
//       exactly one UTF-8 encoded character (lead byte + continuation bytes), no escape character, anchored at both ends, a pattern
//       without wildcards is Eq, NOT LIKE the complement on non-null rows.  Nulls follow arrow 0.12 bool_op over Option<T> (the literal
//       is always valid, the result never null): a null slot gives Eq false, NotEq true, Lt / LtEq true, Gt / GtEq false, and by analogy
//       with Eq / NotEq Like false, NotLike true (recalled, unpinned).  A literal or pattern of more than 4096 bytes: NotImplemented at
//       compile time.  Anything else with a Utf8 literal, Like on other operands, Utf8 column against Utf8 column: refused as before.
//   D10 MIN / MAX of a Utf8 column (typed by the planner like any aggregate, sqlplanner.rs:309-322: the return type is the argument's;
//       the executor panics on the downcast, aggregate.rs:561-603): the argument a bare Utf8 column, the result a nullable Utf8 column
//       named like the aggregate.  Order is Rust `str` Ord, D9's (the empty string is a value and the smallest).  Null arguments are
//       skipped, grouped and ungrouped; a group whose arguments are all null reports NULL, ungrouped over no non-null row one row holding
//       NULL, grouped over empty input zero rows.  (Over a Filter no argument is null: fn filter's output is all-valid, filter.rs:83-92, so
//       a null slot that passes the predicate is the value its bytes spell, the empty string for an Arrow-built null.)  Another declared return type: the InternalError of a numeric mismatch; more GROUP BY
//       expressions than COUNT_DISTINCT takes: NotImplemented; both at creation (dfx_distinct.cpp folds the extrema from the distinct
//       set of the argument at emit, dfx_k_utf8agg.hip).  Parity unpinned.
//   D12 The Parquet data source (declared three times, executed nowhere: FileType::Parquet / `STORED AS PARQUET`, dfparser.rs:31-36,
//       :177-178; DataSourceMeta::ParquetFile { filename, schema, projection }, datasource.rs:87-92; LogicalPlan::ParquetFile in the
//       push-down rule, sqlplanner.rs:525-532): dfx_parquet_datasource_new (dfx_parquet.cpp) serves the file's own schema, flat
//       required / optional leaves of BOOLEAN, INT32 / INT64 with their Int annotations, FLOAT, DOUBLE and String byte arrays, from
//       UNCOMPRESSED or LZ4_RAW chunks of dictionary, V1 and V2 pages in PLAIN, RLE_DICTIONARY and RLE; anything else is NotImplemented at
//       construction.  Parity unpinned; the contract is pyarrow's reader.
//   D13 The Parquet sink (PhysicalPlan::Write { plan, filename, kind }, physicalplan.rs:24-29, with kind = FileType::Parquet,
//       dfparser.rs:31-36: declared, never run): dfx_parquet_write (dfx_parquet_write.cpp) writes a flat schema of the twelve types in
//       UNCOMPRESSED chunks of V1 PLAIN pages whose bodies are encoded on the device (dfx_k_parquet_write.hip); any other column
//       type is NotImplemented before a file exists.  Parity unpinned; the contract: pyarrow and dfx_parquet_datasource_new read back
//       the table that went in, bit for bit.
#include <charconv>
#include <string.h>
#include <strings.h>

#include "dfx_host.hpp"
#include "dfx_kernels.hpp"

namespace dfx {

const char* op_debug(int op) {  // Rust {:?} of logicalplan::Operator
  static const char* names[] = {"Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq", "Plus", "Minus", "Multiply",
                                "Divide", "Modulus", "And", "Or", "Not", "Like", "NotLike"};
  return (op >= 0 && op <= DFX_OP_NOT_LIKE) ? names[op] : "?";
}

namespace {
std::string float_repr(double v, bool debug) {
  if (v != v) return "NaN";
  if (v == __builtin_inf()) return "inf";
  if (v == -__builtin_inf()) return "-inf";
  char buf[512];
  auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
  std::string s(buf, r.ptr);
  if (debug && s.find('.') == std::string::npos) s += ".0";
  return s;
}

std::string float_repr32(float v, bool debug) {
  if (v != v) return "NaN";
  char buf[256];
  auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
  std::string s(buf, r.ptr);
  if (debug && s.find('.') == std::string::npos) s += ".0";
  return s;
}

std::string literal_repr(const dfx_expr_node& n, bool debug) {  // Display (debug=false) or Debug of the ScalarValue
  std::string v;
  switch (n.dtype) {
    case DFX_FLOAT64: v = float_repr(n.lit.f64, debug); break;
    case DFX_FLOAT32: v = float_repr32(n.lit.f32, debug); break;
    case DFX_INT8: case DFX_INT16: case DFX_INT32: case DFX_INT64: v = std::to_string((long long)n.lit.i64); break;
    case DFX_UINT8: case DFX_UINT16: case DFX_UINT32: case DFX_UINT64: v = std::to_string((unsigned long long)n.lit.u64); break;
    case DFX_BOOLEAN: v = n.lit.u64 ? "true" : "false"; break;
    case DFX_UTF8: v = std::string("\"") + (n.name ? n.name : "") + "\""; break;
    default: return "Null";
  }
  if (!debug) return v;
  return std::string(dtype_name(n.dtype)) + "(" + v + ")";
}
}  // namespace

std::string expr_debug(const std::vector<dfx_expr_node>& nodes, int32_t idx) {  // logicalplan.rs:264-309
  if (idx < 0 || idx >= (int32_t)nodes.size()) return "?";
  const dfx_expr_node& n = nodes[idx];
  switch (n.kind) {
    case DFX_EXPR_COLUMN: return "#" + std::to_string(n.column);
    case DFX_EXPR_LITERAL: return literal_repr(n, true);
    case DFX_EXPR_CAST: return "CAST(" + expr_debug(nodes, n.left) + " AS " + dtype_name(n.dtype) + ")";
    case DFX_EXPR_IS_NULL: return expr_debug(nodes, n.left) + " IS NULL";
    case DFX_EXPR_IS_NOT_NULL: return expr_debug(nodes, n.left) + " IS NOT NULL";
    case DFX_EXPR_BINARY:
      return expr_debug(nodes, n.left) + " " + op_debug(n.op) + " " + expr_debug(nodes, n.right);
    case DFX_EXPR_SORT: return expr_debug(nodes, n.left) + (n.reserved ? " DESC" : " ASC");
    case DFX_EXPR_SCALAR_FUNCTION:
    case DFX_EXPR_AGGREGATE_FUNCTION:
      return std::string(n.name ? n.name : "") + "(" + (n.left >= 0 ? expr_debug(nodes, n.left) : "") + ")";
    default: return "?";
  }
}

namespace {
// static result type of a scalar node (the type of the array the closure would produce)
Status node_type(const std::vector<dfx_expr_node>& nodes, int32_t idx, const SchemaInfo& schema, int* out) {
  const dfx_expr_node& n = nodes[idx];
  switch (n.kind) {
    case DFX_EXPR_COLUMN: *out = schema.fields[n.column].dtype; return Status::OK();
    case DFX_EXPR_LITERAL: *out = n.dtype; return Status::OK();
    case DFX_EXPR_CAST: *out = n.dtype; return Status::OK();
    case DFX_EXPR_BINARY:
      if (n.op <= DFX_OP_GT_EQ || n.op == DFX_OP_AND || n.op == DFX_OP_OR || utf8_string_term(nodes, idx, schema, nullptr)) {
        *out = DFX_BOOLEAN;  // (deviation D9: a LIKE string term is Boolean too)
        return Status::OK();
      }
      return node_type(nodes, n.left, schema, out);  // op_type = left_expr.get_type() (expression.rs:408)
    default: *out = DFX_TYPE_NONE; return Status::OK();
  }
}

// compile_scalar_expr's validation (errors mirror expression.rs:283-505); fills the display name
Status validate_scalar(const std::vector<dfx_expr_node>& nodes, int32_t idx, const SchemaInfo& schema,
                       std::string* name, int depth = 0) {
  if (idx < 0 || idx >= (int32_t)nodes.size() || depth > 64)
    return Status::Err(DFX_INTERNAL_ERROR, strfmt("expression node index %d out of range", idx));
  const dfx_expr_node& n = nodes[idx];
  switch (n.kind) {
    case DFX_EXPR_LITERAL:
      if (!dtype_is_numeric(n.dtype))  // expression.rs:306-309
        return Status::Err(DFX_EXECUTION_ERROR, "No support for literal type " + literal_repr(n, true));
      if (name) *name = literal_repr(n, false);  // format!("{}", nn)
      return Status::OK();
    case DFX_EXPR_COLUMN:
      if (n.column < 0 || n.column >= (int32_t)schema.fields.size())  // schema.field(index) panics
        return Status::Err(DFX_INTERNAL_ERROR, strfmt("index out of bounds: column %d of a schema with %zu fields",
                                                      n.column, schema.fields.size()));
      if (name) *name = schema.fields[n.column].name;
      return Status::OK();
    case DFX_EXPR_CAST: {
      std::string child_name;
      DFX_RETURN_IF_ERROR(validate_scalar(nodes, n.left, schema, &child_name, depth + 1));
      int from = DFX_TYPE_NONE;
      DFX_RETURN_IF_ERROR(node_type(nodes, n.left, schema, &from));
      const dfx_expr_node& c = nodes[n.left];
      if (!dtype_is_numeric(from))  // expression.rs:336 panic!("unsupported CAST operation")
        return Status::Err(DFX_INTERNAL_ERROR, "unsupported CAST operation");
      if (!dtype_is_numeric(n.dtype))  // unimplemented!() (:277) / NotImplemented (:363-372)
        return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("CAST from %s to %s", dtype_name(from), dtype_name(n.dtype)));
      if (name) *name = c.kind == DFX_EXPR_COLUMN ? child_name : (c.kind == DFX_EXPR_LITERAL ? "lit" : "cast");
      return Status::OK();
    }
    case DFX_EXPR_BINARY: {
      if (utf8_string_term(nodes, idx, schema, nullptr)) {  // deviation D9: here, and only here, a Utf8 literal is an operand
        const dfx_expr_node& l = nodes[n.left].kind == DFX_EXPR_LITERAL ? nodes[n.left] : nodes[n.right];
        if (strlen(l.name ? l.name : "") > kUtf8MaxLiteral)
          return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("Utf8 literal of more than %u bytes in a string term", kUtf8MaxLiteral));
        if (name) *name = expr_debug(nodes, idx);
        return Status::OK();
      }
      DFX_RETURN_IF_ERROR(validate_scalar(nodes, n.left, schema, nullptr, depth + 1));
      DFX_RETURN_IF_ERROR(validate_scalar(nodes, n.right, schema, nullptr, depth + 1));
      const bool ok = (n.op >= DFX_OP_EQ && n.op <= DFX_OP_DIVIDE) || n.op == DFX_OP_AND || n.op == DFX_OP_OR;
      if (!ok)  // expression.rs:494-497
        return Status::Err(DFX_EXECUTION_ERROR, std::string("operator: ") + op_debug(n.op));
      if (name) *name = expr_debug(nodes, idx);  // format!("{:?} {:?} {:?}", left, op, right)
      return Status::OK();
    }
    default:  // IsNull / IsNotNull / Sort / ScalarFunction / AggregateFunction (expression.rs:500-503)
      return Status::Err(DFX_EXECUTION_ERROR, "expression " + expr_debug(nodes, idx));
  }
}

// Rust `as` on the canonical 64-bit image (same table as the device cast_value / oracle cast_val):
// used to fold CAST(literal) at compile time
int64_t sat_i64(double x, int64_t lo, int64_t hi) {
  if (x != x) return 0;
  if (x <= (double)lo) return lo;
  if (x >= (double)hi) return hi;
  return (int64_t)x;
}
uint64_t sat_u64(double x, uint64_t hi) {
  if (x != x) return 0;
  if (x <= 0.0) return 0;
  if (x >= (double)hi) return hi;
  return (uint64_t)x;
}
uint64_t wrap_int(int t, uint64_t x) {
  switch (t) {
    case DFX_INT8: return (uint64_t)(int64_t)(int8_t)x;
    case DFX_INT16: return (uint64_t)(int64_t)(int16_t)x;
    case DFX_INT32: return (uint64_t)(int64_t)(int32_t)x;
    case DFX_UINT8: return (uint64_t)(uint8_t)x;
    case DFX_UINT16: return (uint64_t)(uint16_t)x;
    case DFX_UINT32: return (uint64_t)(uint32_t)x;
    default: return x;
  }
}
}  // namespace

uint64_t host_cast_value(int from, int to, uint64_t v) {
  if (from == to) return v;
  auto f64b = [](double d) { uint64_t b; memcpy(&b, &d, 8); return b; };
  auto f32b = [](float f) { uint32_t b; memcpy(&b, &f, 4); return (uint64_t)b; };
  if (dtype_is_int(from)) {
    if (dtype_is_int(to)) return wrap_int(to, v);
    if (to == DFX_FLOAT64) return f64b(dtype_is_signed(from) ? (double)(int64_t)v : (double)v);
    return f32b(dtype_is_signed(from) ? (float)(int64_t)v : (float)v);
  }
  double x;
  if (from == DFX_FLOAT32) { uint32_t b = (uint32_t)v; float f; memcpy(&f, &b, 4); x = (double)f; }
  else memcpy(&x, &v, 8);
  switch (to) {
    case DFX_FLOAT32: return from == DFX_FLOAT32 ? v : f32b((float)x);
    case DFX_FLOAT64: return f64b(x);
    case DFX_INT8: return (uint64_t)sat_i64(x, -128, 127);
    case DFX_INT16: return (uint64_t)sat_i64(x, -32768, 32767);
    case DFX_INT32: return (uint64_t)sat_i64(x, -2147483648ll, 2147483647ll);
    case DFX_INT64: return (uint64_t)sat_i64(x, INT64_MIN, INT64_MAX);
    case DFX_UINT8: return sat_u64(x, 255ull);
    case DFX_UINT16: return sat_u64(x, 65535ull);
    case DFX_UINT32: return sat_u64(x, 4294967295ull);
    case DFX_UINT64: return sat_u64(x, UINT64_MAX);
    default: return 0;
  }
}

namespace {
Status copy_tree(const dfx_expr_node* nodes, int32_t n_nodes, int32_t root, dfx_runtime_expr* e) {
  if (!nodes || n_nodes <= 0 || root < 0 || root >= n_nodes)
    return Status::Err(DFX_INTERNAL_ERROR, "invalid expression tree");
  e->nodes.assign(nodes, nodes + n_nodes);
  e->strings.assign((size_t)n_nodes, std::string());
  e->has_name.assign((size_t)n_nodes, 0);
  for (int32_t i = 0; i < n_nodes; ++i) {
    if (nodes[i].name) {
      e->strings[i] = nodes[i].name;
      e->has_name[i] = 1;
    }
  }
  e->rebind();
  e->root = root;
  return Status::OK();
}

}  // namespace

}  // namespace dfx

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
using namespace dfx;

extern "C" {

int32_t dfx_abi_version(void) { return DFX_ABI_VERSION; }

int32_t dfx_compile_scalar_expr(const dfx_expr_node* nodes, int32_t n_nodes, int32_t root,
                                const struct ArrowSchema* input_schema, dfx_runtime_expr** out, char* err,
                                size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!out) return to_c(Status::Err(DFX_INTERNAL_ERROR, "null output"), err, errlen);
    *out = nullptr;
    SchemaInfo schema;
    Status st = schema_from_arrow(input_schema, &schema);
    if (!st.ok()) return to_c(st, err, errlen);
    std::unique_ptr<dfx_runtime_expr> e(new dfx_runtime_expr());
    st = copy_tree(nodes, n_nodes, root, e.get());
    if (!st.ok()) return to_c(st, err, errlen);
    st = validate_scalar(e->nodes, e->root, schema, &e->name);
    if (!st.ok()) return to_c(st, err, errlen);
    st = node_type(e->nodes, e->root, schema, &e->dtype);
    if (!st.ok()) return to_c(st, err, errlen);
    *out = e.release();
    return DFX_OK;
  });
}

int32_t dfx_compile_expr(const dfx_expr_node* nodes, int32_t n_nodes, int32_t root,
                         const struct ArrowSchema* input_schema, dfx_runtime_expr** out, char* err,
                         size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!nodes || root < 0 || root >= n_nodes)
      return to_c(Status::Err(DFX_INTERNAL_ERROR, "invalid expression tree"), err, errlen);
    if (nodes[root].kind != DFX_EXPR_AGGREGATE_FUNCTION)  // expression.rs:119
      return dfx_compile_scalar_expr(nodes, n_nodes, root, input_schema, out, err, errlen);
    if (!out) return to_c(Status::Err(DFX_INTERNAL_ERROR, "null output"), err, errlen);
    *out = nullptr;
    SchemaInfo schema;
    Status st = schema_from_arrow(input_schema, &schema);
    if (!st.ok()) return to_c(st, err, errlen);
    std::unique_ptr<dfx_runtime_expr> e(new dfx_runtime_expr());
    st = copy_tree(nodes, n_nodes, root, e.get());
    if (!st.ok()) return to_c(st, err, errlen);
    const dfx_expr_node& n = e->nodes[root];
    if (n.n_args != 1)  // assert_eq!(1, args.len()) (expression.rs:91)
      return to_c(Status::Err(DFX_INTERNAL_ERROR, strfmt("assertion failed: `(left == right)` left: `1`, right: `%d`", n.n_args)), err, errlen);
    st = validate_scalar(e->nodes, n.left, schema, nullptr);
    if (!st.ok()) return to_c(st, err, errlen);
    const char* nm = n.name ? n.name : "";
    int f = -1;
    if (!strcasecmp(nm, "min")) f = AGG_MIN;
    else if (!strcasecmp(nm, "max")) f = AGG_MAX;
    else if (!strcasecmp(nm, "count")) f = AGG_COUNT;
    else if (!strcasecmp(nm, "sum")) f = AGG_SUM;
    else if (!strcasecmp(nm, "avg")) f = AGG_AVG;  // deviation D7: typed by the planner (sqlplanner.rs:309-322), no executor in the reference
    // deviation D8: AggregateType::CountDistinct (expression.rs:37) has no executor in the reference either.  The number of distinct
    // non-null argument values, UInt64, per group; -0.0 == +0.0 and one NaN; ungrouped over nothing counted, what COUNT(x) gives
    // (dfx_distinct.cpp runs it beside a plain AggregateRelation)
    else if (!strcasecmp(nm, "count_distinct")) f = AGG_COUNT_DISTINCT;
    if (f < 0)  // expression.rs:103-106
      return to_c(Status::Err(DFX_GENERAL, std::string("Unsupported aggregate function '") + nm + "'"), err, errlen);
    e->is_aggregate = true;
    e->agg_func = f;
    e->agg_arg = n.left;
    e->agg_type = n.dtype;
    e->dtype = n.dtype;
    e->name = nm;
    *out = e.release();
    return DFX_OK;
  });
}

const char* dfx_runtime_expr_name(const dfx_runtime_expr* e) { return e ? e->name.c_str() : ""; }
int32_t dfx_runtime_expr_type(const dfx_runtime_expr* e) { return e ? e->dtype : DFX_TYPE_NONE; }
int32_t dfx_runtime_expr_is_aggregate(const dfx_runtime_expr* e) { return (e && e->is_aggregate) ? 1 : 0; }
void dfx_runtime_expr_free(dfx_runtime_expr* e) { delete e; }

}  // extern "C"
