// dfx_project.cpp -- ProjectRelation (src/execution/projection.rs) and its C-ABI constructor.
#include "dfx_relation.hpp"

#include <string.h>

namespace dfx {

ProjectRelation::ProjectRelation(std::unique_ptr<Relation> input, std::vector<dfx_runtime_expr> exprs, SchemaInfo schema)
    : input_(std::move(input)), exprs_(std::move(exprs)), schema_(std::move(schema)) {
  passthrough_.assign(exprs_.size(), -1);
  operands_.assign(exprs_.size(), kNoOperand);
  out_dtype_.assign(exprs_.size(), DFX_TYPE_NONE);
  for (size_t i = 0; i < exprs_.size() && deferred_.ok(); ++i) {
    const dfx_runtime_expr& e = exprs_[i];
    if (e.is_aggregate) {  // RuntimeExpr::get_func() panics on an aggregate (expression.rs:60)
      deferred_ = Status::Err(DFX_INTERNAL_ERROR, "explicit panic: get_func() on an aggregate expression");
      break;
    }
    const dfx_expr_node& root = e.nodes[e.root];
    if (root.kind == DFX_EXPR_COLUMN) {  // Arc clone, zero copy (expression.rs:311-315)
      passthrough_[i] = root.column;
      out_dtype_[i] = input_->schema().fields[root.column].dtype;
      continue;
    }
    int dt = DFX_TYPE_NONE;
    Status st = Status::Err(DFX_NOT_IMPLEMENTED, "");
    if (!groups_.empty() && groups_.back().outputs.size() < (size_t)kMaxOut) {
      // try to extend the current fused program; roll back if it would exceed the device limits
      std::unique_ptr<ProgramBuilder> trial(new ProgramBuilder(*groups_.back().builder));
      st = trial->add(e, e.root, &operands_[i], &dt);
      if (st.ok()) groups_.back().builder = std::move(trial);
    }
    if (!st.ok() && st.code == DFX_NOT_IMPLEMENTED) {
      Group g;
      g.builder.reset(new ProgramBuilder(input_->schema()));
      st = g.builder->add(e, e.root, &operands_[i], &dt);
      if (st.ok()) groups_.push_back(std::move(g));
    }
    if (!st.ok()) {
      deferred_ = st;
      break;
    }
    groups_.back().outputs.push_back(i);
    out_dtype_[i] = dt;
  }
  // the output schema is rebuilt from the expressions (projection.rs:52-57): names from
  // RuntimeExpr::get_name, every field nullable.  Deviation D6: actual array types.
  SchemaInfo derived;
  for (size_t i = 0; i < exprs_.size(); ++i) {
    Field f;
    f.name = exprs_[i].name;
    f.dtype = out_dtype_[i];
    f.nullable = true;
    derived.fields.push_back(f);
  }
  if (schema_.fields.size() != derived.fields.size()) {
    schema_ = derived;
  } else {
    for (size_t i = 0; i < derived.fields.size(); ++i) {
      schema_.fields[i].dtype = derived.fields[i].dtype;
      schema_.fields[i].nullable = true;
      if (schema_.fields[i].name.empty()) schema_.fields[i].name = derived.fields[i].name;
    }
  }
  if (deferred_.ok()) {  // projection push-down: the input only has to produce what the expressions read
    std::vector<char> needed(input_->schema().fields.size(), 0);
    for (int pcol : passthrough_)
      if (pcol >= 0 && pcol < (int)needed.size()) needed[pcol] = 1;
    for (const Group& g : groups_)
      for (int ci : g.builder->columns())
        if (ci >= 0 && ci < (int)needed.size()) needed[ci] = 1;
    input_->require_columns(needed);
  }
}

void ProjectRelation::explain(std::string* out, int depth) const {
  if (!deferred_.ok()) {
    explain_line(out, depth, "Project: error deferred to next(): " + deferred_.msg);
  } else {
    int pass = 0;
    for (int p : passthrough_) pass += p >= 0 ? 1 : 0;
    std::string text = strfmt("Project: %d outputs, %d zero-copy columns, %d fused programs", (int)exprs_.size(), pass, (int)groups_.size());
    for (const Group& g : groups_) text += strfmt(" [%d outputs, %s]", (int)g.outputs.size(), explain_program(g.builder->program()).c_str());
    explain_line(out, depth, text);
  }
  if (input_) input_->explain(out, depth + 1);
}

Status ProjectRelation::next(DeviceBatch* out, bool* has) {
  *has = false;
  DeviceBatch in;
  bool got = false;
  DFX_RETURN_IF_ERROR(input_->next(&in, &got));
  if (!got) return Status::OK();
  if (!deferred_.ok()) return deferred_;
  DFX_RETURN_IF_ERROR(ensure_init());
  hipStream_t s = ctx().stream;
  const int64_t n = in.num_rows;
  out->num_rows = n;
  out->columns.clear();
  out->columns.resize(exprs_.size());
  bool any_computed = false;
  for (size_t i = 0; i < exprs_.size(); ++i) {
    if (passthrough_[i] >= 0) out->columns[i] = in.columns[passthrough_[i]];
    else any_computed = true;
  }
  if (!any_computed || n == 0) {
    for (size_t i = 0; i < exprs_.size(); ++i) {
      if (passthrough_[i] >= 0) continue;
      out->columns[i].dtype = out_dtype_[i];
      out->columns[i].length = 0;
    }
    *has = true;
    return Status::OK();
  }
  if (!ctrl_) DFX_RETURN_IF_ERROR(alloc_zeroed_ctrl(&ctrl_));
  const int64_t n_words = (n + 63) / 64;
  Status st;
  for (const Group& g : groups_) {
    DevProgram prog;
    DevColumns cols;
    DFX_RETURN_IF_ERROR(g.builder->bind(in, &prog, &cols));
    const double in_bytes = program_input_bytes(*g.builder, in, n);
    DevProjectPlan plan;
    memset(&plan, 0, sizeof(plan));
    double out_bytes = 0;
    plan.n_out = (int32_t)g.outputs.size();
    for (size_t k = 0; k < g.outputs.size(); ++k) {
      const size_t i = g.outputs[k];
      DeviceColumn& oc = out->columns[i];
      oc.dtype = out_dtype_[i];
      oc.length = n;
      const size_t vbytes = oc.dtype == DFX_BOOLEAN ? sizeof(uint64_t) * (size_t)n_words : (size_t)n * dtype_width(oc.dtype);
      auto vals = device_alloc(vbytes, &st);
      if (!vals) return st;
      oc.values = vals.get();
      oc.owners.push_back(vals);
      plan.out[k] = operands_[i];
      plan.out_dtype[k] = (uint8_t)oc.dtype;
      plan.out_values[k] = vals.get();
      out_bytes += (double)vbytes;
      if (prog.has_nulls) {  // null in => null out (arrow 0.12 math_op / and / or)
        auto vb = device_alloc(sizeof(uint64_t) * (size_t)n_words, &st);
        if (!vb) return st;
        oc.validity = (const uint8_t*)vb.get();
        oc.null_count = -1;
        oc.owners.push_back(vb);
        plan.out_validity[k] = (uint64_t*)vb.get();
        out_bytes += (double)n / 8.0;
      }
    }
    DFX_HIP(launch_project(prog, cols, plan, n, (uint32_t*)ctrl_.get(), in_bytes + out_bytes, s));
  }
  DFX_RETURN_IF_ERROR(take_ctrl_error(ctrl_, s));
  *has = true;
  return Status::OK();
}

}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_project_relation_new(struct ArrowArrayStream* input, const dfx_runtime_expr* const* exprs,
                                 int32_t n_exprs, const struct ArrowSchema* schema, struct ArrowArrayStream* out,
                                 char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!out || (n_exprs > 0 && !exprs)) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    std::unique_ptr<Relation> in;
    Status st = adopt_input_stream(input, &in);
    if (!st.ok()) return to_c(st, err, errlen);
    SchemaInfo si;
    st = schema_from_arrow(schema, &si);
    if (!st.ok()) return to_c(st, err, errlen);
    if (n_exprs < 1)  // RecordBatch::new asserts at least one column
      return to_c(Status::Err(DFX_INTERNAL_ERROR, "assertion failed: record batch needs at least one column"), err, errlen);
    std::vector<dfx_runtime_expr> ev;
    for (int i = 0; i < n_exprs; ++i) ev.push_back(*exprs[i]);
    std::unique_ptr<Relation> rel(new ProjectRelation(std::move(in), std::move(ev), si));
    export_relation(std::move(rel), out);
    return DFX_OK;
  });
}

}  // extern "C"
