// dfx_filter.cpp -- FilterRelation (src/execution/filter.rs): the predicate's fused programs, next() as a driver over the
// three ways to a bitmap (a Utf8 term's own, the single-pass kernel, mask -> AND -> scan) and the per-column compaction;
// its C-ABI constructors and the test hook that reads the bitmap back.
#include "dfx_gather.hpp"
#include "dfx_relation.hpp"
#include "dfx_row_source.hpp"

#include <string.h>

namespace dfx {

FilterRelation::FilterRelation(std::unique_ptr<Relation> input, const dfx_runtime_expr& expr, SchemaInfo schema, OptionOverrides options)
    : input_(std::move(input)), expr_(expr), schema_(std::move(schema)) {
  opt_.overrides = std::move(options);
  prog_schema_ = input_->schema();
  const Status terms_st = terms_.compile(expr_, input_->schema(), (int)prog_schema_.fields.size());
  terms_.append_fields(&prog_schema_);
  builder_.reset(new ProgramBuilder(prog_schema_));
  int dt = DFX_TYPE_NONE;
  deferred_ = terms_st.ok() ? builder_->add(program_predicate(), program_predicate().root, &pred_operand_, &dt) : terms_st;
  if (deferred_.ok() && dt != DFX_BOOLEAN)  // filter.rs:64-66
    deferred_ = Status::Err(DFX_EXECUTION_ERROR, "Filter expression did not evaluate to boolean");
  memset(&fast_, 0, sizeof(fast_));
  if (!deferred_.ok() && program_limit_error(deferred_)) deferred_ = build_parts();
  else if (deferred_.ok()) builder_->build_fast(pred_operand_, nullptr, 0, nullptr, 0, &fast_);
}

// the predicate does not fit one fused program: split its top-level AND chain
Status FilterRelation::build_parts() {
  const Status whole = deferred_;
  const dfx_runtime_expr& pe = program_predicate();  // (string terms are Boolean columns here)
  std::vector<int32_t> conj;  // roots of the conjuncts, left to right
  {
    std::vector<int32_t> stack{pe.root};
    while (!stack.empty()) {
      const int32_t at = stack.back();
      stack.pop_back();
      if (at < 0 || at >= (int32_t)pe.nodes.size()) return whole;
      const dfx_expr_node& n = pe.nodes[(size_t)at];
      if (n.kind == DFX_EXPR_BINARY && n.op == DFX_OP_AND) {
        stack.push_back(n.right);
        stack.push_back(n.left);
      } else {
        conj.push_back(at);
      }
    }
  }
  if (conj.size() < 2) return whole;  // nothing to split (one oversized comparison / OR tree)
  // AND chain over conj[from, to) as an expression of its own (the original nodes plus the new AND nodes)
  auto chain = [&](size_t from, size_t to) {
    dfx_runtime_expr e = pe;
    int32_t root = conj[from];
    for (size_t i = from + 1; i < to; ++i) {
      dfx_expr_node a;
      memset(&a, 0, sizeof(a));
      a.kind = DFX_EXPR_BINARY;
      a.op = DFX_OP_AND;
      a.dtype = DFX_BOOLEAN;
      a.left = root;
      a.right = conj[i];
      a.column = -1;
      e.nodes.push_back(a);
      e.strings.emplace_back();
      e.has_name.push_back(0);
      root = (int32_t)e.nodes.size() - 1;
    }
    e.root = root;
    e.rebind();
    return e;
  };
  std::vector<Part> parts;
  size_t from = 0;
  while (from < conj.size()) {
    Part best;
    size_t best_to = from;
    for (size_t to = from + 1; to <= conj.size(); ++to) {  // the longest prefix of the remaining conjuncts that fits
      Part p;
      p.builder.reset(new ProgramBuilder(prog_schema_));
      memset(&p.fast, 0, sizeof(p.fast));
      const dfx_runtime_expr e = chain(from, to);
      int dt = DFX_TYPE_NONE;
      Status st = p.builder->add(e, e.root, &p.operand, &dt);
      if (!st.ok()) {
        if (program_limit_error(st) && best_to > from) break;  // the previous prefix is this part
        return st;                                             // a single conjunct that does not fit, or a real error
      }
      if (dt != DFX_BOOLEAN) return Status::Err(DFX_EXECUTION_ERROR, "Filter expression did not evaluate to boolean");
      p.builder->build_fast(p.operand, nullptr, 0, nullptr, 0, &p.fast);
      best = std::move(p);
      best_to = to;
    }
    parts.push_back(std::move(best));
    from = best_to;
  }
  builder_ = std::move(parts[0].builder);
  pred_operand_ = parts[0].operand;
  fast_ = parts[0].fast;
  for (size_t i = 1; i < parts.size(); ++i) more_.push_back(std::move(parts[i]));
  return Status::OK();
}

void FilterRelation::explain(std::string* out, int depth) const {
  if (!deferred_.ok()) {
    explain_line(out, depth, "Filter: error deferred to next(): " + deferred_.msg);
  } else {
    const uint8_t none[kMaxAggs] = {0};
    const DevProgram& P = builder_->program();
    const char* shape = row_source_prose(ScanKernel::filter_fused, row_source_without_batch(ScanKernel::filter_fused, P, fast_, 0, 0, none, none, false), 0);
    int n = 0;
    for (size_t i = 0; i < schema_.fields.size() || i < out_needed_.size(); ++i) n += (out_needed_.empty() || (i < out_needed_.size() && out_needed_[i])) ? 1 : 0;
    const bool single = more_.empty() && opt_.get().filter_single_pass;
    explain_line(out, depth, std::string("Filter: ") + (single ? "single pass (predicate, bitmap, look-back over the tiles' kept counts and compaction of the predicate's own columns in one kernel), "
                                                                 : "mask + scan + compaction (two passes over the predicate's columns), ") +
                                 explain_program(P) + ", " + shape +
                                 (out_needed_.empty() ? std::string(", every column compacted") : strfmt(", %d columns compacted", n)) +
                                 (more_.empty() ? std::string() : strfmt(", conjunction evaluated by %zu fused programs (masks ANDed)", more_.size() + 1)) +
                                 (terms_.empty() ? std::string()
                                                 : std::string(terms_.whole() ? "; the predicate is one Utf8 string term, its bitmap is the mask (no program runs): "
                                                                              : "; Utf8 string terms evaluated per batch into virtual Boolean columns: ") + terms_.explain()));
  }
  if (input_) input_->explain(out, depth + 1);
}

// the consumer reads only `needed` of the filter's output columns: the input must still deliver the predicate's
// columns, and only the needed ones are compacted
void FilterRelation::require_columns(const std::vector<char>& needed) {
  out_needed_ = needed;
  std::vector<char> in_needed = needed;
  in_needed.resize(input_->schema().fields.size(), 1);
  for (int ci : builder_->columns())
    if (ci >= 0 && ci < (int)in_needed.size()) in_needed[ci] = 1;
  for (const Part& p : more_)
    for (int ci : p.builder->columns())
      if (ci >= 0 && ci < (int)in_needed.size()) in_needed[ci] = 1;
  for (const Utf8TermSpec& t : terms_.terms())  // a string term's Utf8 column, although nobody may project it
    if (t.src_col >= 0 && t.src_col < (int)in_needed.size()) in_needed[t.src_col] = 1;
  input_->require_columns(in_needed);
}

// fn filter matches on the column type before it looks at a row, and errs for the batch whatever is projected later
// (filter.rs:105-108)
static Status reject_boolean_columns(const DeviceBatch& in) {
  for (const DeviceColumn& c : in.columns)
    if (c.dtype == DFX_BOOLEAN) return Status::Err(DFX_EXECUTION_ERROR, "filter not supported for Boolean");
  return Status::OK();
}

Status FilterRelation::next(DeviceBatch* out, bool* has) {
  *has = false;
  if (!source_told_) {  // this operator's own option set decides how a host source below moves its batches
    source_told_ = true;
    if (!opt_.overrides.empty()) input_->host_stream_options(host_stream_options_of(opt_.get()));
  }
  DeviceBatch in;
  bool got = false;
  DFX_RETURN_IF_ERROR(input_->next(&in, &got));
  if (!got) return Status::OK();
  if (!deferred_.ok()) return deferred_;
  DFX_RETURN_IF_ERROR(ensure_init());
  out->columns.clear();
  out->columns.resize(in.columns.size());
  if (in.num_rows == 0) {
    DFX_RETURN_IF_ERROR(emit_empty(in, out));
    *has = true;
    return Status::OK();
  }
  // Utf8 string terms first, on the same stream: their bitmaps are bound as virtual Boolean columns after the input's own
  // (`in` stays what the output and fn filter's Boolean check see)
  DeviceBatch ext;
  if (!terms_.empty()) DFX_RETURN_IF_ERROR(terms_.eval(in, &ext));
  const DeviceBatch& pin = terms_.empty() ? in : ext;
  const bool term_is_mask = terms_.whole() && more_.empty();  // the predicate is one string term: no program runs
  Bound first;
  if (!term_is_mask) DFX_RETURN_IF_ERROR(bind_program(*builder_, fast_, pin, in.num_rows, &first));
  if (!ctrl_) DFX_RETURN_IF_ERROR(alloc_zeroed_ctrl(&ctrl_));
  Batch b;
  DFX_RETURN_IF_ERROR(alloc_scratch(in, /*with_mask=*/!term_is_mask, &b));
  bool done = false;
  if (term_is_mask) {
    DFX_RETURN_IF_ERROR(mask_from_term(ext, &b));
    done = true;
  } else if (more_.empty() && opt_.get().filter_single_pass) {
    DFX_RETURN_IF_ERROR(mask_single_pass(in, first, &b, &done));
  }
  if (!done) DFX_RETURN_IF_ERROR(mask_two_pass(pin, first, &b));
  // (a device error has returned by now: it comes before the Boolean-column error on a non-empty batch)
  if (keep_mask_) {
    last_mask_ = b.mask;
    last_mask_rows_ = b.n;
  }
  DFX_RETURN_IF_ERROR(reject_boolean_columns(in));
  for (size_t c = 0; c < in.columns.size(); ++c) {  // fn filter per column (filter.rs:55-57)
    const DeviceColumn& ic = in.columns[c];
    DeviceColumn& oc = out->columns[c];
    oc.dtype = ic.dtype;
    oc.length = (int64_t)b.kept;
    oc.null_count = 0;  // value nulls are ignored: the output is all-valid (filter.rs:83-92)
    if (ic.absent || (c < out_needed_.size() && !out_needed_[c])) oc.absent = true;  // projection push-down: nobody reads it
    else if (ic.dtype == DFX_UTF8) DFX_RETURN_IF_ERROR(compact_utf8(ic, b, &oc));
    else DFX_RETURN_IF_ERROR(compact_fixed(ic, c, b, &oc));
  }
  out->num_rows = (int64_t)b.kept;
  *has = true;
  return Status::OK();
}

// zero-row batches are still emitted (filter.rs:55-62)
Status FilterRelation::emit_empty(const DeviceBatch& in, DeviceBatch* out) {
  DFX_RETURN_IF_ERROR(reject_boolean_columns(in));
  for (size_t c = 0; c < in.columns.size(); ++c) {
    out->columns[c].dtype = in.columns[c].dtype;
    out->columns[c].length = 0;
  }
  out->num_rows = 0;
  return Status::OK();
}

Status FilterRelation::bind_program(const ProgramBuilder& builder, const DevFastPlan& fast, const DeviceBatch& pin, int64_t n, Bound* p) {
  DFX_RETURN_IF_ERROR(builder.bind(pin, &p->prog, &p->cols));
  p->in_bytes = (double)n / 8.0 + program_input_bytes(builder, pin, n);
  p->fast = fast;
  if (!opt_.get().fast) p->fast.valid = 0;
  return Status::OK();
}

Status FilterRelation::alloc_scratch(const DeviceBatch& in, bool with_mask, Batch* b) {
  b->n = in.num_rows;
  b->n_words = (b->n + 63) / 64;
  b->n_tiles = (b->n + kTileRows - 1) / kTileRows;
  b->fused_vals.resize(in.columns.size());
  Status st;
  if (with_mask) {
    b->mask = device_alloc(sizeof(uint64_t) * (size_t)b->n_words, &st);
    if (!b->mask) return st;
  }
  b->counts = device_alloc(sizeof(uint32_t) * (size_t)b->n_tiles, &st);
  if (!b->counts) return st;
  b->offsets = device_alloc(sizeof(uint64_t) * (size_t)(b->n_tiles + 1), &st);
  if (!b->offsets) return st;
  b->tmp = device_alloc(sizeof(uint64_t) * (size_t)(b->n_tiles / 4096 + 4), &st);
  return b->tmp ? Status::OK() : st;
}

// tile counts -> tile offsets, and the kept count on its way to the host (the caller synchronises)
Status FilterRelation::queue_scan_and_kept(Batch* b) {
  hipStream_t s = ctx().stream;
  DFX_HIP(launch_scan_u32((const uint32_t*)b->counts.get(), (uint64_t*)b->offsets.get(), b->n_tiles, (uint64_t*)b->tmp.get(), s));
  DFX_HIP(hipMemcpyAsync(&b->kept, (uint64_t*)b->offsets.get() + b->n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  return Status::OK();
}

// The whole predicate is one string term: its bitmap IS the mask -- tile counts, scan and compaction take it as it is.
// (sel_seen_ is left alone: it sizes the output buffers of the single-pass kernel, which never runs for such a predicate)
Status FilterRelation::mask_from_term(const DeviceBatch& ext, Batch* b) {
  hipStream_t s = ctx().stream;
  b->mask = ext.columns[(size_t)terms_.terms()[0].virt_col].owners[0];
  DFX_HIP(launch_mask_tile_counts((const uint64_t*)b->mask.get(), (uint32_t*)b->counts.get(), b->n, s));
  DFX_RETURN_IF_ERROR(queue_scan_and_kept(b));
  DFX_HIP(hipStreamSynchronize(s));
  return Status::OK();
}

// SINGLE PASS: predicate, bitmap, tile offsets (decoupled look-back) and the compaction of up to kFusedOutCols of
// the predicate's own columns in one kernel -- such a column is read from HBM once (filter.rs:46-110)
Status FilterRelation::mask_single_pass(const DeviceBatch& in, const Bound& p, Batch* b, bool* done) {
  hipStream_t s = ctx().stream;
  const int64_t n = b->n;
  Status st;
  DevFusedOut O;
  memset(&O, 0, sizeof(O));
  // Output buffers sized from the selectivity this stream has shown so far (the first batch: every row): a 2^27-row batch of
  // two Float64 predicate columns pinned 2 GB of HBM however few rows it kept.  A batch that keeps more than its buffers hold
  // has those columns compacted again from the bitmap (compact_fixed): a second read of the column, paid only then.
  const uint64_t fused_cap = sel_seen_ < 0.0 ? (uint64_t)n
                                             : std::min<uint64_t>((uint64_t)n, (uint64_t)((double)n * std::min(1.0, 1.5 * sel_seen_ + 0.02)) + 4096);
  O.cap_rows = fused_cap;
  O.dense = opt_.get().filter_dense < 0 ? (sel_seen_ > 0.22 ? 1u : 0u) : (uint32_t)(opt_.get().filter_dense != 0);
  const bool any_boolean = !reject_boolean_columns(in).ok();  // (the batch errs after the mask: nothing is compacted for it)
  const std::vector<int>& pcols = builder_->columns();
  for (size_t slot = 0; slot < pcols.size() && O.n < kFusedOutCols && !any_boolean; ++slot) {
    const int ci = pcols[slot];
    if (ci < 0 || ci >= (int)in.columns.size()) continue;
    const DeviceColumn& ic = in.columns[ci];
    if (ic.absent || ic.dtype == DFX_UTF8 || ic.dtype == DFX_BOOLEAN) continue;
    if ((size_t)ci < out_needed_.size() && !out_needed_[ci]) continue;  // projection push-down: nobody reads it
    if (b->fused_vals[ci]) continue;
    auto vals = device_alloc((size_t)std::max<uint64_t>(fused_cap, 1) * dtype_width(ic.dtype), &st);
    if (!vals) return st;
    b->fused_vals[ci] = vals;
    O.slot[O.n] = (uint8_t)slot;
    O.dtype[O.n] = (uint8_t)ic.dtype;
    O.out[O.n] = vals.get();
    ++O.n;
  }
  const size_t sync_words = filter_fused_sync_words(n);
  auto sync = device_alloc(sizeof(uint64_t) * sync_words, &st);
  if (!sync) return st;
  DFX_HIP(hipMemsetAsync(sync.get(), 0, sizeof(uint64_t) * sync_words, s));
  DFX_HIP(launch_filter_fused(p.prog, p.fast, p.cols, pred_operand_, n, (uint64_t*)b->mask.get(), (uint64_t*)b->offsets.get(), (uint64_t*)sync.get(), O,
                              (uint32_t*)ctrl_.get(), p.in_bytes, s));
  // the kernel leaves the kept count next to the error word of the control block: one 64-byte copy into pinned memory
  // and one synchronisation per batch (two pageable 8-byte copies cost ~30 us of a 2^27-row batch's 340)
  if (!ctrl_host_) {
    ctrl_host_ = pinned_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
    if (!ctrl_host_) return st;
  }
  // (by a kernel writing the pinned buffer, not by the copy engine: an SDMA device-to-host copy stalls for 6 - 150 ms once in a few
  // hundred calls on these boxes -- tools/d2h_probe.py -- and this one runs once per batch: round 5's bench lines showed one or the other
  // of the dense-filter legs a third slower, never the same one)
  DFX_HIP(launch_copy_to_host(ctrl_.get(), ctrl_host_.get(), sizeof(uint32_t) * CTRL_WORDS, s));
  DFX_HIP(hipStreamSynchronize(s));
  const uint32_t* hc = (const uint32_t*)ctrl_host_.get();
  const uint32_t errbits = hc[CTRL_ERROR];
  if (errbits & 8u) {  // (also next to another error bit: the fused outputs sit at wrong offsets, and the second pass reports the real error)
    // The look-back gave up waiting (its grid is sized for an EMPTY device: other work on the GPU -- another process, a
    // multi-rank dry run -- can keep a workgroup from becoming resident).  Not an error of the query: this batch takes the
    // two-pass form, which has no inter-workgroup waits.  (sel_seen_ learns nothing from it.)
    DFX_HIP(hipMemsetAsync(ctrl_.get(), 0, sizeof(uint32_t) * CTRL_WORDS, s));
    for (auto& v : b->fused_vals) v.reset();
    ++counters().filter_lookback_fallbacks;
    *done = false;
    return Status::OK();
  }
  if (errbits) return clear_ctrl_error(ctrl_, errbits, s);
  b->kept = (uint64_t)hc[CTRL_PASSED_LO] | ((uint64_t)hc[CTRL_PASSED_HI] << 32);
  sel_seen_ = std::max(sel_seen_, (double)b->kept / (double)n);
  if (b->kept > fused_cap) {  // denser than the stream had been: the kernel stored what fitted; compact_fixed does these columns again
    for (auto& v : b->fused_vals) v.reset();
    ++counters().filter_output_regrows;
  }
  *done = true;
  return Status::OK();
}

// TWO PASSES: the first program writes the bitmap and the tile counts, the other conjuncts' masks are ANDed into it (the
// tile counts redone), then scan and read-back.  No inter-workgroup waits.
Status FilterRelation::mask_two_pass(const DeviceBatch& pin, const Bound& first, Batch* b) {
  hipStream_t s = ctx().stream;
  DFX_HIP(launch_predicate_mask(first.prog, first.fast, first.cols, pred_operand_, b->n, (uint64_t*)b->mask.get(), (uint32_t*)b->counts.get(),
                                (uint32_t*)ctrl_.get(), first.in_bytes, s));
  if (!more_.empty()) {
    Status st;
    auto mask2 = device_alloc(sizeof(uint64_t) * (size_t)b->n_words, &st);
    if (!mask2) return st;
    for (const Part& part : more_) {
      Bound p;
      DFX_RETURN_IF_ERROR(bind_program(*part.builder, part.fast, pin, b->n, &p));
      DFX_HIP(launch_predicate_mask(p.prog, p.fast, p.cols, part.operand, b->n, (uint64_t*)mask2.get(), nullptr, (uint32_t*)ctrl_.get(), p.in_bytes, s));
      DFX_HIP(launch_mask_and_count((uint64_t*)b->mask.get(), (const uint64_t*)mask2.get(), (uint32_t*)b->counts.get(), b->n, s));
    }
  }
  DFX_RETURN_IF_ERROR(queue_scan_and_kept(b));
  return take_ctrl_error(ctrl_, s);
}

Status FilterRelation::compact_fixed(const DeviceColumn& ic, size_t c, const Batch& b, DeviceColumn* oc) {
  if (b.fused_vals[c]) {  // compacted by the kernel that evaluated the predicate
    oc->values = b.fused_vals[c].get();
    oc->owners = {b.fused_vals[c]};
    return Status::OK();
  }
  // deviation D2: every fixed-width type, not just Float64
  const int w = dtype_width(ic.dtype);
  const int64_t n = b.n, m = (int64_t)b.kept;
  Status st;
  auto vals = device_alloc((size_t)(m > 0 ? m : 1) * w, &st);
  if (!vals) return st;
  DFX_HIP(launch_compact(ic.values, w, (const uint64_t*)b.mask.get(), (const uint64_t*)b.offsets.get(), n, vals.get(),
                         (double)n * w + (double)m * w + (double)n / 8.0, ctx().stream));
  oc->values = vals.get();
  oc->owners = {vals};
  return Status::OK();
}

// lengths + starts -> compact both -> scan lengths -> gather bytes
Status FilterRelation::compact_utf8(const DeviceColumn& ic, const Batch& b, DeviceColumn* oc) {
  hipStream_t s = ctx().stream;
  const int64_t n = b.n, m = (int64_t)b.kept;
  const uint64_t* mask = (const uint64_t*)b.mask.get();
  const uint64_t* offsets = (const uint64_t*)b.offsets.get();
  Status st;
  auto lens = device_alloc(sizeof(int32_t) * (size_t)n, &st);
  if (!lens) return st;
  auto starts = device_alloc(sizeof(int32_t) * (size_t)n, &st);
  if (!starts) return st;
  auto lens_c = device_alloc(sizeof(int32_t) * (size_t)(m + 1), &st);
  if (!lens_c) return st;
  auto starts_c = device_alloc(sizeof(int32_t) * (size_t)(m + 1), &st);
  if (!starts_c) return st;
  DFX_HIP(launch_utf8_lengths(ic.offsets, n, (int32_t*)lens.get(), (int32_t*)starts.get(), s));
  DFX_HIP(launch_compact(lens.get(), 4, mask, offsets, n, lens_c.get(), 0, s));
  DFX_HIP(launch_compact(starts.get(), 4, mask, offsets, n, starts_c.get(), 0, s));
  std::shared_ptr<void> offs, bytes;  // (a subset of a column that fit: the 2 GB rule cannot fire here)
  DFX_RETURN_IF_ERROR(utf8_layout_from_lens((const int32_t*)lens_c.get(), m, "filtered Utf8 column", &offs, &bytes, &oc->data_bytes));
  DFX_HIP(launch_utf8_gather(ic.data, (const int32_t*)starts_c.get(), (const int32_t*)offs.get(), m, (uint8_t*)bytes.get(), s));
  oc->offsets = (const int32_t*)offs.get();
  oc->data = (const uint8_t*)bytes.get();
  oc->owners = {offs, bytes};
  return Status::OK();
}

}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_filter_relation_new(struct ArrowArrayStream* input, const dfx_runtime_expr* expr,
                                const struct ArrowSchema* schema, struct ArrowArrayStream* out, char* err,
                                size_t errlen) {
  return dfx_filter_relation_new_with_options(input, expr, schema, nullptr, 0, out, err, errlen);
}

int32_t dfx_filter_relation_new_with_options(struct ArrowArrayStream* input, const dfx_runtime_expr* expr,
                                             const struct ArrowSchema* schema, const dfx_option* options, int32_t n_options,
                                             struct ArrowArrayStream* out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!expr || !out || (n_options > 0 && !options)) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    OptionOverrides ov;
    Status st = parse_option_overrides(options, n_options, &ov);
    if (!st.ok()) return to_c(st, err, errlen);
    std::unique_ptr<Relation> in;
    st = adopt_input_stream(input, &in);
    if (!st.ok()) return to_c(st, err, errlen);
    SchemaInfo si;
    st = schema_from_arrow(schema, &si);
    if (!st.ok()) return to_c(st, err, errlen);
    si = schema_names_over(si, in->schema());
    if (expr->is_aggregate)
      return to_c(Status::Err(DFX_INTERNAL_ERROR, "explicit panic: get_func() on an aggregate expression"), err, errlen);
    std::unique_ptr<Relation> rel(new FilterRelation(std::move(in), *expr, si, std::move(ov)));
    export_relation(std::move(rel), out);
    return DFX_OK;
  });
}

// Test hook: the Arrow bitmap FilterRelation computed for its most recent input batch (the BooleanArray of the reference's
// predicate closure, filter.rs:53).  out == NULL switches the keeping on (call before next()); else (rows + 7) / 8 bytes
// are copied to `out`.
int32_t dfx_filter_debug_mask(struct ArrowArrayStream* stream, uint8_t* out, int64_t out_bytes, int64_t* rows, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    Relation* r = peek_exported(stream);
    if (!r || r->kind() != REL_FILTER) return to_c(Status::Err(DFX_GENERAL, "not a FilterRelation of this library"), err, errlen);
    FilterRelation* f = static_cast<FilterRelation*>(r);
    if (!out) {
      f->keep_mask(true);
      return DFX_OK;
    }
    const int64_t n = f->last_mask_rows();
    if (!f->last_mask() || out_bytes < (n + 7) / 8) return to_c(Status::Err(DFX_GENERAL, "no bitmap kept, or the buffer is too small"), err, errlen);
    hipError_t e = hipMemcpy(out, f->last_mask().get(), (size_t)((n + 7) / 8), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s", hipGetErrorString(e))), err, errlen);
    if (rows) *rows = n;
    return DFX_OK;
  });
}

}  // extern "C"
