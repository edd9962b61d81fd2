// dfx_aggregate.cpp -- AggregateRelation (src/execution/aggregate.rs) on the device.
//
//   without_group_by (aggregate.rs:703-785): per input batch ONE fused kernel (predicate +
//     argument expressions + per-aggregate reduction, K5) produces the batch scalars, a one-thread
//     fold kernel applies AccumulatorSet::accumulate_scalar; one row comes back at end of input.
//   with_group_by (aggregate.rs:787-952): per input batch ONE fused kernel (K7 = predicate + key
//     and argument expressions + hash aggregation into an HBM-resident open-addressing table with
//     an LDS front cache); the table grows by rehash when it passes its load limit (rows that do
//     not fit are spilled and replayed); K8 emits dense arrays at end of input.
//   A FilterRelation feeding the aggregate (context.rs:126-139,162-192) is absorbed: its predicate
//   becomes part of the fused program and no filtered batch is ever materialised.
#include "dfx_aggregate_impl.hpp"
#include "dfx_row_source.hpp"

namespace dfx {

AggOptions& agg_options() {
  static AggOptions o;
  return o;
}

// ---- setup ---------------------------------------------------------------------------------------
Status AggregateRelation::Impl::setup(const SchemaInfo& input_schema) {
  bind_schema = input_schema;
  group_rw = group;
  key_out_dtype.assign(group.size(), 0);
  for (size_t k = 0; k < group.size(); ++k) {  // GroupByScalar::Utf8 (aggregate.rs:838-846)
    if (group[k].is_aggregate || group[k].root < 0) continue;
    const dfx_expr_node& r = group[k].nodes[group[k].root];
    if (r.kind != DFX_EXPR_COLUMN || r.column < 0 || r.column >= (int)input_schema.fields.size()) continue;
    if (input_schema.fields[r.column].dtype != DFX_UTF8) continue;
    DictKey d;
    d.key = (int)k;
    d.src_col = r.column;
    d.virt_col = (int)bind_schema.fields.size();
    Field f;
    f.name = "__dict_ids_" + std::to_string(k);
    f.dtype = DFX_UINT64;
    f.nullable = false;
    bind_schema.fields.push_back(f);
    group_rw[k].nodes[group_rw[k].root].column = d.virt_col;
    group_rw[k].dtype = DFX_UINT64;
    key_out_dtype[k] = DFX_UTF8;
    dicts.push_back(std::move(d));
  }
  if (has_pred) {
    DFX_RETURN_IF_ERROR(pred_terms.compile(pred, input_schema, (int)bind_schema.fields.size()));
    pred_terms.append_fields(&bind_schema);
  }
  kw_out = (int)group.size();
  na_total = (int)aggr.size();
  if (kw_out > kMaxKeys) return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("more than %d GROUP BY expressions", kMaxKeys));
  kw = kw_out;
  if (kw_out > 4) {  // (the reference builds a Vec<GroupByScalar> of any length, aggregate.rs:807-852)
    dfx_runtime_expr zero;
    dfx_expr_node n;
    memset(&n, 0, sizeof(n));
    n.kind = DFX_EXPR_LITERAL;
    n.dtype = DFX_INT64;
    n.left = n.right = n.column = -1;
    n.lit.i64 = 0;
    zero.nodes.push_back(n);
    zero.strings.emplace_back();
    zero.has_name.push_back(0);
    zero.root = 0;
    zero.dtype = DFX_INT64;
    zero.name = "0";
    while ((int)group_rw.size() < kMaxKeys) {
      group_rw.push_back(zero);
      key_out_dtype.push_back(DFX_INT64);
    }
    kw = kMaxKeys;
  }
  if (na_total > kMaxAccsTotal) return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("more than %d accumulators", kMaxAccsTotal));
  key_dtype.assign(kw, 0);
  arg_dtype.assign(na_total, 0);
  out_dtype.assign(na_total, 0);
  func.assign(na_total, 0);
  chunks.clear();
  for (int a0 = 0; a0 == 0 || a0 < na_total;) {
    // as many of the next accumulators as ONE fused program takes: <= kMaxAggs, and within the program's limits on
    // distinct columns, computed values and literals (a chunk that does not fit is rebuilt one accumulator shorter)
    int n = std::min(kMaxAggs, na_total - a0);
    for (;;) {
      Chunk ch;
      ch.a0 = a0;
      ch.n = n;
      Status st = build_chunk_programs(ch);
      if (st.ok()) {
        chunks.push_back(std::move(ch));
        break;
      }
      if (!program_limit_error(st) || n <= 1) return st;  // (a genuinely unsupported aggregate is not rebuilt kMaxAggs times)
      --n;
    }
    a0 += std::max(n, 1);
  }
  cur_chunk = 0;  // chunk 0 becomes the active one
  // one key, two or more aggregates that do not all take the same operand: the per-aggregate chunking for the partitioned
  // strategy (see single_chunks).  Built now so that a shape the one-aggregate programs cannot take shows up here, not mid-stream.
  if (kw == 1 && kw_out == 1 && na_total >= 2 && chunks.size() == 1) {  // (agg.split_aggregates / agg.shared_planes are read when the operator runs: options freeze at first use)
    std::vector<Chunk> singles;
    bool ok = true;
    for (int a = 0; a < na_total && ok; ++a) {
      Chunk ch;
      ch.a0 = a;
      ch.n = 1;
      ok = build_chunk_programs(ch).ok();
      if (ok) singles.push_back(std::move(ch));
    }
    if (ok) {
      single_chunks = std::move(singles);
      phase = Phase::Undecided;
      {  // (shared_operand() without the option: options are not frozen yet)
        split_is_shared = na() >= 2;  // (any number of aggregates of one operand: a pass 2 per plane has no limit of three)
        for (int a = 1; a < na(); ++a)
          if (active().plan.arg[a] != active().plan.arg[0]) split_is_shared = false;
        split_distinct = 1;
        split_ops = 0;
        for (int a = 1; a < na(); ++a) {
          if (active().plan.arg[a] == active().plan.arg[0]) continue;
          if (split_distinct == 1) {
            split_distinct = 2;
            split_arg1 = (uint32_t)a;
          }
          if (active().plan.arg[a] == active().plan.arg[split_arg1]) split_ops |= 1u << a;
          else split_distinct = 3;
        }
      }
    }
  }
  return Status::OK();
}

// the fused programs of one chunk: predicate + keys + arguments [a0, a0 + n), and the predicate-free twin
Status AggregateRelation::Impl::build_chunk_programs(Chunk& ch) {
  ch.fused.builder.reset(new ProgramBuilder(bind_schema));
  ProgramBuilder* builder = ch.fused.builder.get();
  DevAggPlan& plan = ch.fused.plan;
  DevFastPlan& fast = ch.fused.fast;
  memset(&plan, 0, sizeof(plan));
  memset(&fast, 0, sizeof(fast));
  plan.pred = kNoOperand;
  if (has_pred) {
    int dt = 0;
    const dfx_runtime_expr& pe = pred_terms.empty() ? pred : pred_terms.rewritten();
    DFX_RETURN_IF_ERROR(builder->add(pe, pe.root, &plan.pred, &dt));
    if (dt != DFX_BOOLEAN) return Status::Err(DFX_EXECUTION_ERROR, "Filter expression did not evaluate to boolean");
  }
  for (int k = 0; k < kw; ++k) {
    if (k < kw_out && group[k].is_aggregate) return Status::Err(DFX_INTERNAL_ERROR, "explicit panic: get_func() on an aggregate expression");
    int dt = 0;
    DFX_RETURN_IF_ERROR(builder->add(group_rw[k], group_rw[k].root, &plan.key[k], &dt));
    if (!dtype_is_int(dt))  // aggregate.rs:848-850 (floats and booleans are rejected)
      return Status::Err(DFX_EXECUTION_ERROR, "Unsupported GROUP BY data type");
    key_dtype[k] = dt;
    if (!key_out_dtype[k]) key_out_dtype[k] = dt;
    plan.key_dtype[k] = (uint8_t)dt;
  }
  for (int a = ch.a0; a < ch.a0 + ch.n; ++a) {
    const int la = a - ch.a0;  // index inside the chunk
    const dfx_runtime_expr& e = aggr[a];
    if (!e.is_aggregate)  // create_accumulators (aggregate.rs:335-337)
      return Status::Err(DFX_EXECUTION_ERROR, "invalid aggregate expression");
    int dt = 0;
    DFX_RETURN_IF_ERROR(builder->add(e, e.agg_arg, &plan.arg[la], &dt));
    arg_dtype[a] = dt;
    plan.arg_dtype[la] = (uint8_t)dt;
    func[a] = e.agg_func;
    const int t = e.agg_type;
    uint8_t& acc_kind_a = acc_kind_all[a];
    uint8_t& val_xform_a = val_xform_all[a];
    uint64_t& acc_init_a = acc_init_all[a];
    if (e.agg_func == AGG_COUNT) {  // deviation D3 (reference: "unsupported aggregate function")
      out_dtype[a] = DFX_UINT64;
      acc_kind_a = ACC_ADD_U64;
      val_xform_a = VT_COUNT_VALID;
      acc_init_a = 0;
      continue;
    }
    if (!dtype_is_numeric(t)) {  // array_min/max/sum `_ =>` arms (aggregate.rs:406-408 ...)
      const char* fn = e.agg_func == AGG_MIN ? "MIN" : e.agg_func == AGG_MAX ? "MAX" : "SUM";
      return Status::Err(DFX_EXECUTION_ERROR, std::string("Unsupported data type for ") + fn);
    }
    if (dt != t)  // downcast_ref::<T>().unwrap() by the declared type (aggregate.rs:347, :563)
      return Status::Err(DFX_INTERNAL_ERROR, strfmt("called `Option::unwrap()` on a `None` value (aggregate argument is %s, declared %s)",
                                                    dtype_name(dt), dtype_name(t)));
    out_dtype[a] = t;
    const bool grouped = kw > 0;
    if (e.agg_func == AGG_SUM) {
      val_xform_a = VT_RAW;
      if (t == DFX_FLOAT64) {
        acc_kind_a = ACC_ADD_F64;
        // grouped: the first value initialises the accumulator => identity is -0.0 (x + -0.0 == x
        // bit for bit); ungrouped: array_ops::sum starts from 0.0 (aggregate.rs:480-546)
        acc_init_a = grouped ? 0x8000000000000000ull : 0ull;
      } else if (t == DFX_FLOAT32) {
        acc_kind_a = ACC_ADD_F32;
        acc_init_a = grouped ? 0x80000000ull : 0ull;
      } else {
        acc_kind_a = ACC_ADD_U64;
        acc_init_a = 0;
      }
    } else {
      const bool is_min = e.agg_func == AGG_MIN;
      if (t == DFX_FLOAT64 || t == DFX_FLOAT32) {
        val_xform_a = t == DFX_FLOAT64 ? (is_min ? VT_F64_ORD_MIN : VT_F64_ORD_MAX) : (is_min ? VT_F32_ORD_MIN : VT_F32_ORD_MAX);
        acc_kind_a = is_min ? ACC_MIN_U64 : ACC_MAX_U64;
        acc_init_a = is_min ? ~0ull : 0ull;
      } else if (dtype_is_signed(t)) {
        val_xform_a = VT_RAW;
        acc_kind_a = is_min ? ACC_MIN_S64 : ACC_MAX_S64;
        acc_init_a = is_min ? 0x7FFFFFFFFFFFFFFFull : 0x8000000000000000ull;
      } else {
        val_xform_a = VT_RAW;
        acc_kind_a = is_min ? ACC_MIN_U64 : ACC_MAX_U64;
        acc_init_a = is_min ? ~0ull : 0ull;
      }
    }
  }
  builder->build_fast(plan.pred, plan.key, kw, plan.arg, ch.n, &fast);
  if (has_pred) {  // predicate-free twin (operands are numbered differently: its own plan)
    Programs& np = ch.np;
    np.builder.reset(new ProgramBuilder(bind_schema));
    np.plan = plan;
    np.plan.pred = kNoOperand;
    int dt = 0;
    for (int k = 0; k < kw; ++k) DFX_RETURN_IF_ERROR(np.builder->add(group_rw[k], group_rw[k].root, &np.plan.key[k], &dt));
    for (int a = ch.a0; a < ch.a0 + ch.n; ++a) DFX_RETURN_IF_ERROR(np.builder->add(aggr[a], aggr[a].agg_arg, &np.plan.arg[a - ch.a0], &dt));
    np.builder->build_fast(np.plan.pred, np.plan.key, kw, np.plan.arg, ch.n, &np.fast);
  }
  return Status::OK();
}

// Replace the chunking (grouped aggregates only): `next` becomes the chunk list, its first chunk the active one.  The
// accumulator planes are per ACCUMULATOR, not per chunk: nothing moves.
void AggregateRelation::Impl::install_chunks(std::vector<Chunk>&& next) {
  chunks = std::move(next);
  cur_chunk = 0;
  if (kw > 0 && accs_full) T = view_of(T, accs_full, 0);
  win.layout_valid = false;  // (routed rows change width)
}

// Make chunk c the active one: programs, accumulator algebra, ungrouped buffers and the table view.
void AggregateRelation::Impl::activate(int c) {
  if (c == cur_chunk) return;
  cur_chunk = c;
  if (kw > 0 && accs_full) T = view_of(T, accs_full, c);
  else if (kw == 0) set_algebra(&T);
}

// the active chunk's accumulator algebra in a table descriptor (entries beyond its accumulators stay as they are)
void AggregateRelation::Impl::set_algebra(DevTable* t) const {
  t->na = na();
  for (int a = 0; a < na(); ++a) {
    t->acc_kind[a] = acc_kind()[a];
    t->val_xform[a] = val_xform()[a];
    t->acc_init[a] = acc_init()[a];
  }
}

// chunk c's view of a table: same keys / control block, accumulator planes [a0, a0 + n)
DevTable AggregateRelation::Impl::view_of(const DevTable& any_view, uint64_t* full_accs, int c) const {
  DevTable v = any_view;
  const Chunk& ch = chunks[(size_t)c];
  v.accs = full_accs + (uint64_t)ch.a0 * v.stride;
  v.na = ch.n;
  for (int a = 0; a < kMaxAggs; ++a) {
    v.acc_kind[a] = a < ch.n ? acc_kind_all[ch.a0 + a] : 0;
    v.val_xform[a] = a < ch.n ? val_xform_all[ch.a0 + a] : 0;
    v.acc_init[a] = a < ch.n ? acc_init_all[ch.a0 + a] : 0;
  }
  return v;
}

// EVERY accumulator plane of a table as one view (the planes are contiguous by accumulator index, whatever the chunking):
// what the public partial_* entry points move.  The drain may have replaced the chunk list (one scan per aggregate,
// agg.split_aggregates): a chunk's view would then carry one plane of several and the others would be emitted with their
// init values (round-4 advisor finding).  Valid while all accumulators fit one kernel's view (<= kMaxAggs).
DevTable AggregateRelation::Impl::full_view(const DevTable& any_view, uint64_t* full_accs) const {
  DevTable v = any_view;
  v.accs = full_accs;
  v.na = na_total;
  for (int a = 0; a < kMaxAggs; ++a) {
    v.acc_kind[a] = a < na_total ? acc_kind_all[a] : 0;
    v.val_xform[a] = a < na_total ? val_xform_all[a] : 0;
    v.acc_init[a] = a < na_total ? acc_init_all[a] : 0;
  }
  return v;
}

// (after the drain: the chunk list is final)
Status AggregateRelation::Impl::partial_view_check() const {
  if (na_total > kMaxAggs) return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("multi-GPU exchange of more than %d accumulators", kMaxAggs));
  return Status::OK();
}

// what the calibration slice's outcome depends on: the fused program (predicate, key and argument expressions with
// their literals), the input columns it binds and the plan's operands (FNV-1a over the bytes)
uint64_t AggregateRelation::Impl::program_fingerprint() const {
  uint64_t h = 0xCBF29CE484222325ull;
  auto mix = [&](const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
  };
  const DevProgram& P = active().builder->program();
  mix(&P.n_ins, sizeof(P.n_ins));
  mix(&P.n_cols, sizeof(P.n_cols));
  mix(&P.n_imm, sizeof(P.n_imm));
  mix(P.ins, sizeof(DevIns) * (size_t)std::max(0, std::min<int>(P.n_ins, kMaxRegs)));
  mix(P.imm, sizeof(uint64_t) * (size_t)std::max(0, std::min<int>(P.n_imm, kMaxImm)));
  mix(P.col_dtype, sizeof(P.col_dtype));
  for (int ci : active().builder->columns()) mix(&ci, sizeof(ci));
  for (const Utf8TermSpec& t : pred_terms.terms()) {  // (the literals of string terms live outside the program)
    mix(&t.src_col, sizeof(t.src_col));
    mix(&t.op, sizeof(t.op));
    mix(t.literal.data(), t.literal.size());
  }
  mix(&active().plan.pred, 1);
  mix(active().plan.key, sizeof(active().plan.key));
  mix(active().plan.arg, sizeof(active().plan.arg));
  mix(&kw, sizeof(kw));
  const int na_now = na();
  mix(&na_now, sizeof(na_now));
  return h;
}

Status AggregateRelation::Impl::drain() {
  if (built) return Status::OK();
  ScopedUs t_drain(&counters().agg_drain_us);
  DFX_RETURN_IF_ERROR(ensure_init());
  if (!options.overrides.empty() && input) input->host_stream_options(host_stream_options_of(opt()));  // (its own option set: how a host source below moves batches)
  if (phase == Phase::Undecided && !split_allowed()) phase = Phase::NotApplicable;  // (the options are frozen by now)
  hipStream_t s = ctx().stream;
  Status st;
  if (kw == 0) {
    memset(&T, 0, sizeof(T));
    ctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
    if (!ctrl) return st;
    DFX_HIP(hipMemsetAsync(ctrl.get(), 0, sizeof(uint32_t) * CTRL_WORDS, s));
    for (int c = (int)chunks.size() - 1; c >= 0; --c) {  // every chunk: batch partials, running state, type tables (chunk 0 last: it stays active)
      activate(c);
      cur().partial = device_alloc(sizeof(uint64_t) * kReduceSlots * kReduceSlotWords, &st);
      if (!cur().partial) return st;
      cur().state = device_alloc(sizeof(uint64_t) * 2 * kMaxAggs, &st);
      if (!cur().state) return st;
      cur().dev_arg_dtype = device_alloc(kMaxAggs, &st);
      if (!cur().dev_arg_dtype) return st;
      cur().dev_func = device_alloc(kMaxAggs, &st);
      if (!cur().dev_func) return st;
      std::vector<uint64_t> hpv((size_t)kReduceSlots * kReduceSlotWords, 0);
      uint64_t* hp = hpv.data();
      uint8_t hd[kMaxAggs], hf[kMaxAggs];
      memset(hd, 0, sizeof(hd));
      memset(hf, 0, sizeof(hf));
      const int a0 = chunks[(size_t)c].a0;
      for (int a = 0; a < na(); ++a) {
        for (int sl = 0; sl < kReduceSlots; ++sl) {
          hp[(size_t)sl * kReduceSlotWords + 4 * a] = acc_init()[a];
          hp[(size_t)sl * kReduceSlotWords + 4 * a + 2] = ~0ull;
        }
        hd[a] = (uint8_t)arg_dtype[a0 + a];
        hf[a] = (uint8_t)func[a0 + a];
      }
      DFX_HIP(hipMemcpy(cur().partial.get(), hp, sizeof(uint64_t) * hpv.size(), hipMemcpyHostToDevice));  // (blocking: stack / loop-local sources)
      DFX_HIP(hipMemcpy(cur().dev_arg_dtype.get(), hd, sizeof(hd), hipMemcpyHostToDevice));
      DFX_HIP(hipMemcpy(cur().dev_func.get(), hf, sizeof(hf), hipMemcpyHostToDevice));
      DFX_HIP(hipMemsetAsync(cur().state.get(), 0, sizeof(uint64_t) * 2 * kMaxAggs, s));
    }
    set_algebra(&T);
    DFX_HIP(hipStreamSynchronize(s));
  } else {
    int cap_log2 = opt().capacity_log2 > 0 ? opt().capacity_log2 : 21;
    cap_log2 = std::max(6, std::min(cap_log2, 31));
    DFX_RETURN_IF_ERROR(alloc_table(cap_log2, &T, &table_owners, true, &accs_full));
    spill.words = nullptr;
    spill.capacity = 0;
  }
  // one slice per routing window from a resident table, whatever batch width its scan was created with (the result of an
  // aggregate does not depend on it; every slice costs a pass-1 launch)
  if (opt().merge_scan_batches) input->prefer_batch_rows((int64_t)1 << 27);
  for (;;) {
    DeviceBatch b;
    bool has = false;
    DFX_RETURN_IF_ERROR(input->next(&b, &has));
    if (!has) break;
    DFX_RETURN_IF_ERROR(consume_batch(b));
  }
  DFX_RETURN_IF_ERROR(run_held());  // (batches a multi-chunk aggregate was still holding)
  if (kw == 0) {
    uint32_t hc[CTRL_WORDS];
    DFX_RETURN_IF_ERROR(read_ctrl(hc));
    if (hc[CTRL_ERROR]) return error_from_ctrl(hc[CTRL_ERROR]);
  } else {
    DFX_RETURN_IF_ERROR(finish_launched(0, dec.use_partition));  // (partitioned: the last pass 2 ran after the last snapshot -- errors, spilled rows, growth)
    DFX_RETURN_IF_ERROR(routed_shadow_maybe());  // (a query that bound the operand's shadow leaves the table its routed shadow: the next one scans it)
  }
  built = true;
  return Status::OK();
}

// ---- public class -----------------------------------------------------------------------------------
AggregateRelation::AggregateRelation(SchemaInfo schema, std::unique_ptr<Relation> input,
                                     std::vector<dfx_runtime_expr> group, std::vector<dfx_runtime_expr> aggr, OptionOverrides options)
    : schema_(std::move(schema)), impl_(new Impl()) {
  Impl& m = *impl_;
  m.options.overrides = std::move(options);
  m.group = std::move(group);
  for (const dfx_runtime_expr& e : aggr) {  // AVG(x) -> SUM(x), COUNT(x)
    Impl::OutAgg o;
    o.acc = (int)m.aggr.size();
    o.avg = e.is_aggregate && e.agg_func == AGG_AVG;
    o.dtype = e.agg_func == AGG_COUNT ? (int)DFX_UINT64 : e.agg_type;
    o.name = e.name;
    m.outs.push_back(o);
    if (o.avg) {
      dfx_runtime_expr sum = e, cnt = e;
      sum.agg_func = AGG_SUM;
      cnt.agg_func = AGG_COUNT;
      cnt.agg_type = DFX_UINT64;
      m.aggr.push_back(sum);
      m.aggr.push_back(cnt);
    } else {
      m.aggr.push_back(e);
    }
  }
  // Filter -> Aggregate fusion (K7)
  if (input->kind() == REL_FILTER) {
    FilterRelation* f = static_cast<FilterRelation*>(input.get());
    // the predicate joins the scan's fused program only if it fits next to the keys and at least one argument; otherwise
    // (or when the Filter itself needed several programs) the Filter stays a relation of its own below the aggregate
    bool fits = f->single_program();
    if (fits && !f->predicate().is_aggregate) {
      // EVERY accumulator must fit beside the predicate and the keys on its own (setup() splits the accumulators into
      // chunks down to one per program, never below): one that does not would fail the whole query with NotImplemented
      // where the reference -- which has no such limit -- runs it; un-fused, its program holds keys + argument only
      for (size_t a = 0; a < std::max<size_t>(m.aggr.size(), 1) && fits; ++a) {
        ProgramBuilder trial(f->program_schema());  // (string terms count as the Boolean columns they become)
        uint8_t opnd = kNoOperand;
        int dt = 0;
        Status tst = trial.add(f->program_predicate(), f->program_predicate().root, &opnd, &dt);
        for (size_t k = 0; k < m.group.size() && tst.ok(); ++k)
          if (!m.group[k].is_aggregate) tst = trial.add(m.group[k], m.group[k].root, &opnd, &dt);
        if (tst.ok() && a < m.aggr.size() && m.aggr[a].is_aggregate && m.aggr[a].agg_arg >= 0) tst = trial.add(m.aggr[a], m.aggr[a].agg_arg, &opnd, &dt);
        if (program_limit_error(tst)) fits = false;
      }
    }
    if (fits && !f->predicate().is_aggregate) {
      m.has_pred = true;
      m.pred = f->predicate();
      std::unique_ptr<Relation> inner = f->release_input();
      input = std::move(inner);
    }
  }
  m.input = std::move(input);
  m.deferred = m.setup(m.input->schema());
  if (m.deferred.ok()) {  // projection push-down: predicate, key and argument columns only (incl. the Utf8 key sources)
    std::vector<char> needed(m.input->schema().fields.size(), 0);
    for (const Impl::Chunk& ch : m.chunks) mark_columns(&needed, ch.fused.builder->columns());  // every chunk of accumulators reads its own columns from the same batches
    for (const Impl::DictKey& d : m.dicts)
      if (d.src_col >= 0 && d.src_col < (int)needed.size()) needed[d.src_col] = 1;
    for (const Utf8TermSpec& t : m.pred_terms.terms())
      if (t.src_col >= 0 && t.src_col < (int)needed.size()) needed[t.src_col] = 1;
    m.input->require_columns(needed);
  }
  // output schema: group columns then aggregates (aggregate.rs:894-949); context.rs:185 passes
  // Schema::empty(), so derive names/types from the expressions when none is given
  SchemaInfo derived;
  for (size_t k = 0; k < m.group.size(); ++k) {
    Field f;
    f.name = m.group[k].name;
    f.dtype = k < m.key_out_dtype.size() && m.key_out_dtype[k] ? m.key_out_dtype[k] : m.group[k].dtype;
    f.nullable = false;
    derived.fields.push_back(f);
  }
  for (const Impl::OutAgg& o : m.outs) {
    Field f;
    f.name = o.name;
    f.dtype = o.dtype;
    f.nullable = true;
    derived.fields.push_back(f);
  }
  if (schema_.fields.size() == derived.fields.size()) {
    for (size_t i = 0; i < derived.fields.size(); ++i) {
      derived.fields[i].name = schema_.fields[i].name;
    }
  }
  schema_ = derived;
}

AggregateRelation::~AggregateRelation() {}

void AggregateRelation::explain(std::string* out, int depth) const {
  const Impl& m = *impl_;
  if (!m.deferred.ok()) {
    explain_line(out, depth, "Aggregate: error deferred to next(): " + m.deferred.msg);
  } else {
    const DevProgram& P = m.active().builder->program();
    // the row source in words: the launchers' own choice (dfx_row_source.hpp) for the program as built -- no batch is bound, so the
    // scan plan wherever one can be built
    DevFastPlan F = m.active().fast;
    F.plan_mode = m.opt().plan;
    const ScanKernel kernel = m.kw == 0 ? ScanKernel::reduce : ScanKernel::hash_agg;
    const char* shape = row_source_prose(kernel, row_source_without_batch(kernel, P, F, m.kw, m.na(), m.acc_kind(), m.val_xform(),
                                                                           scan_plan_shape_ok(P, F, m.kw, m.na(), m.val_xform())), m.kw);
    if (m.kw == 1 && sig_matches<SigKeyAffSumPred2F64>(P, F, 1, m.na(), m.acc_kind(), m.val_xform())) shape = "static shape KeyAffSumPred2F64 (pass 1 of the partitioned strategy)";
    std::string text = strfmt("Aggregate: %d keys%s, %d accumulators", m.kw_out, m.kw != m.kw_out ? " (as 8 key words)" : "", m.na_total);
    if (m.chunks.size() > 1) text += strfmt(" in %d chunks of <= %d (one fused program each, the same table)", (int)m.chunks.size(), kMaxAggs);
    const bool plan_fuses = m.opt().plan != 0 && m.opt().fast != 0 && scan_plan_shape_ok(P, m.active().fast, m.kw, m.na(), m.val_xform());
    text += !m.has_pred ? ", no predicate" : plan_fuses ? ", Filter below fused into the scan (batches with nulls too: the scan plan judges a null by arrow's comparison rule and counts every surviving slot as valid)"
                                                        : ", Filter below fused into the scan (un-fused for batches with nulls in its columns)";
    text += ", " + explain_program(P) + ", " + shape;
    if (m.kw == 0) text += ", ungrouped reduce (64 partial copies + fold)";
    else if (m.kw == 1) text += ", strategy chosen on the first 2^18 rows: register accumulators (<= 8 groups) / LDS front cache (<= 8192) / table / "
                               "partitioned (>= 16384 groups: pass 1 routes rows to table blocks, pass 2 aggregates blocks in LDS)";
    else text += ", strategy chosen on the first 2^18 rows: register accumulators (<= 8 groups) / LDS front cache (<= 8192) / table";
    if (m.shared_operand())
      text += strfmt("; %d aggregates of ONE operand: the partitioned strategy routes 12-byte rows {hash image, raw operand} while keys are "
                     "narrow and batches have no nulls; pass 2 runs once per accumulator plane with that aggregate's transform "
                     "(agg.shared_planes; 0: one pass 2 over 4096-slot blocks that hold every plane)", m.na());
    if (m.pair_scan()) text += m.pair_planes() ? "; ran the one-value pass 1 with a pass 2 per accumulator plane" : "; ran the pair scan (both operands routed by one scan, a pass 2 per accumulator plane: agg.pair_scan)";
    if (!m.single_chunks.empty() && !m.split_is_shared && !m.pair_scan())
      text += strfmt("; %d aggregates of different operands: if the calibration slice chooses the partitioned strategy, one scan per "
                     "aggregate (its own fused program and accumulator plane over the same keys: 12-byte routed rows, the one-aggregate "
                     "kernels; agg.split_aggregates)", m.na_total);
    if (m.phase == Impl::Phase::PerAggregate) text += strfmt("; ran one scan per aggregate (%d scans per batch: agg.split_aggregates)", (int)m.chunks.size());
    if (m.shadows.key_shadow_launches > 0) text += strfmt("; %lld pass-1 launches read the key from its Int32 shadow (4 bytes of key per row instead of 8: agg.key_shadow)", (long long)m.shadows.key_shadow_launches);
    if (m.shadows.value_shadow_launches > 0) text += strfmt("; %lld of them read the operand from its Float32 shadow as well (every value of the column is exactly its float: 8 bytes per row, agg.value_shadow)", (long long)m.shadows.value_shadow_launches);
    if (m.shadows.row8_launches > 0) text += strfmt("; %lld of those routed 8-byte rows {hash image, Float32 bits} (row8: sixteen rows per 128-byte line, pass 2 widens the bits; agg.routed_row8)", (long long)m.shadows.row8_launches);
    if (m.shadows.routed_shadow_launches > 0) text += strfmt("; %lld launches scanned a window of the table's routed shadow (narrow8_pred: one kernel per window reads the kept 8-byte rows and evaluates the predicate, no pass 1; agg.routed_shadow)", (long long)m.shadows.routed_shadow_launches);
    if (!m.dicts.empty()) text += strfmt(", %d Utf8 keys dictionary-encoded on the device", (int)m.dicts.size());
    if (m.built && m.kw > 0)  // after the input was drained: what actually ran
      text += strfmt("; ran %lld rows: %s, %llu of 2^%d table slots occupied", (long long)m.rows_seen,
                     m.dec.use_partition ? "partitioned" : (m.dec.lds_enabled && m.dec.occupied_known <= 8 && m.opt().fewgroup) ? "few groups (register accumulators or LDS front cache)"
                                     : m.dec.lds_enabled ? "LDS front cache + table" : "table (global atomics)",
                     (unsigned long long)m.dec.occupied_known, 64 - m.T.shift);
    else if (m.built)
      text += strfmt("; ran %lld rows", (long long)m.rows_seen);
    explain_line(out, depth, text);
  }
  if (m.input) m.input->explain(out, depth + 1);
}

Status AggregateRelation::next(DeviceBatch* out, bool* has) {
  *has = false;
  Impl& m = *impl_;
  if (m.done) return Status::OK();  // end_of_results (aggregate.rs:616-618)
  m.done = true;
  if (!m.deferred.ok()) return m.deferred;
  if (m.group.empty() && m.aggr.empty())
    return Status::Err(DFX_INTERNAL_ERROR, "assertion failed: record batch needs at least one column");
  DFX_RETURN_IF_ERROR(m.drain());
  if (m.kw == 0) DFX_RETURN_IF_ERROR(m.emit_ungrouped(out));
  // (Utf8 keys: Utf8Dict::to_utf8 indexes the dictionary with the compacted ids before the scan's total could contradict the host's
  // count -- the table's own count first, one round trip more)
  else DFX_RETURN_IF_ERROR(m.emit_grouped(out, (m.opt().emit_async && m.dicts.empty()) ? (int64_t)m.dec.occupied_known : -1));
  *has = true;
  return Status::OK();
}

}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_aggregate_relation_new(const struct ArrowSchema* schema, struct ArrowArrayStream* input,
                                   const dfx_runtime_expr* const* group_exprs, int32_t n_group,
                                   const dfx_runtime_expr* const* aggr_exprs, int32_t n_aggr,
                                   struct ArrowArrayStream* out, char* err, size_t errlen) {
  return dfx_aggregate_relation_new_with_options(schema, input, group_exprs, n_group, aggr_exprs, n_aggr, nullptr, 0, out, err, errlen);
}

int32_t dfx_aggregate_relation_new_with_options(const struct ArrowSchema* schema, struct ArrowArrayStream* input,
                                                const dfx_runtime_expr* const* group_exprs, int32_t n_group,
                                                const dfx_runtime_expr* const* aggr_exprs, int32_t n_aggr,
                                                const dfx_option* options, int32_t n_options,
                                                struct ArrowArrayStream* out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!out || (n_options > 0 && !options)) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    OptionOverrides ov;
    Status st = parse_option_overrides(options, n_options, &ov);
    if (!st.ok()) return to_c(st, err, errlen);
    std::unique_ptr<Relation> in;
    st = adopt_input_stream(input, &in);
    if (!st.ok()) return to_c(st, err, errlen);
    SchemaInfo si;
    st = schema_from_arrow(schema, &si);
    if (!st.ok()) return to_c(st, err, errlen);
    std::vector<dfx_runtime_expr> g, a;
    for (int i = 0; i < n_group; ++i) g.push_back(*group_exprs[i]);
    for (int i = 0; i < n_aggr; ++i) a.push_back(*aggr_exprs[i]);
    std::unique_ptr<Relation> rel;
    if (needs_distinct_sets(a, in->schema())) {  // COUNT(DISTINCT), MIN / MAX of Utf8: a relation of its own around a plain aggregate (dfx_distinct.cpp)
      st = make_distinct_aggregate(si, std::move(in), std::move(g), std::move(a), std::move(ov), &rel);
      if (!st.ok()) return to_c(st, err, errlen);
      export_relation(std::move(rel), out);
      return DFX_OK;
    }
    rel.reset(new AggregateRelation(si, std::move(in), std::move(g), std::move(a), std::move(ov)));
    export_relation(std::move(rel), out);
    return DFX_OK;
  });
}

}  // extern "C"
