// dfx_distinct.cpp -- the aggregates that read a distinct set: COUNT(DISTINCT x) (deviation D8: the reference declares
// AggregateType::CountDistinct, expression.rs:37, and has no executor for it) and MIN / MAX of a Utf8 column (deviation D10: typed by
// the planner, sqlplanner.rs:309-322, a panic on the downcast in the executor, aggregate.rs:561-603).
//
// The plain AggregateRelation is not touched: a query with such an aggregate becomes
//
//   DistinctAggregateRelation            distinct sets (one per distinct argument), emit + splice
//     AggregateRelation                  the plain aggregates (possibly none: GROUP BY k alone keeps every group)
//       DistinctTap                      pulls a batch, queues the distinct inserts for it, hands it on
//         input
//
// A set is a DevTable with na == 0 whose key is the tuple (group key words, zero padding, canonical argument image), width 1
// ungrouped, kw_out + 1 grouped (five to seven keys padded to eight words).  Growth needs no host synchronisation per batch:
// rows the set cannot take go to a spill list that holds a whole batch, the set's control block is read back one batch behind
// (a kernel writes it to pinned memory), and a set past its load limit or with spilled rows is rehashed into a larger one and
// the spill replayed before the next batch is inserted.  At emit every set counts its tuples per key prefix into a small count
// table, and each group the inner aggregate emits looks its key up there (0 when absent).
//
// MIN(x) / MAX(x) of a Utf8 column x per group is the extremum over the group's distinct values of x: such an aggregate asks for
// the set of its argument column -- the set COUNT_DISTINCT(x) builds, shared with it -- and nothing of it runs per input row.  At
// emit the set's tuples are folded per key prefix into an extrema table, the count table's twin (dfx_k_utf8agg.hip: strings compared
// out of the dictionary), each emitted group looks up its two ids, and the ids become a nullable Utf8 column the way a Utf8 key
// column is built from its ids.
#include "dfx_distinct_impl.hpp"

namespace dfx {
namespace {

// structural identity of an expression subtree: two distinct aggregates with the same argument share one set
void expr_signature(const dfx_runtime_expr& e, int32_t idx, std::string* out) {
  if (idx < 0 || idx >= (int32_t)e.nodes.size()) {
    *out += "()";
    return;
  }
  const dfx_expr_node& n = e.nodes[(size_t)idx];
  *out += strfmt("(%d %d %d %d %d %llx %s ", (int)n.kind, (int)n.op, (int)n.dtype, (int)n.column, (int)n.n_args,
                 (unsigned long long)n.lit.u64, n.name ? n.name : "");
  expr_signature(e, n.left, out);
  expr_signature(e, n.right, out);
  *out += ")";
}

// The type of an aggregate's argument where it can be Utf8: a column's, a literal's, a cast's target (whatever else the compiler
// accepts computes a number or a Boolean).
int argument_type(const dfx_runtime_expr& e, const SchemaInfo& in) {
  if (e.agg_arg < 0 || e.agg_arg >= (int32_t)e.nodes.size()) return DFX_TYPE_NONE;
  const dfx_expr_node& n = e.nodes[(size_t)e.agg_arg];
  if (n.kind == DFX_EXPR_COLUMN) return n.column >= 0 && n.column < (int)in.fields.size() ? in.fields[(size_t)n.column].dtype : (int)DFX_TYPE_NONE;
  return n.kind == DFX_EXPR_LITERAL || n.kind == DFX_EXPR_CAST ? n.dtype : (int)DFX_TYPE_NONE;
}
bool is_utf8_extremum(const dfx_runtime_expr& e, const SchemaInfo& in) {
  return e.is_aggregate && (e.agg_func == AGG_MIN || e.agg_func == AGG_MAX) && argument_type(e, in) == DFX_UTF8;
}

}  // namespace

Status DistinctTap::next(DeviceBatch* out, bool* has) {
  DFX_RETURN_IF_ERROR(input_->next(out, has));
  if (*has) DFX_RETURN_IF_ERROR(owner_->consume(*out));
  return Status::OK();
}

void DistinctTap::require_columns(const std::vector<char>& needed) {
  std::vector<char> u = needed;
  const std::vector<char>& mine = owner_->needed();
  for (size_t i = 0; i < u.size() && i < mine.size(); ++i) u[i] = u[i] || mine[i];
  input_->require_columns(u);
}

// Utf8 column -> its dictionary (one per column, shared by keys and arguments); a new one appends its id column to the bind schema
int DistinctAggregateRelation::dict_of(int col) {
  for (size_t d = 0; d < dicts_.size(); ++d)
    if (dicts_[d].src_col == col) return (int)d;
  DistinctDict d;
  d.src_col = col;
  d.virt_col = (int)bind_schema_.fields.size();
  Field f;
  f.name = "__distinct_ids_" + std::to_string(col);
  f.dtype = DFX_UINT64;
  f.nullable = true;
  bind_schema_.fields.push_back(f);
  dicts_.push_back(std::move(d));
  return (int)dicts_.size() - 1;
}

// the Utf8 input column that node idx of e names, -1 when it is anything else
int DistinctAggregateRelation::utf8_column(const dfx_runtime_expr& e, int32_t idx) const {
  if (idx < 0 || idx >= (int32_t)e.nodes.size()) return -1;
  const dfx_expr_node& r = e.nodes[(size_t)idx];
  if (r.kind != DFX_EXPR_COLUMN || r.column < 0 || r.column >= (int)bind_schema_.fields.size()) return -1;
  return bind_schema_.fields[(size_t)r.column].dtype == DFX_UTF8 ? r.column : -1;
}

// A Utf8 argument reaches its set as the ids of its column's dictionary, so it has to BE a column: the one check of that, for
// COUNT_DISTINCT and the Utf8 extrema alike.  *col: the column, -1 for an argument of another type.
Status DistinctAggregateRelation::utf8_argument(const dfx_runtime_expr& e, const char* what, int* col) const {
  *col = utf8_column(e, e.agg_arg);
  if (*col < 0 && argument_type(e, bind_schema_) == DFX_UTF8)
    return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("%s of a Utf8 expression other than a bare column", what));
  return Status::OK();
}

// establishes key_dict_ and p->group_rw: the group keys as the sets' programs read them, Utf8 columns through a dictionary
void DistinctAggregateRelation::rewrite_utf8_keys(Planning* p) {
  p->group_rw = group_;
  key_dict_.assign((size_t)kw_out_, -1);
  for (int k = 0; k < kw_out_; ++k) {
    if (group_[k].is_aggregate) continue;
    const int c = utf8_column(group_[k], group_[k].root);
    if (c < 0) continue;
    key_dict_[(size_t)k] = dict_of(c);
    p->group_rw[k].nodes[(size_t)group_[k].root].column = dicts_[(size_t)key_dict_[(size_t)k]].virt_col;
    p->group_rw[k].dtype = DFX_UINT64;
  }
}

// establishes where every output column comes from (out_src_ / out_role_, the sets' want_*): plain aggregates go to the inner
// aggregate (p->plain), the others to the set of their argument (p->set_of), shared by equal arguments
Status DistinctAggregateRelation::assign_aggregates_to_sets(Planning* p) {
  p->set_of.assign(p->aggr.size(), -1);
  for (size_t j = 0; j < p->aggr.size(); ++j) {
    const dfx_runtime_expr& e = p->aggr[j];
    const bool extremum = is_utf8_extremum(e, bind_schema_);
    if (!extremum && !(e.is_aggregate && e.agg_func == AGG_COUNT_DISTINCT)) {
      out_src_.push_back(kw_out_ + (int)p->plain.size());
      out_role_.push_back(ROLE_PLAIN);
      p->plain.push_back(e);
      continue;
    }
    int c = -1;
    DFX_RETURN_IF_ERROR(utf8_argument(e, extremum ? "MIN/MAX" : "COUNT_DISTINCT", &c));
    if (extremum && e.agg_type != DFX_UTF8)  // downcast_ref::<T>().unwrap() by the declared type (aggregate.rs:347, :563), as for the numeric types
      return Status::Err(DFX_INTERNAL_ERROR, strfmt("called `Option::unwrap()` on a `None` value (aggregate argument is %s, declared %s)",
                                                    dtype_name(DFX_UTF8), dtype_name(e.agg_type)));
    std::string sig;
    expr_signature(e, e.agg_arg, &sig);
    int si = -1;
    for (size_t s = 0; s < sets_.size(); ++s)
      if (sets_[s]->signature == sig) si = (int)s;
    if (si < 0) {
      std::unique_ptr<DistinctSet> S(new DistinctSet());
      S->signature = sig;
      S->kw = kw_out_ == 0 ? 1 : kw_out_ + 1 <= 4 ? kw_out_ + 1 : kMaxKeys;
      S->builder.reset(new ProgramBuilder(bind_schema_));  // (bind_schema_ may still grow: the builder keeps a reference)
      sets_.push_back(std::move(S));
      si = (int)sets_.size() - 1;
      dfx_runtime_expr arg = e;
      if (c >= 0) {
        sets_[(size_t)si]->arg_col = c;
        sets_[(size_t)si]->arg_dict = dict_of(c);
        arg.nodes[(size_t)e.agg_arg].column = dicts_[(size_t)sets_[(size_t)si]->arg_dict].virt_col;
      }
      p->aggr[j] = arg;  // (the program below reads the rewritten argument)
    }
    p->set_of[j] = si;
    out_src_.push_back(-1 - si);
    out_role_.push_back(!extremum ? ROLE_COUNT : e.agg_func == AGG_MIN ? ROLE_MIN : ROLE_MAX);
    DistinctSet& S = *sets_[(size_t)si];
    S.want_count = S.want_count || !extremum;
    S.want_min = S.want_min || (extremum && e.agg_func == AGG_MIN);
    S.want_max = S.want_max || (extremum && e.agg_func == AGG_MAX);
  }
  return Status::OK();
}

// establishes every set's fused program (keys + argument, no predicate) and the input columns the sets read (needed_)
Status DistinctAggregateRelation::build_set_programs(const Planning& p) {
  for (size_t s = 0; s < sets_.size(); ++s) {
    DistinctSet& S = *sets_[s];
    const dfx_runtime_expr* arg = nullptr;
    for (size_t j = 0; j < p.aggr.size() && !arg; ++j)
      if (p.set_of[j] == (int)s) arg = &p.aggr[j];
    memset(&S.plan, 0, sizeof(S.plan));
    memset(&S.fast, 0, sizeof(S.fast));
    S.plan.pred = kNoOperand;
    for (int k = 0; k < kw_out_; ++k) {
      if (group_[k].is_aggregate) return Status::Err(DFX_INTERNAL_ERROR, "explicit panic: get_func() on an aggregate expression");
      int dt = 0;
      DFX_RETURN_IF_ERROR(S.builder->add(p.group_rw[k], p.group_rw[k].root, &S.plan.key[k], &dt));
      if (!dtype_is_int(dt)) return Status::Err(DFX_EXECUTION_ERROR, "Unsupported GROUP BY data type");  // aggregate.rs:848-850
      S.plan.key_dtype[k] = (uint8_t)dt;
    }
    int dt = 0;
    DFX_RETURN_IF_ERROR(S.builder->add(*arg, arg->agg_arg, &S.plan.arg[0], &dt));
    S.arg_dtype = dt;
    S.plan.arg_dtype[0] = (uint8_t)dt;
    S.builder->build_fast(kNoOperand, S.plan.key, kw_out_, S.plan.arg, 1, &S.fast);
    for (int ci : S.builder->columns())
      if (ci >= 0 && ci < (int)needed_.size()) needed_[(size_t)ci] = 1;
  }
  for (const DistinctDict& d : dicts_) needed_[(size_t)d.src_col] = 1;
  return Status::OK();
}

// establishes hidden_count_ and that the inner aggregate has something to run.  Ungrouped, COUNT(x) of every set's argument rides
// along, so that input with nothing to count gives what COUNT(x) gives; with no aggregate at all a COUNT(1) only drains the input.
void DistinctAggregateRelation::add_hidden_counts(Planning* p) {
  if (kw_out_ != 0) return;
  for (size_t s = 0; s < sets_.size(); ++s) {
    for (size_t j = 0; j < p->aggr.size(); ++j) {
      if (p->set_of[j] != (int)s) continue;
      dfx_runtime_expr cnt = p->orig[j];
      if (utf8_column(cnt, cnt.agg_arg) >= 0) {  // (COUNT takes no Utf8 argument: the set's count is always valid)
        hidden_count_.push_back(-1);
        break;
      }
      cnt.agg_func = AGG_COUNT;
      cnt.agg_type = DFX_UINT64;
      cnt.dtype = DFX_UINT64;
      cnt.name = "__distinct_count_" + std::to_string(s);
      hidden_count_.push_back((int)p->plain.size());
      p->plain.push_back(cnt);
      break;
    }
  }
  if (p->plain.empty()) {  // the inner aggregate still drains the input: COUNT(1), not emitted
    dfx_runtime_expr one;
    dfx_expr_node lit;
    memset(&lit, 0, sizeof(lit));
    lit.kind = DFX_EXPR_LITERAL;
    lit.dtype = DFX_INT64;
    lit.left = lit.right = lit.column = -1;
    lit.lit.i64 = 1;
    dfx_expr_node fn = lit;
    fn.kind = DFX_EXPR_AGGREGATE_FUNCTION;
    fn.dtype = DFX_UINT64;
    fn.left = 0;
    fn.n_args = 1;
    one.nodes = {lit, fn};
    one.strings.assign(2, std::string());
    one.has_name.assign(2, 0);
    one.rebind();
    one.root = 1;
    one.is_aggregate = true;
    one.agg_func = AGG_COUNT;
    one.agg_arg = 0;
    one.agg_type = one.dtype = DFX_UINT64;
    one.name = "__distinct_rows";
    p->plain.push_back(one);
  }
}

// establishes schema_: keys, then the aggregates in their order (distinct counts UInt64, Utf8 extrema Utf8, named like the others)
void DistinctAggregateRelation::derive_schema(const Planning& p, const SchemaInfo& caller) {
  const SchemaInfo& is = inner_->schema();
  SchemaInfo derived;
  for (int k = 0; k < kw_out_ && k < (int)is.fields.size(); ++k) derived.fields.push_back(is.fields[(size_t)k]);
  for (size_t j = 0; j < p.aggr.size(); ++j) {
    const int src = out_src_[j];
    if (src >= 0 && src < (int)is.fields.size()) {
      derived.fields.push_back(is.fields[(size_t)src]);
    } else {
      Field f;
      f.name = p.aggr[j].name;
      f.dtype = out_role_[j] == ROLE_COUNT ? DFX_UINT64 : DFX_UTF8;
      f.nullable = true;
      derived.fields.push_back(f);
    }
  }
  if (caller.fields.size() == derived.fields.size())
    for (size_t i = 0; i < derived.fields.size(); ++i) derived.fields[i].name = caller.fields[i].name;
  schema_ = derived;
}

Status DistinctAggregateRelation::init(SchemaInfo caller, std::unique_ptr<Relation> input, std::vector<dfx_runtime_expr> group,
                                       std::vector<dfx_runtime_expr> aggr, OptionOverrides options) {
  opt_.overrides = options;
  group_ = group;
  kw_out_ = (int)group.size();
  if (kw_out_ > kMaxKeys - 1) {
    bool counts = false;
    for (const dfx_runtime_expr& e : aggr) counts = counts || (e.is_aggregate && e.agg_func == AGG_COUNT_DISTINCT);
    return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("%s with more than %d GROUP BY expressions (the distinct set's tuple is "
                                                   "the key words and one more, at most %d words)", counts ? "COUNT_DISTINCT" : "MIN/MAX of Utf8",
                                                   kMaxKeys - 1, kMaxKeys));
  }
  bind_schema_ = input->schema();
  needed_.assign(bind_schema_.fields.size(), 0);
  Planning p;
  p.orig = aggr;
  p.aggr = std::move(aggr);
  rewrite_utf8_keys(&p);
  DFX_RETURN_IF_ERROR(assign_aggregates_to_sets(&p));
  DFX_RETURN_IF_ERROR(build_set_programs(p));
  add_hidden_counts(&p);
  std::unique_ptr<DistinctTap> tap(new DistinctTap(std::move(input), this));
  tap_ = tap.get();
  inner_.reset(new AggregateRelation(SchemaInfo(), std::move(tap), group, p.plain, options));
  derive_schema(p, caller);
  return Status::OK();
}

void DistinctAggregateRelation::explain(std::string* out, int depth) const {
  bool counts = false, extrema = false;
  for (const auto& S : sets_) {
    counts = counts || S->want_count;
    extrema = extrema || S->want_min || S->want_max;
  }
  const char* readers = !extrema ? "COUNT_DISTINCT" : !counts ? "Utf8 MIN/MAX" : "COUNT_DISTINCT + Utf8 MIN/MAX";
  std::string text = strfmt("DistinctAggregate: %d %s set%s of %d-word tuples (%s%s), ", (int)sets_.size(), readers,
                            sets_.size() == 1 ? "" : "s", sets_.empty() ? 0 : sets_[0]->kw,
                            kw_out_ == 0 ? "argument" : "group keys + argument", kw_out_ > 3 ? ", keys padded to 7 words" : "");
  bool plan_shape = false;
  const uint8_t xf[kMaxAggs] = {VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW, VT_RAW};
  for (const auto& S : sets_)
    plan_shape = plan_shape || (opt().plan != 0 && opt().fast != 0 && S->fast.valid && scan_plan_shape_ok(S->builder->program(), S->fast, kw_out_, 1, xf));
  text += plan_shape ? "k_distinct_insert: scan plan (PlanPolicy) for plain columns, else the SSA interpreter"
                     : "k_distinct_insert: SSA interpreter";
  if (!sets_.empty()) text += ", " + explain_program(sets_[0]->builder->program());
  if (!dicts_.empty()) text += strfmt(", %d Utf8 columns dictionary-encoded on the device", (int)dicts_.size());
  if (extrema) {  // the Utf8 extrema beside the set they read
    text += "; Utf8 extrema folded from the sets at emit (k_utf8_extrema_fold, strings compared out of the dictionary):";
    const char* sep = " ";
    for (size_t si = 0; si < sets_.size(); ++si) {
      const DistinctSet& S = *sets_[si];
      if (!S.want_min && !S.want_max) continue;
      const std::string by = std::string(S.want_count ? "COUNT_DISTINCT " : "") + (S.want_min ? "MIN " : "") + (S.want_max ? "MAX " : "");
      text += sep + strfmt("set %d of #%d read by %s", (int)si, S.arg_col, by.substr(0, by.size() - 1).c_str());
      sep = ", ";
    }
  }
  text += "; the plain aggregates run below (a Filter under it is compacted by FilterRelation, not fused)";
  if (done_) text += strfmt("; ran %lld rows, %lld set growths (rehash), %lld spilled rows replayed", (long long)rows_seen_, growths_, spill_rows_);
  explain_line(out, depth, text);
  inner_->explain(out, depth + 1);
}

std::string DistinctAggregateRelation::exchange_refusal() const {
  bool counts = false, extrema = false;
  for (const auto& S : sets_) {
    counts = counts || S->want_count;
    extrema = extrema || S->want_min || S->want_max;
  }
  std::string msg;
  if (counts) msg = "COUNT_DISTINCT: distinct counts do not add across ranks (the exchange of (key, value) tuples is not implemented)";
  if (extrema) msg += std::string(counts ? "; " : "") + "MIN/MAX of Utf8: the extrema are folded from a distinct set of (key, string id) tuples over a rank-local "
                                                        "dictionary (the exchange of such tuples is not implemented)";
  return msg;
}

bool needs_distinct_sets(const std::vector<dfx_runtime_expr>& aggr, const SchemaInfo& input_schema) {
  for (const dfx_runtime_expr& e : aggr)
    if ((e.is_aggregate && e.agg_func == AGG_COUNT_DISTINCT) || is_utf8_extremum(e, input_schema)) return true;
  return false;
}

Status distinct_sets_exchange_refusal(const Relation* r) {
  if (!r || r->kind() != REL_DISTINCT_AGGREGATE) return Status::OK();
  return Status::Err(DFX_NOT_IMPLEMENTED, static_cast<const DistinctAggregateRelation*>(r)->exchange_refusal());
}

Status make_distinct_aggregate(SchemaInfo schema, std::unique_ptr<Relation> input, std::vector<dfx_runtime_expr> group,
                               std::vector<dfx_runtime_expr> aggr, OptionOverrides options, std::unique_ptr<Relation>* out) {
  std::unique_ptr<DistinctAggregateRelation> rel(new DistinctAggregateRelation());
  DFX_RETURN_IF_ERROR(rel->init(std::move(schema), std::move(input), std::move(group), std::move(aggr), std::move(options)));
  *out = std::move(rel);
  return Status::OK();
}

}  // namespace dfx
