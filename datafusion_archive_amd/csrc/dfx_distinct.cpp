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
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "dfx_relation.hpp"

namespace dfx {
namespace {

constexpr uint64_t kSetProbes = 256;

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

Status upload_bytes(const void* host, size_t bytes, std::shared_ptr<void>* dev) {
  Status st;
  *dev = device_alloc(std::max<size_t>(bytes, 8), &st);
  if (!*dev) return st;
  // (on the library's stream: it is non-blocking, a plain hipMemcpy would not wait for its work)
  DFX_HIP(hipMemcpyAsync(dev->get(), host, bytes, hipMemcpyHostToDevice, ctx().stream));
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  return Status::OK();
}

// An emit-time table keyed by the key prefix of a set's tuples (the set's width, the argument word zeroed): the count table, the
// extrema table.  At most half full -- a set of `occupied` tuples has at most as many prefixes -- with probing over the whole
// table, and `planes` zeroed accumulator planes.  Ungrouped (kw == 1) the prefix has no words: one entry, stride 1, no keys.
struct EmitTable {
  DevTable T;
  std::vector<std::shared_ptr<void>> owners;
};
Status alloc_emit_table(int kw, uint64_t occupied, int planes, EmitTable* E) {
  hipStream_t s = ctx().stream;
  Status st;
  DevTable& T = E->T;
  memset(&T, 0, sizeof(T));
  int lg = 10;
  while ((1ull << lg) < occupied * 2 + 2 && lg < 34) ++lg;
  const uint64_t cap = 1ull << lg;
  T.kw = kw;
  T.na = planes;
  T.stride = kw == 1 ? 1 : cap + 64;
  if (kw > 1) {
    T.mask = cap - 1;
    T.shift = 64 - lg;
    T.load_limit = cap;
    T.max_probe = (int)std::min<uint64_t>(cap, 1u << 30);
    T.block_mask = (uint32_t)(cap - 1);
    auto keys = device_alloc(sizeof(uint64_t) * T.stride * (size_t)kw, &st);
    if (!keys) return st;
    auto state = device_alloc(sizeof(uint32_t) * T.stride, &st);
    if (!state) return st;
    T.keys = (uint64_t*)keys.get();
    T.state = (uint32_t*)state.get();
    E->owners.push_back(keys);
    E->owners.push_back(state);
    DFX_HIP(hipMemsetAsync(T.state, 0, sizeof(uint32_t) * T.stride, s));
  }
  auto accs = device_alloc(sizeof(uint64_t) * T.stride * (size_t)planes, &st);
  if (!accs) return st;
  auto ctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
  if (!ctrl) return st;
  T.accs = (uint64_t*)accs.get();
  T.ctrl = (uint32_t*)ctrl.get();
  E->owners.push_back(accs);
  E->owners.push_back(ctrl);
  for (int a = 0; a < planes; ++a) {
    T.acc_kind[a] = ACC_ADD_U64;
    T.val_xform[a] = VT_RAW;
  }
  DFX_HIP(hipMemsetAsync(T.accs, 0, sizeof(uint64_t) * T.stride * (size_t)planes, s));
  DFX_HIP(hipMemsetAsync(T.ctrl, 0, sizeof(uint32_t) * CTRL_WORDS, s));
  return Status::OK();
}

// a Utf8 column's device dictionary (the dict_* kernels, as the GROUP BY's Utf8 keys use them): strings -> stable UInt64 ids
struct Dict {
  int src_col = 0;   // the Utf8 column of the input schema
  int virt_col = 0;  // its id column in the bind schema
  DevDict D;
  std::shared_ptr<void> state, hash, sid, str_off, str_len, pool, cursors;
  uint64_t ids_used = 0, pool_used = 0;
  bool allocated = false;

  Status alloc(int slots_log2, uint64_t pool_cap, bool keep) {
    hipStream_t s = ctx().stream;
    const uint64_t slots = 1ull << slots_log2, id_cap = slots / 2;
    Status st;
    auto dstate = device_alloc(sizeof(uint32_t) * slots, &st);
    if (!dstate) return st;
    auto h = device_alloc(sizeof(uint64_t) * slots, &st);
    if (!h) return st;
    auto sd = device_alloc(sizeof(uint64_t) * slots, &st);
    if (!sd) return st;
    auto so = device_alloc(sizeof(uint64_t) * id_cap, &st);
    if (!so) return st;
    auto sl = device_alloc(sizeof(uint32_t) * id_cap, &st);
    if (!sl) return st;
    auto pl = device_alloc(std::max<uint64_t>(pool_cap, 64), &st);
    if (!pl) return st;
    auto cur = device_alloc(sizeof(uint64_t) * DICT_WORDS, &st);
    if (!cur) return st;
    DFX_HIP(hipMemsetAsync(dstate.get(), 0, sizeof(uint32_t) * slots, s));
    if (keep && allocated) {
      if (pool_used) DFX_HIP(hipMemcpyAsync(pl.get(), pool.get(), pool_used, hipMemcpyDeviceToDevice, s));
      if (ids_used) {
        DFX_HIP(hipMemcpyAsync(so.get(), str_off.get(), sizeof(uint64_t) * ids_used, hipMemcpyDeviceToDevice, s));
        DFX_HIP(hipMemcpyAsync(sl.get(), str_len.get(), sizeof(uint32_t) * ids_used, hipMemcpyDeviceToDevice, s));
      }
    } else {
      ids_used = pool_used = 0;
    }
    const uint64_t hc[DICT_WORDS] = {pool_used, ids_used, 0, 0};
    DFX_HIP(hipMemcpyAsync(cur.get(), hc, sizeof(hc), hipMemcpyHostToDevice, s));
    DFX_HIP(hipStreamSynchronize(s));  // hc is a stack buffer; the old arrays are released below
    state = dstate; hash = h; sid = sd; str_off = so; str_len = sl; pool = pl; cursors = cur;
    D.state = (uint32_t*)dstate.get();
    D.hash = (uint64_t*)h.get();
    D.sid = (uint64_t*)sd.get();
    D.str_off = (uint64_t*)so.get();
    D.str_len = (uint32_t*)sl.get();
    D.pool = (uint8_t*)pl.get();
    D.cursors = (uint64_t*)cur.get();
    D.mask = slots - 1;
    D.shift = 64 - slots_log2;
    D.id_cap = id_cap;
    D.pool_cap = std::max<uint64_t>(pool_cap, 64);
    allocated = true;
    if (ids_used) DFX_HIP(launch_dict_rebuild(D, ids_used, s));
    return Status::OK();
  }

  // ids of n strings (grows and re-encodes on overflow); the id column keeps the strings' validity
  Status encode(const DeviceColumn& src, int64_t n, int capacity_log2, DeviceColumn* ids_col) {
    hipStream_t s = ctx().stream;
    Status st;
    auto ids = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(n, 1), &st);
    if (!ids) return st;
    if (!allocated) {
      int lg = capacity_log2 > 0 ? capacity_log2 : 16;
      lg = std::max(4, std::min(lg, 30));
      DFX_RETURN_IF_ERROR(alloc(lg, std::max<uint64_t>((uint64_t)src.data_bytes * 2, 1u << 16), false));
    }
    for (int attempt = 0; n > 0; ++attempt) {
      if (attempt > 16) return Status::Err(DFX_INTERNAL_ERROR, "Utf8 dictionary does not converge");
      DFX_HIP(launch_dict_encode(src.offsets, src.data, n, D, ids_used, (uint64_t*)ids.get(), s));
      uint64_t hc[DICT_WORDS];
      DFX_HIP(hipMemcpyAsync(hc, D.cursors, sizeof(hc), hipMemcpyDeviceToHost, s));
      DFX_HIP(hipStreamSynchronize(s));
      if (hc[DICT_OVERFLOW] == 2) return Status::Err(DFX_INTERNAL_ERROR, "Utf8 dictionary: slot claim timed out");
      if (hc[DICT_OVERFLOW] == 0) {
        ids_used = hc[DICT_IDS];
        pool_used = hc[DICT_POOL];
        break;
      }
      int lg = 64 - D.shift;
      const uint64_t want_ids = std::max<uint64_t>(hc[DICT_IDS], ids_used + 1);
      while ((1ull << lg) / 2 < want_ids * 2 && lg < 31) ++lg;
      lg = std::min(31, std::max(lg, 64 - D.shift + 2));
      const uint64_t want_pool = std::max<uint64_t>(hc[DICT_POOL], pool_used + (uint64_t)src.data_bytes) * 2;
      DFX_RETURN_IF_ERROR(alloc(lg, std::max<uint64_t>(want_pool, D.pool_cap), true));
    }
    ids_col->dtype = DFX_UINT64;
    ids_col->length = n;
    ids_col->values = ids.get();
    ids_col->null_count = src.null_count;
    ids_col->validity = src.null_count ? src.validity : nullptr;
    ids_col->bit_offset = src.bit_offset;
    ids_col->offsets = nullptr;
    ids_col->data = nullptr;
    ids_col->owners.clear();
    ids_col->owners.push_back(ids);
    ids_col->owners.insert(ids_col->owners.end(), src.owners.begin(), src.owners.end());  // (the validity bitmap)
    return Status::OK();
  }
};

// one distinct set: the tuples of one distinct argument
struct DistinctSet {
  std::string signature;
  std::unique_ptr<ProgramBuilder> builder;
  DevAggPlan plan;
  DevFastPlan fast;
  int arg_dtype = 0;
  int kw = 1;  // tuple words
  DevTable T;
  std::vector<std::shared_ptr<void>> owners;  // keys, state, ctrl
  DevRows spill;
  std::shared_ptr<void> spill_owner;
  std::shared_ptr<void> snap;  // pinned: the control block after the last insert
  hipEvent_t snap_ev = nullptr;
  bool snap_pending = false;
  int64_t snap_rows = 0;
  bool plan_kernel = false;  // the last insert ran the scan-plan flavour
  // who reads the set at emit: COUNT_DISTINCT its tuple counts, a Utf8 MIN / MAX the extrema of its argument's strings
  bool want_count = false, want_min = false, want_max = false;
  int arg_col = -1;   // the argument when it is a bare Utf8 column ...
  int arg_dict = -1;  // ... and its dictionary
  DistinctSet() {
    memset(&T, 0, sizeof(T));
    memset(&spill, 0, sizeof(spill));
  }
  ~DistinctSet() {
    if (snap_ev) (void)hipEventDestroy(snap_ev);
  }
};

class DistinctAggregateRelation;

// between the input and the inner aggregate: every batch passes through consume() on its way up
class DistinctTap : public Relation {
 public:
  DistinctTap(std::unique_ptr<Relation> input, DistinctAggregateRelation* owner) : input_(std::move(input)), owner_(owner) {}
  RelationKind kind() const override { return REL_DISTINCT_TAP; }
  Status next(DeviceBatch* out, bool* has) override;
  const SchemaInfo& schema() const override { return input_->schema(); }
  void require_columns(const std::vector<char>& needed) override;
  void explain(std::string* out, int depth) const override { input_->explain(out, depth); }  // (no line of its own)
  ScanMemo* scan_memo() override { return input_->scan_memo(); }
  void prefer_batch_rows(int64_t rows) override { input_->prefer_batch_rows(rows); }
  void host_stream_options(const HostStreamOptions& o) override { input_->host_stream_options(o); }
  Relation* input() const { return input_.get(); }

 private:
  std::unique_ptr<Relation> input_;
  DistinctAggregateRelation* owner_;
};

class DistinctAggregateRelation : public Relation {
 public:
  RelationKind kind() const override { return REL_DISTINCT_AGGREGATE; }
  Status next(DeviceBatch* out, bool* has) override;
  const SchemaInfo& schema() const override { return schema_; }
  void explain(std::string* out, int depth) const override;

  Status init(SchemaInfo caller, std::unique_ptr<Relation> input, std::vector<dfx_runtime_expr> group,
              std::vector<dfx_runtime_expr> aggr, OptionOverrides options);
  Status consume(const DeviceBatch& b);
  const std::vector<char>& needed() const { return needed_; }
  std::string exchange_refusal() const;

 private:
  SchemaInfo schema_;
  SchemaInfo bind_schema_;
  std::unique_ptr<AggregateRelation> inner_;
  DistinctTap* tap_ = nullptr;  // owned by inner_
  int kw_out_ = 0;
  std::vector<dfx_runtime_expr> group_;
  std::vector<int> key_dict_;  // per GROUP BY key: index into dicts_ (-1: not Utf8)
  std::vector<Dict> dicts_;
  std::vector<std::unique_ptr<DistinctSet>> sets_;
  // output column j: inner column (>= 0) or distinct set (-1 - set), of which it reads out_role_[j]
  std::vector<int> out_src_;
  enum Role { ROLE_PLAIN = 0, ROLE_COUNT, ROLE_MIN, ROLE_MAX };
  std::vector<int> out_role_;
  std::vector<int> hidden_count_;  // ungrouped: per set, the inner column of its COUNT(x)
  std::vector<char> needed_;
  mutable OperatorOptions opt_;
  bool done_ = false;
  int64_t rows_seen_ = 0;
  long long growths_ = 0, spill_rows_ = 0;  // this operator's share of distinct_set_growths / distinct_spill_rows

  const AggOptions& opt() const { return opt_.get(); }
  Status alloc_set(DistinctSet& S, int cap_log2);
  Status ensure_spill(DistinctSet& S, int64_t rows);
  Status settle(DistinctSet& S, const uint32_t* hc, int64_t rows, bool synced);
  Status grow(DistinctSet& S, uint64_t occupied, uint64_t spilled);
  Status read_ctrl(DistinctSet& S, uint32_t* hc);
  Status emitted_keys(const DeviceBatch& inner_out, DevDistinctKeys* K, std::vector<DeviceColumn>* ids);
  Status emit_counts(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* col, uint64_t* ungrouped_total);
  Status emit_extrema(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* min_col, DeviceColumn* max_col);
};

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

Status DistinctAggregateRelation::init(SchemaInfo caller, std::unique_ptr<Relation> input, std::vector<dfx_runtime_expr> group,
                                       std::vector<dfx_runtime_expr> aggr, OptionOverrides options) {
  opt_.overrides = options;
  group_ = group;
  kw_out_ = (int)group.size();
  const SchemaInfo& in_schema = input->schema();
  if (kw_out_ > kMaxKeys - 1) {
    bool counts = false;
    for (const dfx_runtime_expr& e : aggr) counts = counts || (e.is_aggregate && e.agg_func == AGG_COUNT_DISTINCT);
    return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("%s with more than %d GROUP BY expressions (the distinct set's tuple is "
                                                   "the key words and one more, at most %d words)", counts ? "COUNT_DISTINCT" : "MIN/MAX of Utf8",
                                                   kMaxKeys - 1, kMaxKeys));
  }
  bind_schema_ = in_schema;
  needed_.assign(in_schema.fields.size(), 0);
  auto dict_of = [&](int col) -> int {  // Utf8 column -> its dictionary (one per column, shared by keys and arguments)
    for (size_t d = 0; d < dicts_.size(); ++d)
      if (dicts_[d].src_col == col) return (int)d;
    Dict d;
    memset(&d.D, 0, sizeof(d.D));
    d.src_col = col;
    d.virt_col = (int)bind_schema_.fields.size();
    Field f;
    f.name = "__distinct_ids_" + std::to_string(col);
    f.dtype = DFX_UINT64;
    f.nullable = true;
    bind_schema_.fields.push_back(f);
    dicts_.push_back(std::move(d));
    return (int)dicts_.size() - 1;
  };
  auto utf8_column = [&](const dfx_runtime_expr& e, int32_t idx) -> int {
    if (idx < 0 || idx >= (int32_t)e.nodes.size()) return -1;
    const dfx_expr_node& r = e.nodes[(size_t)idx];
    if (r.kind != DFX_EXPR_COLUMN || r.column < 0 || r.column >= (int)in_schema.fields.size()) return -1;
    return in_schema.fields[(size_t)r.column].dtype == DFX_UTF8 ? r.column : -1;
  };
  // A Utf8 argument reaches its set as the ids of its column's dictionary, so it has to BE a column: the one check of that, for
  // COUNT_DISTINCT and the Utf8 extrema alike.  *col: the column, -1 for an argument of another type.
  auto utf8_argument = [&](const dfx_runtime_expr& e, const char* what, int* col) -> Status {
    *col = utf8_column(e, e.agg_arg);
    if (*col < 0 && argument_type(e, in_schema) == DFX_UTF8)
      return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("%s of a Utf8 expression other than a bare column", what));
    return Status::OK();
  };
  // group keys as the GROUP BY reads them: Utf8 columns through a dictionary
  std::vector<dfx_runtime_expr> group_rw = group;
  key_dict_.assign((size_t)kw_out_, -1);
  for (int k = 0; k < kw_out_; ++k) {
    if (group[k].is_aggregate) continue;
    const int c = utf8_column(group[k], group[k].root);
    if (c < 0) continue;
    key_dict_[(size_t)k] = dict_of(c);
    group_rw[k].nodes[(size_t)group[k].root].column = dicts_[(size_t)key_dict_[(size_t)k]].virt_col;
    group_rw[k].dtype = DFX_UINT64;
  }
  // aggregates: plain ones go to the inner aggregate, the others to the set of their argument (shared by equal arguments)
  const std::vector<dfx_runtime_expr> orig = aggr;  // (arguments of Utf8 columns are rewritten to their id columns below)
  std::vector<dfx_runtime_expr> plain;
  std::vector<int> set_of(aggr.size(), -1);
  for (size_t j = 0; j < aggr.size(); ++j) {
    const dfx_runtime_expr& e = aggr[j];
    const bool extremum = is_utf8_extremum(e, in_schema);
    if (!extremum && !(e.is_aggregate && e.agg_func == AGG_COUNT_DISTINCT)) {
      out_src_.push_back(kw_out_ + (int)plain.size());
      out_role_.push_back(ROLE_PLAIN);
      plain.push_back(e);
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
      aggr[j] = arg;  // (the program below reads the rewritten argument)
    }
    set_of[j] = si;
    out_src_.push_back(-1 - si);
    out_role_.push_back(!extremum ? ROLE_COUNT : e.agg_func == AGG_MIN ? ROLE_MIN : ROLE_MAX);
    DistinctSet& S = *sets_[(size_t)si];
    S.want_count = S.want_count || !extremum;
    S.want_min = S.want_min || (extremum && e.agg_func == AGG_MIN);
    S.want_max = S.want_max || (extremum && e.agg_func == AGG_MAX);
  }
  // the sets' fused programs: keys + argument, no predicate
  for (size_t s = 0; s < sets_.size(); ++s) {
    DistinctSet& S = *sets_[s];
    const dfx_runtime_expr* arg = nullptr;
    for (size_t j = 0; j < aggr.size() && !arg; ++j)
      if (set_of[j] == (int)s) arg = &aggr[j];
    memset(&S.plan, 0, sizeof(S.plan));
    memset(&S.fast, 0, sizeof(S.fast));
    S.plan.pred = kNoOperand;
    for (int k = 0; k < kw_out_; ++k) {
      if (group[k].is_aggregate) return Status::Err(DFX_INTERNAL_ERROR, "explicit panic: get_func() on an aggregate expression");
      int dt = 0;
      DFX_RETURN_IF_ERROR(S.builder->add(group_rw[k], group_rw[k].root, &S.plan.key[k], &dt));
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
  for (const Dict& d : dicts_) needed_[(size_t)d.src_col] = 1;
  // ungrouped: COUNT(x) of every set's argument rides along, so that input with nothing to count gives what COUNT(x) gives
  if (kw_out_ == 0) {
    for (size_t s = 0; s < sets_.size(); ++s) {
      for (size_t j = 0; j < aggr.size(); ++j) {
        if (set_of[j] != (int)s) continue;
        dfx_runtime_expr cnt = orig[j];
        if (utf8_column(cnt, cnt.agg_arg) >= 0) {  // (COUNT takes no Utf8 argument: the set's count is always valid)
          hidden_count_.push_back(-1);
          break;
        }
        cnt.agg_func = AGG_COUNT;
        cnt.agg_type = DFX_UINT64;
        cnt.dtype = DFX_UINT64;
        cnt.name = "__distinct_count_" + std::to_string(s);
        hidden_count_.push_back((int)plain.size());
        plain.push_back(cnt);
        break;
      }
    }
  }
  if (kw_out_ == 0 && plain.empty()) {  // the inner aggregate still drains the input: COUNT(1), not emitted
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
    plain.push_back(one);
  }
  std::unique_ptr<DistinctTap> tap(new DistinctTap(std::move(input), this));
  tap_ = tap.get();
  inner_.reset(new AggregateRelation(SchemaInfo(), std::move(tap), group, plain, options));
  // output schema: keys, then the aggregates in their order (distinct counts UInt64, Utf8 extrema Utf8, named like the others)
  const SchemaInfo& is = inner_->schema();
  SchemaInfo derived;
  for (int k = 0; k < kw_out_ && k < (int)is.fields.size(); ++k) derived.fields.push_back(is.fields[(size_t)k]);
  for (size_t j = 0; j < aggr.size(); ++j) {
    const int src = out_src_[j];
    if (src >= 0 && src < (int)is.fields.size()) {
      derived.fields.push_back(is.fields[(size_t)src]);
    } else {
      Field f;
      f.name = aggr[j].name;
      f.dtype = out_role_[j] == ROLE_COUNT ? DFX_UINT64 : DFX_UTF8;
      f.nullable = true;
      derived.fields.push_back(f);
    }
  }
  if (caller.fields.size() == derived.fields.size())
    for (size_t i = 0; i < derived.fields.size(); ++i) derived.fields[i].name = caller.fields[i].name;
  schema_ = derived;
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

Status DistinctAggregateRelation::alloc_set(DistinctSet& S, int cap_log2) {
  hipStream_t s = ctx().stream;
  memset(&S.T, 0, sizeof(S.T));
  const uint64_t cap = 1ull << cap_log2;
  DevTable& T = S.T;
  T.stride = cap + 64;
  T.mask = cap - 1;
  T.shift = 64 - cap_log2;
  T.kw = S.kw;
  T.na = 0;
  T.load_limit = cap / 2;
  // Probing runs over the whole set but a row gives up after kSetProbes slots: a set that filled past its load limit while the
  // scan was in flight would otherwise have every row walk all of it before the spill list.  Rehash and replay use max_probe = cap.
  T.max_probe = (int)std::min<uint64_t>(cap, kSetProbes);
  T.block_mask = (uint32_t)(cap - 1);
  Status st;
  auto keys = device_alloc(sizeof(uint64_t) * T.stride * (size_t)S.kw, &st);
  if (!keys) return st;
  auto ctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
  if (!ctrl) return st;
  T.keys = (uint64_t*)keys.get();
  T.accs = nullptr;
  T.ctrl = (uint32_t*)ctrl.get();
  S.owners.clear();
  S.owners.push_back(keys);
  S.owners.push_back(ctrl);
  if (S.kw > 1) {
    auto state = device_alloc(sizeof(uint32_t) * T.stride, &st);
    if (!state) return st;
    T.state = (uint32_t*)state.get();
    S.owners.push_back(state);
    DFX_HIP(hipMemsetAsync(T.state, 0, sizeof(uint32_t) * T.stride, s));
  } else {
    DFX_HIP(launch_fill_u64(T.keys, kEmptyKey, (int64_t)T.stride, s));
  }
  DFX_HIP(hipMemsetAsync(T.ctrl, 0, sizeof(uint32_t) * CTRL_WORDS, s));
  return Status::OK();
}

Status DistinctAggregateRelation::ensure_spill(DistinctSet& S, int64_t rows) {
  if (S.spill.words && S.spill.capacity >= (uint64_t)rows) return Status::OK();
  DFX_HIP(hipStreamSynchronize(ctx().stream));  // (the old list may still be read)
  Status st;
  S.spill_owner = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(rows, 64) * (size_t)S.kw, &st);
  if (!S.spill_owner) return st;
  S.spill.words = (uint64_t*)S.spill_owner.get();
  S.spill.capacity = (uint64_t)std::max<int64_t>(rows, 64);
  return Status::OK();
}

Status DistinctAggregateRelation::read_ctrl(DistinctSet& S, uint32_t* hc) {
  DFX_HIP(hipMemcpyAsync(hc, S.T.ctrl, sizeof(uint32_t) * CTRL_WORDS, hipMemcpyDeviceToHost, ctx().stream));
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  return Status::OK();
}

// Rehash into a set with room for every tuple (occupied + spilled, four times over) and replay the spill list.  The caller has
// synchronised: the control words are exact.
Status DistinctAggregateRelation::grow(DistinctSet& S, uint64_t occupied, uint64_t spilled) {
  hipStream_t s = ctx().stream;
  int lg = 64 - S.T.shift;
  while ((1ull << lg) / 2 < (occupied + spilled) * 2 && lg < 34) ++lg;
  lg = std::max(lg, 64 - S.T.shift + 1);
  DevTable from = S.T;
  std::vector<std::shared_ptr<void>> from_owners = S.owners;
  DFX_RETURN_IF_ERROR(alloc_set(S, lg));
  ++counters().distinct_set_growths;
  ++growths_;
  // Rows neither the rehash nor the replay can place would go to this list.  With probing over the whole table and a load of at
  // most 1/2 none can; it exists for the kernels' contract, and a non-zero cursor is reported.
  Status st;
  auto tmp = device_alloc(sizeof(uint64_t) * 64 * (size_t)S.kw, &st);
  if (!tmp) return st;
  DevRows none;
  none.words = (uint64_t*)tmp.get();
  none.capacity = 64;
  DevTable all = S.T;  // (a set at most a quarter full: every tuple finds a slot when the probe may walk the whole set)
  all.max_probe = (int)std::min<uint64_t>(all.mask + 1, 1u << 30);
  DFX_HIP(launch_rehash(from, all, none, s));
  if (spilled) {
    counters().distinct_spill_rows += (long long)spilled;
    spill_rows_ += (long long)spilled;
    DFX_HIP(launch_merge_rows(S.spill, 0, (int64_t)std::min<uint64_t>(spilled, S.spill.capacity), all, none, s));
  }
  DFX_HIP(hipStreamSynchronize(s));
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(read_ctrl(S, hc));
  if (hc[CTRL_SPILL_LO] || hc[CTRL_SPILL_HI]) return Status::Err(DFX_INTERNAL_ERROR, "COUNT_DISTINCT: a grown set did not take its tuples");
  return Status::OK();
}

// a snapshot of the set's control block after an insert of `rows` rows: errors, spill replay, growth
Status DistinctAggregateRelation::settle(DistinctSet& S, const uint32_t* hc, int64_t rows, bool synced) {
  (void)rows;
  if (hc[CTRL_ERROR]) return error_from_ctrl(hc[CTRL_ERROR]);
  const uint64_t spilled = (uint64_t)hc[CTRL_SPILL_LO] | ((uint64_t)hc[CTRL_SPILL_HI] << 32);
  const uint64_t occupied = hc[CTRL_OCCUPIED] + (uint64_t)0;
  if (spilled == 0 && occupied <= S.T.load_limit) return Status::OK();
  if (spilled > S.spill.capacity) return Status::Err(DFX_INTERNAL_ERROR, "COUNT_DISTINCT: spill list overflow");
  if (!synced) DFX_HIP(hipStreamSynchronize(ctx().stream));
  return grow(S, occupied, spilled);
}

Status DistinctAggregateRelation::consume(const DeviceBatch& b) {
  hipStream_t s = ctx().stream;
  const int64_t n = b.num_rows;
  rows_seen_ += n;
  if (sets_.empty() || n <= 0) return Status::OK();
  DeviceBatch ab;  // the batch + the dictionary id columns
  ab.num_rows = n;
  ab.columns = b.columns;
  ab.columns.resize(bind_schema_.fields.size());
  for (Dict& d : dicts_) DFX_RETURN_IF_ERROR(d.encode(b.columns[(size_t)d.src_col], n, opt().dict_capacity_log2, &ab.columns[(size_t)d.virt_col]));
  for (auto& sp : sets_) {
    DistinctSet& S = *sp;
    if (!S.T.keys) {
      int lg = opt().distinct_capacity_log2 > 0 ? opt().distinct_capacity_log2 : 20;
      DFX_RETURN_IF_ERROR(alloc_set(S, std::max(6, std::min(lg, 34))));
      Status st;
      S.snap = pinned_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
      if (!S.snap) return st;
      DFX_HIP(hipEventCreateWithFlags(&S.snap_ev, hipEventDisableTiming));
    }
    // the previous batch's snapshot (its insert has long finished: the inner aggregate's kernels for it were queued behind)
    if (S.snap_pending) {
      DFX_HIP(hipEventSynchronize(S.snap_ev));
      S.snap_pending = false;
      DFX_RETURN_IF_ERROR(settle(S, (const uint32_t*)S.snap.get(), S.snap_rows, false));
    }
    DFX_RETURN_IF_ERROR(ensure_spill(S, n));
    DevProgram P;
    DevColumns C;
    DFX_RETURN_IF_ERROR(S.builder->bind(ab, &P, &C));
    DevFastPlan F = S.fast;
    F.plan_mode = opt().fast != 0 ? (opt().plan & 3) : 0;
    if (!opt().fast) F.valid = 0;
    DFX_HIP(launch_distinct_insert(P, F, C, S.plan, kw_out_, S.T, S.spill, n, &S.plan_kernel, s));
    DFX_HIP(launch_copy_to_host(S.T.ctrl, S.snap.get(), sizeof(uint32_t) * CTRL_WORDS, s));
    DFX_HIP(hipEventRecord(S.snap_ev, s));
    S.snap_pending = true;
    S.snap_rows = n;
  }
  return Status::OK();
}

// the emitted keys as the sets' programs saw them (Utf8: through this side's dictionary); *ids keeps the id columns alive
Status DistinctAggregateRelation::emitted_keys(const DeviceBatch& inner_out, DevDistinctKeys* K, std::vector<DeviceColumn>* ids) {
  memset(K, 0, sizeof(*K));
  ids->assign(dicts_.size(), DeviceColumn());
  for (int k = 0; k < kw_out_; ++k) {
    const DeviceColumn& kc = inner_out.columns[(size_t)k];
    if (key_dict_[(size_t)k] >= 0) {
      Dict& d = dicts_[(size_t)key_dict_[(size_t)k]];
      DFX_RETURN_IF_ERROR(d.encode(kc, inner_out.num_rows, opt().dict_capacity_log2, &(*ids)[(size_t)key_dict_[(size_t)k]]));
      K->values[k] = (*ids)[(size_t)key_dict_[(size_t)k]].values;
      K->dtype[k] = T_U64;
    } else {
      K->values[k] = kc.values;
      K->dtype[k] = (uint8_t)kc.dtype;
    }
  }
  return Status::OK();
}

// g dictionary ids + validity -> a nullable Arrow Utf8 column on the device, the way the GROUP BY turns the ids of a Utf8 key column
// back into strings (lengths, scan, gather).  A null row carries the id of the empty string: length 0, nothing gathered.
Status utf8_column_from_ids(const DevDict& D, const std::shared_ptr<void>& ids, int64_t g, const std::shared_ptr<void>& validity,
                            int64_t null_count, DeviceColumn* out) {
  hipStream_t s = ctx().stream;
  Status st;
  auto lens = device_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(g, 1), &st);
  if (!lens) return st;
  auto starts = device_alloc(sizeof(uint64_t) * (size_t)(g + 1), &st);
  if (!starts) return st;
  auto tmp = device_alloc(sizeof(uint64_t) * (size_t)(g / 4096 + 4), &st);
  if (!tmp) return st;
  auto offs = device_alloc(sizeof(int32_t) * (size_t)(g + 1), &st);
  if (!offs) return st;
  uint64_t total = 0;
  if (g > 0) {
    DFX_HIP(launch_dict_lengths((const uint64_t*)ids.get(), g, D, (uint32_t*)lens.get(), s));
    DFX_HIP(launch_scan_u32((const uint32_t*)lens.get(), (uint64_t*)starts.get(), g, (uint64_t*)tmp.get(), s));
    DFX_HIP(hipMemcpyAsync(&total, (uint64_t*)starts.get() + g, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
  } else {
    DFX_HIP(hipMemsetAsync(starts.get(), 0, sizeof(uint64_t), s));
  }
  if (total > 0x7FFFFFFFull) return Status::Err(DFX_EXECUTION_ERROR, "Utf8 MIN/MAX results exceed 2 GB (Arrow Utf8 offsets are 32-bit)");
  auto data = device_alloc((size_t)std::max<uint64_t>(total, 8), &st);
  if (!data) return st;
  DFX_HIP(launch_dict_gather((const uint64_t*)ids.get(), g, D, (const uint64_t*)starts.get(), (int32_t*)offs.get(), (uint8_t*)data.get(), s));
  out->dtype = DFX_UTF8;
  out->length = g;
  out->null_count = null_count;
  out->validity = null_count ? (const uint8_t*)validity.get() : nullptr;
  out->bit_offset = 0;
  out->values = nullptr;
  out->offsets = (const int32_t*)offs.get();
  out->data = (const uint8_t*)data.get();
  out->data_bytes = (int64_t)total;
  out->owners.clear();
  out->owners.push_back(offs);
  out->owners.push_back(data);
  if (null_count) out->owners.push_back(validity);
  return Status::OK();
}

// g rows of NULL: what a set that no tuple reached gives every group
Status utf8_null_column(int64_t g, DeviceColumn* out) {
  hipStream_t s = ctx().stream;
  Status st;
  auto offs = device_alloc(sizeof(int32_t) * (size_t)(g + 1), &st);
  if (!offs) return st;
  const size_t vbytes = sizeof(uint64_t) * (size_t)std::max<int64_t>((g + 63) / 64, 1);
  auto validity = device_alloc(vbytes, &st);
  if (!validity) return st;
  auto data = device_alloc(8, &st);
  if (!data) return st;
  DFX_HIP(hipMemsetAsync(offs.get(), 0, sizeof(int32_t) * (size_t)(g + 1), s));
  DFX_HIP(hipMemsetAsync(validity.get(), 0, vbytes, s));
  out->dtype = DFX_UTF8;
  out->length = g;
  out->null_count = g;
  out->validity = g ? (const uint8_t*)validity.get() : nullptr;
  out->bit_offset = 0;
  out->values = nullptr;
  out->offsets = (const int32_t*)offs.get();
  out->data = (const uint8_t*)data.get();
  out->data_bytes = 0;
  out->owners = {offs, data, validity};
  return Status::OK();
}

// MIN / MAX of the set's Utf8 argument per emitted group (ungrouped: of the one row): fold the set into the extrema table, look
// every group up, ids -> strings.  A group without a non-null argument has no entry, or an empty word: NULL.
Status DistinctAggregateRelation::emit_extrema(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* min_col, DeviceColumn* max_col) {
  hipStream_t s = ctx().stream;
  Status st;
  const int64_t g = inner_out.num_rows;
  DeviceColumn* cols[2] = {S.want_min ? min_col : nullptr, S.want_max ? max_col : nullptr};
  if (!S.T.keys || g == 0 || S.arg_dict < 0) {  // no batch reached the set (or there is no group to report)
    for (DeviceColumn* c : cols)
      if (c) DFX_RETURN_IF_ERROR(utf8_null_column(g, c));
    return Status::OK();
  }
  Dict& d = dicts_[(size_t)S.arg_dict];
  // The id a NULL is gathered through: the empty string's, put into the dictionary if no row held it (the sets are not touched).
  // Every encode of this emit comes before the fold: growth replaces the dictionary's arrays (ids stay).
  uint64_t null_id = 0;
  {
    auto zero = device_alloc(16, &st);
    if (!zero) return st;
    DFX_HIP(hipMemsetAsync(zero.get(), 0, 16, s));
    DeviceColumn empty, id_col;
    empty.dtype = DFX_UTF8;
    empty.length = 1;
    empty.offsets = (const int32_t*)zero.get();
    empty.data = (const uint8_t*)zero.get() + 8;
    empty.owners.push_back(zero);
    DFX_RETURN_IF_ERROR(d.encode(empty, 1, opt().dict_capacity_log2, &id_col));
    DFX_HIP(hipMemcpyAsync(&null_id, id_col.values, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    if (null_id >= d.ids_used) return Status::Err(DFX_INTERNAL_ERROR, "MIN/MAX of Utf8: the dictionary did not take the empty string");
  }
  DevDistinctKeys K;
  std::vector<DeviceColumn> key_ids;
  DFX_RETURN_IF_ERROR(emitted_keys(inner_out, &K, &key_ids));
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(read_ctrl(S, hc));
  if (!S.want_count) counters().distinct_inserted += (long long)hc[CTRL_OCCUPIED];  // (emit_counts adds it for a set it reads too)
  EmitTable E;
  DFX_RETURN_IF_ERROR(alloc_emit_table(S.kw, hc[CTRL_OCCUPIED], 2, &E));
  DFX_HIP(launch_utf8_extrema_fold(S.T, E.T, d.D, d.ids_used, (S.want_min ? 1u : 0u) | (S.want_max ? 2u : 0u), s));
  for (int plane = 0; plane < 2; ++plane) {
    if (!cols[plane]) continue;
    auto ids = device_alloc(sizeof(uint64_t) * (size_t)g, &st);
    if (!ids) return st;
    auto validity = device_alloc(sizeof(uint64_t) * (size_t)((g + 63) / 64), &st);
    if (!validity) return st;
    auto nulls = device_alloc(sizeof(uint64_t), &st);
    if (!nulls) return st;
    DFX_HIP(hipMemsetAsync(nulls.get(), 0, sizeof(uint64_t), s));
    DFX_HIP(launch_utf8_extrema_lookup(E.T, K, kw_out_, g, plane, null_id, (uint64_t*)ids.get(), (uint64_t*)validity.get(), (uint64_t*)nulls.get(), s));
    uint64_t null_count = 0;
    uint32_t cc[CTRL_WORDS];
    DFX_HIP(hipMemcpyAsync(&null_count, nulls.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipMemcpyAsync(cc, E.T.ctrl, sizeof(cc), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    if (cc[CTRL_ERROR] & 0x200u) return Status::Err(DFX_INTERNAL_ERROR, "MIN/MAX of Utf8: a tuple's argument is no id of the dictionary");
    if (cc[CTRL_ERROR]) return Status::Err(DFX_INTERNAL_ERROR, "MIN/MAX of Utf8: extrema table overflow");
    DFX_RETURN_IF_ERROR(utf8_column_from_ids(d.D, ids, g, validity, (int64_t)null_count, cols[plane]));
  }
  return Status::OK();
}

// the set's count per emitted group (grouped) or its tuple count (ungrouped)
Status DistinctAggregateRelation::emit_counts(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* col, uint64_t* ungrouped_total) {
  hipStream_t s = ctx().stream;
  Status st;
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(read_ctrl(S, hc));
  const uint64_t occupied = hc[CTRL_OCCUPIED];
  counters().distinct_inserted += (long long)occupied;
  auto total = device_alloc(sizeof(uint64_t), &st);
  if (!total) return st;
  DFX_HIP(hipMemsetAsync(total.get(), 0, sizeof(uint64_t), s));
  if (kw_out_ == 0) {
    DevTable none;
    memset(&none, 0, sizeof(none));
    DFX_HIP(launch_distinct_count(S.T, none, (uint64_t*)total.get(), s));
    DFX_HIP(hipMemcpyAsync(ungrouped_total, total.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    return Status::OK();
  }
  // count table: the key prefix + one ACC_ADD_U64 plane
  EmitTable E;
  DFX_RETURN_IF_ERROR(alloc_emit_table(S.kw, occupied, 1, &E));
  const DevTable& Cn = E.T;
  DFX_HIP(launch_distinct_count(S.T, Cn, (uint64_t*)total.get(), s));
  const int64_t g = inner_out.num_rows;
  DevDistinctKeys K;
  std::vector<DeviceColumn> ids;
  DFX_RETURN_IF_ERROR(emitted_keys(inner_out, &K, &ids));
  auto vals = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(g, 1), &st);
  if (!vals) return st;
  DFX_HIP(launch_distinct_lookup(Cn, K, kw_out_, g, (uint64_t*)vals.get(), s));
  DFX_HIP(hipStreamSynchronize(s));
  uint32_t cc[CTRL_WORDS];
  DFX_HIP(hipMemcpyAsync(cc, Cn.ctrl, sizeof(cc), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  if (cc[CTRL_ERROR]) return Status::Err(DFX_INTERNAL_ERROR, "COUNT_DISTINCT: count table overflow");
  col->dtype = DFX_UINT64;
  col->length = g;
  col->null_count = 0;
  col->values = vals.get();
  col->validity = nullptr;
  col->owners.push_back(vals);
  return Status::OK();
}

Status DistinctAggregateRelation::next(DeviceBatch* out, bool* has) {
  *has = false;
  if (done_) return Status::OK();
  done_ = true;
  DeviceBatch in;
  bool in_has = false;
  DFX_RETURN_IF_ERROR(inner_->next(&in, &in_has));  // drains the input through the tap
  if (!in_has) return Status::OK();
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  for (auto& sp : sets_) {  // the last batch's spill and growth
    DistinctSet& S = *sp;
    if (!S.T.keys) continue;
    S.snap_pending = false;
    uint32_t hc[CTRL_WORDS];
    DFX_RETURN_IF_ERROR(read_ctrl(S, hc));
    DFX_RETURN_IF_ERROR(settle(S, hc, S.snap_rows, true));
  }
  out->num_rows = in.num_rows;
  out->columns.clear();
  for (int k = 0; k < kw_out_; ++k) out->columns.push_back(in.columns[(size_t)k]);
  std::vector<DeviceColumn> set_cols(sets_.size()), min_cols(sets_.size()), max_cols(sets_.size());
  std::vector<uint64_t> set_total(sets_.size(), 0);
  for (size_t si = 0; si < sets_.size(); ++si) {
    DistinctSet& S = *sets_[si];
    if (S.want_min || S.want_max) DFX_RETURN_IF_ERROR(emit_extrema(S, in, &min_cols[si], &max_cols[si]));
    if (!S.want_count) continue;
    if (!S.T.keys) {  // no batch reached the set: every group counts 0
      if (kw_out_ > 0) {
        Status st;
        auto vals = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(in.num_rows, 1), &st);
        if (!vals) return st;
        DFX_HIP(hipMemsetAsync(vals.get(), 0, sizeof(uint64_t) * (size_t)std::max<int64_t>(in.num_rows, 1), ctx().stream));
        set_cols[si].dtype = DFX_UINT64;
        set_cols[si].length = in.num_rows;
        set_cols[si].values = vals.get();
        set_cols[si].owners.push_back(vals);
      }
      continue;
    }
    DFX_RETURN_IF_ERROR(emit_counts(S, in, &set_cols[si], &set_total[si]));
  }
  if (kw_out_ == 0) {  // one row: the set's count, valid exactly where COUNT(x) of the same rows is
    for (size_t si = 0; si < sets_.size(); ++si) {
      if (!sets_[si]->want_count) continue;
      const bool valid = hidden_count_[si] < 0 || in.columns[(size_t)hidden_count_[si]].null_count == 0;
      const uint64_t v = valid ? set_total[si] : 0;
      DeviceColumn& c = set_cols[si];
      c.dtype = DFX_UINT64;
      c.length = 1;
      std::shared_ptr<void> dv;
      DFX_RETURN_IF_ERROR(upload_bytes(&v, 8, &dv));
      c.values = dv.get();
      c.owners.push_back(dv);
      if (!valid) {
        const uint8_t vb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::shared_ptr<void> dn;
        DFX_RETURN_IF_ERROR(upload_bytes(vb, 8, &dn));
        c.validity = (const uint8_t*)dn.get();
        c.null_count = 1;
        c.owners.push_back(dn);
      }
    }
  }
  for (size_t j = 0; j < out_src_.size(); ++j) {
    const int src = out_src_[j];
    if (src >= 0) out->columns.push_back(in.columns[(size_t)src]);
    else out->columns.push_back((out_role_[j] == ROLE_MIN ? min_cols : out_role_[j] == ROLE_MAX ? max_cols : set_cols)[(size_t)(-1 - src)]);
  }
  *has = true;
  return Status::OK();
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

}  // namespace

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
