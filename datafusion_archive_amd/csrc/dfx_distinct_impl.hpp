// dfx_distinct_impl.hpp -- what the translation units of the distinct-set aggregates share (dfx_distinct*.cpp include it, nothing
// else does; dfx_relation.hpp declares the three entry points).
//   dfx_distinct.cpp       the design, planning (init and its steps), explain, the exchange refusal, the entry points
//   dfx_distinct_sets.cpp  per batch: the sets' tables, spill lists, growth, the insert (consume)
//   dfx_distinct_emit.cpp  at emit: count and extrema tables, the result columns, next
#pragma once
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "dfx_relation.hpp"
#include "dfx_utf8_dict.hpp"

namespace dfx {

// a Utf8 column's device dictionary (one per column, shared by the keys and arguments that read it): strings -> stable UInt64 ids
struct DistinctDict {
  int src_col = 0;   // the Utf8 column of the input schema
  int virt_col = 0;  // its id column in the bind schema
  Utf8Dict dict{"Utf8 dictionary"};
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

// An emit-time table keyed by the key prefix of a set's tuples (the set's width, the argument word zeroed): the count table, the
// extrema table.  At most half full -- a set of `occupied` tuples has at most as many prefixes -- with probing over the whole
// table, and `planes` zeroed accumulator planes.  Ungrouped (kw == 1) the prefix has no words: one entry, stride 1, no keys.
struct EmitTable {
  DevTable T;
  std::vector<std::shared_ptr<void>> owners;
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
  ScanMemo* column_memo() override { return input_->column_memo(); }
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
  SchemaInfo bind_schema_;  // the input schema + the dictionaries' id columns (UInt64: every Utf8 field of it is an input column)
  std::unique_ptr<AggregateRelation> inner_;
  DistinctTap* tap_ = nullptr;  // owned by inner_
  int kw_out_ = 0;
  std::vector<dfx_runtime_expr> group_;
  std::vector<int> key_dict_;  // per GROUP BY key: index into dicts_ (-1: not Utf8)
  std::vector<DistinctDict> dicts_;
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
  // ---- planning (dfx_distinct.cpp): init and its steps ----
  struct Planning {  // what the steps of init hand on
    std::vector<dfx_runtime_expr> group_rw;  // the GROUP BY expressions, Utf8 columns redirected to their id columns
    std::vector<dfx_runtime_expr> orig;      // the aggregates as written
    std::vector<dfx_runtime_expr> aggr;      // ... the first of every set with a Utf8 argument redirected to its id column
    std::vector<int> set_of;                 // per aggregate: its set (-1: plain)
    std::vector<dfx_runtime_expr> plain;     // the inner aggregate's list
  };
  int dict_of(int col);
  int utf8_column(const dfx_runtime_expr& e, int32_t idx) const;
  Status utf8_argument(const dfx_runtime_expr& e, const char* what, int* col) const;
  void rewrite_utf8_keys(Planning* p);
  Status assign_aggregates_to_sets(Planning* p);
  Status build_set_programs(const Planning& p);
  void add_hidden_counts(Planning* p);
  void derive_schema(const Planning& p, const SchemaInfo& caller);
  // ---- per batch (dfx_distinct_sets.cpp) ----
  Status alloc_set(DistinctSet& S, int cap_log2);
  Status ensure_spill(DistinctSet& S, int64_t rows);
  Status read_ctrl(DistinctSet& S, uint32_t* hc);
  Status grow(DistinctSet& S, uint64_t occupied, uint64_t spilled);
  Status settle(DistinctSet& S, const uint32_t* hc, bool synced);
  // (consume and emitted_keys: the two places whose ids a set's program binds)
  Status encode_with_validity(DistinctDict& d, const DeviceColumn& src, int64_t n, DeviceColumn* ids_col);
  // ---- emit (dfx_distinct_emit.cpp) ----
  Status emitted_keys(const DeviceBatch& inner_out, DevDistinctKeys* K, std::vector<DeviceColumn>* ids);
  Status emit_counts(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* col, uint64_t* ungrouped_total);
  Status emit_extrema(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* min_col, DeviceColumn* max_col);
};

}  // namespace dfx
