// dfx_aggregate_impl.hpp -- AggregateRelation::Impl: the state the translation units of the aggregate operator share
// (dfx_aggregate*.cpp include it, nothing else does; dfx_relation.hpp only forward-declares Impl).
//   dfx_aggregate.cpp           set-up, chunks of accumulators, explain, next, drain
//   dfx_aggregate_strategy.cpp  one batch through the strategy state machine (Phase, StrategyDecision)
//   dfx_aggregate_table.cpp     the table and its spill list: allocation, growth and replay
//   dfx_aggregate_ctrl.cpp      control-block checks one batch behind the launches (CtrlPipeline)
//   dfx_aggregate_shadow.cpp    the column shadows a launch binds, the routed shadow (ShadowBindings)
//   dfx_aggregate_launch.cpp    routing regions (Pass2Window), the launches of one slice of rows
//   dfx_aggregate_emit.cpp      the key column ahead of time (EarlyKeys), the result batch
//   dfx_aggregate_partial.cpp   multi-GPU export / import
// The Utf8 key dictionaries are Utf8Dict (dfx_utf8_dict.hpp), shared with the distinct-set aggregates.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "dfx_agg_rules.hpp"
#include "dfx_pass1_layout.hpp"
#include "dfx_relation.hpp"
#include "dfx_sigs.hpp"
#include "dfx_utf8_dict.hpp"

namespace dfx {

inline uint64_t ctrl_spilled(const uint32_t* hc) { return ((uint64_t)hc[CTRL_SPILL_HI] << 32) | hc[CTRL_SPILL_LO]; }  // the spill cursor of a control block on the host

inline DevRows no_spill_rows() {  // for kernels that must not spill (rehash, merges into a table sized for its rows)
  DevRows r;
  r.words = nullptr;
  r.capacity = 0;
  return r;
}

inline void mark_columns(std::vector<char>* needed, const std::vector<int>& cols) {
  for (int ci : cols)
    if (ci >= 0 && ci < (int)needed->size()) (*needed)[(size_t)ci] = 1;
}

// The strategy follows the number of groups: up to kLdsGroupsMax the LDS front cache pays (every later row is an LDS atomic); from
// kPartitionGroupsMin on (one key word) per-row global atomics would cap the query near 24 G rows/s, so rows are routed to their
// table blocks instead (dfx_k_partition.hip); in between, the global table alone.
constexpr uint64_t kLdsGroupsMax = 8192, kPartitionGroupsMin = 16384;

// What the calibration slice (or the resident table's memo, or a forced strategy) decided for the rest of the stream.
struct StrategyDecision {
  bool calibrated = false;     // the decision has been taken
  bool lds_enabled = true;
  bool use_partition = false;  // strategy 3: route rows to table blocks, aggregate blocks in LDS
  bool narrow = false;         // every key the calibration slice saw is below 2^32: 12-byte routed rows (PTF_NARROW)
  bool dense_seen = false;     // more than half of the calibration slice's rows passed the predicate: pass 2 after every batch
  bool mostly_seen = false;    // ... more than two thirds: pass 1's wave-specialised kernel runs 4 scanner + 12 router waves instead of 8 + 8
  bool skew_seen = false;      // the calibration slice's front cache absorbed a sizeable share of its rows: heavy keys
  uint64_t occupied_known = 0;
  // the memo word (ScanMemo): the group count below four flag bits
  uint64_t pack() const {
    return occupied_known | (skew_seen ? 1ull << 63 : 0ull) | (narrow ? 1ull << 62 : 0ull) | (dense_seen ? 1ull << 61 : 0ull) | (mostly_seen ? 1ull << 60 : 0ull);
  }
  void unpack(uint64_t w) {
    skew_seen = (w >> 63) != 0;
    narrow = ((w >> 62) & 1) != 0;
    dense_seen = ((w >> 61) & 1) != 0;
    mostly_seen = ((w >> 60) & 1) != 0;
    occupied_known = w & ~(15ull << 60);
  }
  void apply_group_count(int kw) {  // (the caller sizes the spill list when this turns use_partition on)
    calibrated = true;
    lds_enabled = occupied_known <= kLdsGroupsMax;
    if (!lds_enabled && kw == 1 && occupied_known >= kPartitionGroupsMin) use_partition = true;
  }
};

// Pass 2 is DEFERRED: pass 1 of several batches appends to the same routing regions (their fill counters live in
// PT.counts between launches) and one pass 2 aggregates them all -- its table-block load/store, its launch and its
// short-region tails are paid once per window instead of once per batch.  The window closes when the regions could
// overflow: fill_bound is an upper bound of the largest region fill, from the control-block snapshots
// (CTRL_MAX_FILL, one batch behind) plus `worst` rows for every batch launched since.
struct Pass2Window {
  std::shared_ptr<void> rows, counts;  // the routing regions and their fill counters (DevPartition::rows / counts)
  size_t rows_bytes = 0, cnt_bytes = 0;
  bool layout_valid = false;
  int64_t layout_rows = 0;     // batch length the region layout was sized for
  uint32_t worst = 0;          // rows one batch of that length adds to a region in the expected worst case (2 x average + 64)
  int pending = 0;             // pass-1 launches waiting for their pass 2
  uint64_t fill_bound = 0;
  int64_t last_p2_seq = -1;    // batch_seq at the last pass-2 launch: older snapshots say nothing about the current fills
  int64_t rows_in_flight = 0;  // input rows of the pending launches (all of them may still end up in the spill list)
  std::shared_ptr<void> snap_done;  // device word of DevPartition::snap_done
  bool snap_armed = false;          // the batch just launched writes its own control-block snapshot (no copy on the side stream)
  void closed() { pending = 0, fill_bound = 0, rows_in_flight = 0; }  // nothing is waiting for a pass 2
};

// Control block checks run ONE BATCH BEHIND the launches: after batch i its control block is copied to pinned memory
// asynchronously, batch i + 1 is launched, and only then is batch i's copy examined, so the device never idles on a host
// round trip between batches.
struct CtrlPipeline {
  std::shared_ptr<void> host;                  // pinned, 2 x CTRL_WORDS
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipEvent_t main_ev[2] = {nullptr, nullptr};  // "batch i launched" markers on the main stream
  bool pending[2] = {false, false};
  int64_t rows[2] = {0, 0};
  int64_t seq[2] = {0, 0};                     // batch_seq of the launch each snapshot follows
  int64_t batch_seq = 0;
  uint64_t unconfirmed_rows = 0;               // rows of launched batches whose control block is not examined yet
  void forget() { pending[0] = pending[1] = false, unconfirmed_rows = 0; }  // a synchronous read of the block supersedes the snapshots
};

// What one query knows of the resident table's shadows (ScanMemo: dfx_key_shadow.hpp, dfx_value_shadow.hpp, dfx_routed_shadow.hpp).
struct ShadowBindings {
  bool key_shadow_asked = false, value_shadow_asked = false;  // the query's first question of each column shadow may build it
  bool shadow_built_here = false;      // a query that builds a shadow itself keeps its 12-byte rows to the end (both_shadows_bind)
  int64_t key_shadow_launches = 0, value_shadow_launches = 0, row8_launches = 0, routed_shadow_launches = 0;  // (explain)
  // the (key, operand) pair whose operand shadow a pass-1 launch of this query bound: what routed_shadow_maybe builds the routed shadow of
  const void *routed_keys = nullptr, *routed_values = nullptr;
  int64_t routed_rows = 0;
  uint32_t ws_scanners_of_build = 4;   // the build's split of scanner and router waves (the dense layout's)
};

struct AggregateRelation::Impl {
  std::unique_ptr<Relation> input;
  bool has_pred = false;
  dfx_runtime_expr pred;
  std::vector<dfx_runtime_expr> group, aggr;
  // Utf8 GROUP BY keys are dictionary-encoded on the device into UInt64 ids that live in extra ("virtual")
  // columns appended to every input batch; the fused program sees an ordinary integer key (dfx_k_dict.hip)
  struct DictKey {
    int key = 0;       // index among the GROUP BY expressions
    int src_col = 0;   // the Utf8 column of the input schema
    int virt_col = 0;  // its UInt64 id column in `bind_schema`
    Utf8Dict dict{"Utf8 key dictionary"};
  };
  std::vector<DictKey> dicts;
  SchemaInfo bind_schema;                  // input schema + the virtual id columns + the string terms' Boolean columns (what the program binds to)
  // Utf8 string terms of the absorbed predicate (deviation D9): their bitmaps are computed per batch beside the dictionary ids
  // and bound as virtual Boolean columns; `pred` stays as written (the real FilterRelation of a null batch compiles its own)
  Utf8Terms pred_terms;
  // Several chunks of accumulators scan the same batches one after the other: the terms are evaluated ONCE per batch and the bitmaps
  // reused by every chunk.  Entries live only inside the chunk loops of consume_batch / run_held, while the batches they were
  // computed from are held (so a batch is safely named by its offsets pointer and row count).
  struct TermCacheEntry {
    const void* offsets = nullptr;
    int64_t rows = 0;
    std::vector<DeviceColumn> cols;  // the virtual Boolean columns, in pred_terms.terms() order
  };
  std::vector<TermCacheEntry> term_cache;
  bool term_cache_on = false;
  struct TermCacheScope {  // the cache is on for the lifetime of this object (also left on an error return)
    Impl& m;
    explicit TermCacheScope(Impl& i) : m(i) { m.term_cache_on = true; }
    ~TermCacheScope() {
      m.term_cache_on = false;
      m.term_cache.clear();
    }
  };
  std::vector<dfx_runtime_expr> group_rw;  // GROUP BY expressions with Utf8 columns redirected to their id columns
  std::vector<int> key_out_dtype;          // result type of each key column (DFX_UTF8 for dictionary keys)
  // result aggregates -> accumulators: AVG(x) is the pair SUM(x), COUNT(x) of consecutive accumulators, divided at
  // emit time (deviation D7).  `aggr` holds the ACCUMULATOR expressions (AVG already expanded), `outs` the results.
  struct OutAgg {
    int acc = 0;
    bool avg = false;
    int dtype = 0;
    std::string name;
  };
  std::vector<OutAgg> outs;
  // More accumulators than one fused program takes (the reference has no limit: create_accumulators builds any number,
  // aggregate.rs:319-342; real TPC-H Q1 needs 11) are split into CHUNKS -- <= kMaxAggs accumulators whose arguments fit the
  // program's limits on columns / computed values / literals: one fused program per chunk
  // (predicate + keys + that chunk's arguments), all chunks updating their own accumulator planes of the SAME table --
  // the second chunk's kernels find the key the first one inserted.  The programs stay in their chunk; cur() is the ACTIVE one,
  // active() its programs in use, and the table view T always describes it.
  static constexpr int kMaxAccsTotal = 32;
  struct Programs {
    std::unique_ptr<ProgramBuilder> builder;
    DevAggPlan plan;
    DevFastPlan fast;
  };
  struct Chunk {
    int a0 = 0, n = 0;  // accumulators [a0, a0 + n)
    Programs fused;     // predicate + keys + arguments
    // The same program WITHOUT the absorbed predicate, for batches whose referenced columns carry nulls: the reference's
    // FilterRelation emits all-valid arrays (fn filter ignores value nulls, filter.rs:83-92), so an aggregate over a Filter
    // sees every surviving slot as valid -- COUNT counts them, SUM adds whatever the slot holds.  A fused evaluation would
    // apply the ORIGINAL validity to the aggregate arguments; such batches are therefore filtered for real
    // (FilterRelation's kernels) and then aggregated without a predicate.  Null-free batches stay fused.
    Programs np;
    std::shared_ptr<void> partial, state, dev_arg_dtype, dev_func;  // ungrouped state of this chunk
  };
  std::vector<Chunk> chunks;
  int cur_chunk = 0;
  bool unfused_now = false;  // the batch in hand went through a real FilterRelation: the predicate-free programs are in use
  Chunk& cur() { return chunks[(size_t)cur_chunk]; }
  const Chunk& cur() const { return chunks[(size_t)cur_chunk]; }
  Programs& active() { return unfused_now ? cur().np : cur().fused; }
  const Programs& active() const { return unfused_now ? cur().np : cur().fused; }
  // the active chunk's accumulators: a window into the per-accumulator arrays
  int na() const { return cur().n; }
  const uint8_t* acc_kind() const { return acc_kind_all + cur().a0; }
  const uint8_t* val_xform() const { return val_xform_all + cur().a0; }
  const uint64_t* acc_init() const { return acc_init_all + cur().a0; }
  // ONE key, several aggregates of DIFFERENT operands (SUM(v), MIN(w) ...): under the partitioned strategy a scan per aggregate --
  // each through the one-value kernels (12-byte routed rows, 256 partitions, the wave-specialised pass 1, the lean pass 2) -- beats
  // one scan that routes a row per key with every operand (24-byte rows: 512 partitions, 4-row chunks: pass 1 alone 1.42 ms per 2^27
  // rows against 2 x 0.43).  `single_chunks` holds that chunking, built at set-up; it replaces `chunks` when the strategy decision
  // (calibration slice or the resident table's memo) says "partitioned" -- few groups keep the one scan for all aggregates.
  std::vector<Chunk> single_chunks;  // (non-empty: built and not installed)
  // Round 6, late: the PAIR scan.  Two aggregates, narrow keys, a program the scan plan binds with three columns: the all-aggregates
  // program keeps running -- ONE scan routes {operand 0, image, operand 1} (20-byte rows, six per 128-byte line: PTF_PAIR) and pass 2
  // runs once per accumulator plane over the same regions, each launch the one-value kernel with its 96 KB block.  16 + 24 bytes read
  // per row become 24.  `single_chunks` stays in reserve: the stream falls back to it at a batch boundary when the pair kernels no
  // longer apply (the table outgrew 256 partitions, a batch the plan cannot bind).
  // The same host logic serves 2..3 aggregates of ONE operand (split_is_shared; PTF_PLANES, agg.shared_planes): the raw operand goes
  // through the one-value pass 1 exactly as the headline's does, pass 2 runs once per accumulator plane with that aggregate's
  // transform.  Rounds 3-6 gave such queries 4096-slot blocks holding every plane (twice the partitions, 8-row chunks of 96 bytes).
  //
  // Where the stream stands between the all-aggregates program and the scans per aggregate.  The legal states, all of them:
  //   NotApplicable  no per-aggregate chunking was built (setup), or the options switch it off (drain, once they are frozen)
  //   Undecided      built; no strategy decision yet (an empty first batch stays here)
  //   OneScan        decided, not partitioned: the all-aggregates program for the rest of the stream
  //   PairScan       decided, partitioned, pair rows (or planes: split_is_shared); single_chunks in reserve
  //   PerAggregate   single_chunks installed
  // Transitions, nothing else:
  //   NotApplicable -> Undecided                      setup, when single_chunks is built
  //   Undecided -> NotApplicable                      drain, before the first batch: agg.split_aggregates / agg.shared_planes say no
  //   Undecided -> OneScan | PairScan | PerAggregate  consume_batch, after the strategy decision
  //   PairScan -> PerAggregate                        pair_fall_back, at a batch boundary
  enum class Phase { NotApplicable, Undecided, OneScan, PairScan, PerAggregate };
  Phase phase = Phase::NotApplicable;
  bool pair_wide_seen = false;   // PairScan only: a key without a 32-bit image turned up; its rows take the spill list until the next batch
                                 // boundary, where the stream leaves for the scans per aggregate (they have a wide routed form)
  bool pair_scan() const { return phase == Phase::PairScan; }
  bool pair_planes() const { return pair_scan() && split_is_shared; }  // the shared-operand flavour
  // (while the per-aggregate chunking is pending -- the table's blocks are sized for one accumulator per scan -- the all-aggregates
  // program never takes the partitioned strategy: its pass 2 would not fit a block into LDS)
  bool partition_allowed() const { return phase != Phase::Undecided && phase != Phase::OneScan; }
  bool split_is_shared = false;  // the aggregates single_chunks splits all take the same operand
  // ... or exactly TWO different operands between them (SUM(v), COUNT(v), MAX(w) ...): split_ops bit a = the operand (0 / 1) of
  // accumulator a, split_arg1 = the first accumulator of operand 1.  Two aggregates: the pair scan as described; three and more: the
  // operands travel RAW in the pair row (null-free batches only) and every accumulator gets its own pass 2 with its transform
  int split_distinct = 0;        // distinct operands among the aggregates (3: more than two)
  uint32_t split_ops = 0, split_arg1 = 0;
  // (four and more aggregates of one operand never had the all-planes block -- shared_operand() stops at three --: they keep the scans per
  // aggregate when the planes are switched off)
  bool split_allowed() const { return opt().split_aggregates && (!split_is_shared || opt().shared_planes || na_total > 3); }
  bool same_operand_all() const {  // shared_operand() without its limit of three
    if (kw != 1 || na() < 2 || !opt().shared_operand) return false;
    for (int a = 1; a < na(); ++a)
      if (active().plan.arg[a] != active().plan.arg[0]) return false;
    return true;
  }
  Pass1LayoutOptions layout_options() const {  // what choose_routed_layout (dfx_pass1_layout.hpp) reads of the options
    const AggOptions& o = opt();
    return {o.narrow_keys, o.narrow_chunk16, o.hot_keys, o.pass2_stream, o.pass1_ws, o.pass1_ws_dense, o.pass1_ws_dense_scanners,
            o.partition_mode, o.partition_layout, o.partition_block, o.partition_producers, o.partition_defer, o.partition_cap_rows, o.partition_pad};
  }
  bool pair_batch_ok(const DeviceBatch& b);
  Status pair_fall_back();
  void install_chunks(std::vector<Chunk>&& next);
  int na_total = 0;
  uint8_t acc_kind_all[kMaxAccsTotal], val_xform_all[kMaxAccsTotal];
  uint64_t acc_init_all[kMaxAccsTotal];
  uint64_t* accs_full = nullptr;  // plane 0 of the table's accumulators (T.accs is the active chunk's first plane)
  DevTable import_T;              // multi-GPU exchange: the table the received group partials are merged into
  uint64_t* import_accs_full = nullptr;
  std::vector<std::shared_ptr<void>> import_owners, import_keep;
  void activate(int c);
  void set_algebra(DevTable* t) const;
  DevTable view_of(const DevTable& any_view, uint64_t* full_accs, int c) const;
  DevTable full_view(const DevTable& any_view, uint64_t* full_accs) const;
  Status partial_view_check() const;
  Status build_chunk_programs(Chunk& ch);
  bool plan_required = false;  // the batch in hand has nulls under the fused predicate and was left fused for a scan plan
  DevFastPlan fast_plan(bool required_bit = true) const {  // the active fast plan as the launchers take it
    DevFastPlan fp = active().fast;
    if (!opt().fast) fp.valid = 0;
    fp.plan_mode = opt().plan | (required_bit && plan_required ? 4 : 0);
    return fp;
  }
  Status deferred;
  bool done = false;
  bool built = false;
  int kw = 0;
  int kw_out = 0;  // GROUP BY expressions of the query = key columns of the result (kw: key WORDS the kernels see -- five to
                   // seven keys are padded to eight with constant zero words, the table kernels being built for 1, 2, 3, 4, 8)
  std::vector<int> key_dtype, arg_dtype, out_dtype, func;
  // grouped state
  DevTable T;
  std::vector<std::shared_ptr<void>> table_owners;
  std::shared_ptr<void> ctrl;
  std::shared_ptr<void> stats;  // DevTable::stats
  DevRows spill;
  std::shared_ptr<void> spill_owner;
  StrategyDecision dec;
  bool calibrating = false;      // the launch in progress is the calibration slice
  int64_t launch_rows_hint = 0;  // > 0: the current batch is routed in launches of at most this many rows
  void force_partition_maybe();
  Status apply_group_count(int64_t n);
  DevPartition PT;
  Pass2Window win;
  int64_t rows_seen = 0;
  // Several chunks of accumulators over ONE table (more than 8 aggregates, or one scan per aggregate): every chunk's scan of a batch
  // ends with a host check of the control block -- rows spilled under chunk c must be replayed while chunk c is active -- i.e. with
  // an idle device for a host round trip.  Round 6: up to chunk_hold batches are HELD and each chunk scans all of them in a row
  // (between batches of one chunk the checks run one batch behind, as in a single-chunk stream): one round trip per chunk and
  // hold, not per chunk and batch (two aggregates of different operands over 10^9 rows: 16 -> 4).
  std::vector<DeviceBatch> held;
  size_t held_bytes = 0;
  Status run_held();
  CtrlPipeline ctl;
  // export
  std::vector<uint64_t> export_counts;
  mutable OperatorOptions options;  // this operator's option set (process defaults + its own overrides, frozen at first use)
  const AggOptions& opt() const { return options.get(); }

  Status setup(const SchemaInfo& input_schema);
  uint64_t program_fingerprint() const;
  Status consume_batch(const DeviceBatch& b);
  // decided != nullptr: return as soon as the strategy is decided; *decided = the rows of b that are done by then
  Status consume_batch_chunk(const DeviceBatch& b, int64_t* decided = nullptr);
  int widest_chunk() const {  // accumulators of the widest chunk: what a slot of the table, a row of the spill list holds at most
    int widest = 0;
    for (const Chunk& ch : chunks) widest = std::max(widest, ch.n);
    return widest;
  }
  // ---- dfx_aggregate_table.cpp
  Status alloc_table(int cap_log2, DevTable* T, std::vector<std::shared_ptr<void>>* owners, bool new_ctrl, uint64_t** full_accs_out);
  Status ensure_spill(int64_t rows);
  Status grow_and_replay(uint64_t occupied, uint64_t spilled, uint64_t replay_from = 0);
  void replace_table(const DevTable& Tn, uint64_t* accs_full_new, const std::vector<std::shared_ptr<void>>& owners, bool forget_snapshot);
  // ---- dfx_aggregate_ctrl.cpp
  Status read_ctrl(uint32_t* host_ctrl);
  Status alloc_ctrl_host();
  Status post_ctrl(int64_t rows);
  Status arm_snapshot(uint32_t** snap_to);
  Status handle_ctrl(const uint32_t* hc, int64_t n);
  Status examine_ctrl(int slot);
  Status settle_ctrl();
  Status finish_launched(int64_t rows, bool read_back = true);
  // ---- dfx_aggregate_shadow.cpp
  ShadowBindings shadows;
  size_t shadow_query_bytes() const;  // the memory rule's "what this query holds"
  // The key column's Int32 shadow (agg.key_shadow; dfx_key_shadow.hpp): the 4-byte words of the key rows this bound batch starts at,
  // or null -- no resident table below, another shape, wide keys, nulls, the option, memory.  The query's first question may build it.
  const uint32_t* key_shadow_words(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt);
  // ... and the operand column's Float32 shadow (agg.value_shadow; dfx_value_shadow.hpp), only beside a bound key shadow: prog, pt are
  // the launch's with the key already bound.  *operand_col: the slot it belongs in
  const uint32_t* value_shadow_words(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt, int* operand_col);
  // The routed row form (agg.routed_row8): would a launch of this bound batch bind BOTH shadows -- each eligible and already built?
  // Asked before ensure_partition, without side effects: nothing is counted, nothing is built.
  int key_shadow_column(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt) const;    // -1: not this launch
  int value_shadow_column(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt) const;  // -1: not this launch
  bool both_shadows_bind(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, int64_t rows, int64_t row0);
  // The routed shadow (agg.routed_shadow; dfx_routed_shadow.hpp): pass 1's unfiltered output per window of the table, kept by the table.
  // routed_pair: the resident (key, operand) columns this bound two-column batch reads, and the table row its first row is.
  // routed_shadow_launch: a launch over exactly one window of a built shadow, of the shape that routes 8-byte rows today, is ONE
  // kernel (Pass2Rows::narrow8_pred) -- *took says whether it was.  routed_shadow_maybe (drain, after the last batch): the build,
  // by a query that bound the operand's shadow.  routed_split_rows: W if this batch's pair has a shadow (launches of whole windows).
  bool routed_pair(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const void** keys, const void** values, int64_t* rows, int64_t* row) const;
  Status routed_shadow_launch(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, int64_t row0, int64_t n, bool* took);
  Status routed_shadow_maybe();
  int64_t routed_split_rows(const DevProgram& prog, const DevColumns& cols) const;
  // ---- dfx_aggregate_launch.cpp
  bool shared_operand() const;
  RoutedLayoutQuery layout_query(int64_t rows, bool nulls_now, bool both_shadows) const;
  // both_shadows: every launch these regions are sized for binds both column shadows (launch_rows: both_shadows_bind)
  Status ensure_partition(int64_t rows, bool nulls_now = false, bool both_shadows = false);
  Status flush_pass2(uint32_t* snap_to = nullptr);  // snap_to: this pass 2 publishes the control block there (arm_snapshot)
  Status launch_rows(const DeviceBatch& b, const DevProgram& prog, const DevColumns& cols, int64_t row0, int64_t n);
  // launch_rows' steps (described where they are defined)
  Status bind_shadows(const DevProgram& prog_in, const DevColumns& cols_in, const DevFastPlan& fp, int64_t row0, int64_t n, int64_t layout_rows,
                      DevProgram* prog, DevColumns* cols, DevPartition* pt, double* bytes);
  bool window_closes() const { return window_must_close(calibrating, win.pending, opt().partition_defer_batches, pair_scan(), win.fill_bound, win.worst, PT.cap_rows); }
  Status launch_routed(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevAggPlan& p, DevPartition pt, int64_t n, double bytes);
  Status launch_table(const DevProgram& prog, const DevColumns& cols, DevAggPlan p, int64_t n, double bytes);
  Status drain();
  Status emit_grouped(DeviceBatch* out, int64_t expected);
  std::shared_ptr<void> emit_total;  // pinned: the scan's group count
  // The key column ahead of time (agg.early_keys).  The result download is the one part of a query that cannot start before its
  // last kernel -- except for the keys: once every group exists, the key column is final.  When the group count has not changed
  // between two consecutive control-block snapshots, the compaction of the key plane and its copy to pinned memory are queued on
  // the side stream while the scan goes on.  At emit the copy is valid iff no group was added since (groups are never removed: the
  // count then differs) and the table was not replaced; it is attached to the key column and the exporter hands it out.
  // Round 6: NOBODY WAITS for the copy.  Round 2 found the DMA engine's device-to-host copies stalling for 6-150 ms once in a few
  // hundred calls (that is why the result itself is downloaded by a kernel), and emit used to sit in hipEventSynchronize behind
  // this one.  Now emit asks (hipEventQuery): a copy that has not finished is RETIRED -- its event, its buffers and the table
  // it reads (`keep`) move to a list that is emptied as the events complete -- and the step takes the path it would have taken
  // without the copy (+0.15 ms, not +100).
  struct EarlyKeys {
    bool armed = false;
    uint64_t occupied = 0;    // group count it was made for
    uint64_t generation = 0;  // table generation it was made from
    size_t bytes = 0;
    std::shared_ptr<void> host, total;          // pinned: the column, the compaction's own group count
    std::vector<std::shared_ptr<void>> scratch;  // device buffers the side stream is still using
    std::vector<std::shared_ptr<void>> keep;     // the table planes its kernels read (alive until they have run)
    hipEvent_t done = nullptr, start = nullptr;
    struct Retired {
      hipEvent_t done;
      std::vector<std::shared_ptr<void>> buffers;
    };
    std::vector<Retired> retired;
    bool ready() const { return !armed || !done || hipEventQuery(done) == hipSuccess; }
    void reap(bool block) {  // retired copies whose side-stream work has finished give their buffers back
      for (size_t i = 0; i < retired.size();) {
        if (block) (void)hipEventSynchronize(retired[i].done);
        if (block || hipEventQuery(retired[i].done) == hipSuccess) {
          (void)hipEventDestroy(retired[i].done);
          retired.erase(retired.begin() + (long)i);
        } else {
          ++i;
        }
      }
    }
    void drop() {  // forget the copy without waiting for it (before the table it reads is replaced, or when emit finds it unfinished)
      if (armed && done && hipEventQuery(done) != hipSuccess) {
        Retired r;
        r.done = done;
        done = nullptr;  // (a new event next time)
        r.buffers = std::move(scratch);
        r.buffers.insert(r.buffers.end(), keep.begin(), keep.end());
        r.buffers.push_back(host);
        r.buffers.push_back(total);  // (the pending copies write both)
        total.reset();
        retired.push_back(std::move(r));
      }
      armed = false;
      scratch.clear();
      keep.clear();
      host.reset();
      reap(false);
    }
    void cancel() { drop(); }
    ~EarlyKeys() {
      drop();
      reap(true);
      if (done) (void)hipEventDestroy(done);
      if (start) (void)hipEventDestroy(start);
    }
  } early;
  uint64_t table_generation = 0;
  uint64_t early_last_occupied = ~0ull;  // the group count of the previous snapshot
  Status early_keys_maybe();
  Status emit_ungrouped(DeviceBatch* out);
  ~Impl() {
    if (ctl.pending[0] || ctl.pending[1]) (void)hipStreamSynchronize(ctx().aux);  // snapshots still in flight
    for (int i = 0; i < 2; ++i) {
      if (ctl.ev[i]) (void)hipEventDestroy(ctl.ev[i]);
      if (ctl.main_ev[i]) (void)hipEventDestroy(ctl.main_ev[i]);
    }
  }
};

}  // namespace dfx
