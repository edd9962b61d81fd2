// dfx_aggregate_strategy.cpp -- AggregateRelation: one input batch through the strategy state machine (calibration slice, memo,
// the split into scans per aggregate, pair scan / planes and their fall-back, held batches).
#include "dfx_aggregate_impl.hpp"

namespace dfx {

namespace {
// one batch as a relation (input of the per-batch FilterRelation of the unfused path)
struct OneBatchRelation : Relation {
  DeviceBatch batch;
  SchemaInfo schema_;
  bool done = false;
  RelationKind kind() const override { return REL_TABLE_SCAN; }
  const SchemaInfo& schema() const override { return schema_; }
  Status next(DeviceBatch* out, bool* has) override {
    *has = !done;
    if (!done) *out = batch;
    done = true;
    return Status::OK();
  }
};
}  // namespace

// the forced strategy (agg.strategy = 3): no calibration slice -- optimistic about the keys (tests); ensure_partition looks at the shape
void AggregateRelation::Impl::force_partition_maybe() {
  if (opt().strategy != 3 || kw != 1) return;
  if (!dec.use_partition && opt().narrow_keys > 0) dec.narrow = true;
  dec.use_partition = true;
}

// what follows from the group count in dec.occupied_known (the calibration slice's, or the memo's), for a batch of n rows
Status AggregateRelation::Impl::apply_group_count(int64_t n) {
  dec.apply_group_count(kw);
  if (dec.use_partition) DFX_RETURN_IF_ERROR(ensure_spill(2 * n + (int64_t)std::max(1, opt().partition_defer_batches) * n + 65536));
  return Status::OK();
}

Status AggregateRelation::Impl::consume_batch_chunk(const DeviceBatch& b, int64_t* decided) {
  plan_required = false;
  if (has_pred && !unfused_now && b.num_rows > 0) {
    bool nulls = false;
    for (int ci : active().builder->columns())
      if (ci >= 0 && ci < (int)b.columns.size() && b.columns[(size_t)ci].validity && b.columns[(size_t)ci].null_count != 0) nulls = true;
    if (pred_terms.source_has_nulls(b)) nulls = true;  // (a string term's own column: the Filter's all-valid output decides what the aggregate sees)
    // A scan plan evaluates the fused form with exactly those rules -- a null judged by arrow's comparison rule, every
    // surviving slot valid, value(row) read regardless (DevScanPlan::count_valid) -- in one pass: no materialised filter.
    if (nulls && opt().plan != 0 && opt().fast != 0 && scan_plan_shape_ok(active().builder->program(), active().fast, kw, na(), val_xform())) {
      nulls = false;
      plan_required = true;  // (this batch's launchers must bind the plan: nothing else evaluates the fused form correctly)
    }
    if (nulls) {  // FilterRelation for real (its output is all-valid), then the predicate-free program
      std::unique_ptr<OneBatchRelation> one(new OneBatchRelation());
      one->batch = b;
      one->schema_ = input->schema();
      FilterRelation filter(std::move(one), pred, input->schema());
      std::vector<char> needed(input->schema().fields.size(), 0);
      mark_columns(&needed, cur().np.builder->columns());
      for (const DictKey& d : dicts)
        if (d.src_col >= 0 && d.src_col < (int)needed.size()) needed[(size_t)d.src_col] = 1;
      filter.require_columns(needed);
      DeviceBatch fb;
      bool got = false;
      DFX_RETURN_IF_ERROR(filter.next(&fb, &got));
      if (!got) return Status::OK();
      unfused_now = true;  // (active(): the predicate-free programs)
      ++counters().agg_unfused_batches;
      Status st = consume_batch_chunk(fb);  // (the filtered batch is this call's own: it is consumed whole, whatever is decided on the way)
      if (decided) *decided = b.num_rows;
      unfused_now = false;
      return st;
    }
  }
  // The absorbed FilterRelation's batch-level error survives the fusion: fn filter has no arm for Boolean
  // (filter.rs:105-108), so a batch with a Boolean column fails under a Filter whether or not anybody reads that column
  // and whether this batch runs fused (no nulls) or through a real FilterRelation (nulls in the program's columns)
  if (has_pred && !unfused_now)
    for (size_t c = 0; c < b.columns.size(); ++c)
      if (b.columns[c].dtype == DFX_BOOLEAN) return Status::Err(DFX_EXECUTION_ERROR, "filter not supported for Boolean");
  const int64_t n = b.num_rows;
  if (n == 0 && kw > 0) return Status::OK();  // (ungrouped: an empty batch still folds Some(0) into COUNT)
  hipStream_t s = ctx().stream;
  DevProgram prog;
  DevColumns cols;
  const bool terms_now = has_pred && !unfused_now && !pred_terms.empty();
  if (dicts.empty() && !terms_now) {
    DFX_RETURN_IF_ERROR(active().builder->bind(b, &prog, &cols));
  } else {  // append the id column of every Utf8 key and the bitmap of every string term of the absorbed predicate
    DeviceBatch ab = b;
    ab.columns.resize(bind_schema.fields.size());
    for (DictKey& d : dicts) {
      if (d.src_col >= (int)b.columns.size() || b.columns[d.src_col].dtype != DFX_UTF8)
        return Status::Err(DFX_INTERNAL_ERROR, "GROUP BY key column is not Utf8 in this batch");
      DFX_RETURN_IF_ERROR(d.dict.encode(b.columns[d.src_col], n, opt().dict_capacity_log2, &ab.columns[d.virt_col]));
    }
    if (terms_now) {
      const std::vector<Utf8TermSpec>& ts = pred_terms.terms();
      const void* key = ts[0].src_col < (int)b.columns.size() ? (const void*)b.columns[(size_t)ts[0].src_col].offsets : nullptr;
      const TermCacheEntry* hit = nullptr;
      if (term_cache_on && key)
        for (const TermCacheEntry& e : term_cache)
          if (e.offsets == key && e.rows == n) hit = &e;
      if (hit) {
        for (size_t k = 0; k < ts.size(); ++k) ab.columns[(size_t)ts[k].virt_col] = hit->cols[k];
      } else {
        DFX_RETURN_IF_ERROR(pred_terms.eval(b, &ab));
        if (term_cache_on && key) {
          TermCacheEntry e;
          e.offsets = key;
          e.rows = n;
          for (const Utf8TermSpec& t : ts) e.cols.push_back(ab.columns[(size_t)t.virt_col]);
          term_cache.push_back(std::move(e));
        }
      }
    }
    DFX_RETURN_IF_ERROR(active().builder->bind(ab, &prog, &cols));
  }
  if (kw == 0) {
    double bytes = 0;
    for (int i = 0; i < prog.n_cols; ++i) bytes += (double)n * (prog.col_dtype[i] == T_BOOL ? 0.125 : dtype_width(prog.col_dtype[i]));
    DFX_HIP(launch_reduce(prog, fast_plan(), cols, active().plan, T, n, (uint64_t*)cur().partial.get(), (uint32_t*)ctrl.get(), bytes, s));
    DFX_HIP(launch_reduce_fold(T, (const uint8_t*)cur().dev_arg_dtype.get(), (const uint8_t*)cur().dev_func.get(),
                               (uint64_t*)cur().partial.get(), (uint64_t*)cur().state.get(), (uint32_t*)ctrl.get(), s));
    rows_seen += n;
    return Status::OK();
  }
  // grouped: can this batch overflow the table in the worst case (every row a new group)?
  force_partition_maybe();
  const bool may_spill = dec.use_partition || dec.occupied_known + ctl.unconfirmed_rows + (uint64_t)n > T.load_limit;
  // two batches can be in flight unchecked; with a deferred pass 2 every row of the window may still be spilled (by pass 2
  // itself, when its block is full)
  // (pair scan: a row whose key finds no slot in its block is spilled once per OPERAND -- by the last plane of each, dfx_k_pass2.hip --;
  // planes of a shared operand: once.  Their windows hold at most two batches, launch_rows)
  const int64_t window_rows = spill_window_rows(dec.use_partition, pair_scan(), split_is_shared, opt().partition_defer_batches, n, win.layout_rows);
  if (may_spill) DFX_RETURN_IF_ERROR(ensure_spill(2 * n + window_rows + 65536));
  T.max_probe = may_spill ? 128 : (int)std::min<uint64_t>(T.mask + 1, 1u << 30);
  int64_t row0 = 0;
  const AggOptions& o = opt();
  // (a batch that went through a real FilterRelation is not the table's first rows: its calibration says nothing about them)
  ScanMemo* memo = (o.calibration_memo && !unfused_now) ? input->scan_memo() : nullptr;
  uint64_t remembered = 0;
  if (!dec.calibrated && o.strategy == 0 && n > (1 << 21) && memo && memo->lookup(program_fingerprint(), &remembered)) {
    // an earlier query of this shape over the same resident table already ran the calibration slice: same decision,
    // no slice, no synchronous read-back (the real group count arrives with the control-block snapshots as always)
    dec.unpack(remembered);
    ++counters().agg_memo_decisions;
    DFX_RETURN_IF_ERROR(apply_group_count(n));
  }
  if (!dec.calibrated && o.strategy == 0 && n > (1 << 21)) {
    // calibration slice: measure the LDS front-cache hit rate and the group count on the first
    // 2^18 rows before committing the rest of the stream to a strategy
    const int64_t n0 = 1 << 18;
    ++counters().agg_calibrations;
    calibrating = true;
    Status cst = launch_rows(b, prog, cols, 0, n0);
    calibrating = false;
    DFX_RETURN_IF_ERROR(cst);
    if (kw == 1) DFX_HIP(launch_probe_wide_keys(T, ctx().stream));  // does any key of the slice lack a 32-bit image?
    uint32_t hc[CTRL_WORDS];
    DFX_RETURN_IF_ERROR(read_ctrl(hc));
    if (hc[CTRL_ERROR]) return error_from_ctrl(hc[CTRL_ERROR]);
    if (ctrl_spilled(hc) > 0 || hc[CTRL_SATURATED]) {
      // The slice did not fit the table (a table that starts very small: agg.capacity_log2): its spilled rows sit in the spill list
      // that the strategy decision below is about to REPLACE by a larger one.  Round 6, found by a test of the pair scan at 2^14
      // slots: nothing replayed them first -- the spill cursor went on counting them, the rebuild after the batch replayed whatever
      // the new list's memory held in their place (60-80 of 200 000 groups missing, or keys that never were in the data).  Grow /
      // replay now; the decision then reads the real group count of the slice.
      ++counters().agg_calibration_replays;
      DFX_RETURN_IF_ERROR(handle_ctrl(hc, n0));
      DFX_RETURN_IF_ERROR(read_ctrl(hc));
      if (hc[CTRL_ERROR]) return error_from_ctrl(hc[CTRL_ERROR]);
    }
    // (a property of the KEYS: whether a launch routes 12-byte rows also depends on the aggregates of the chunk it serves --
    // ensure_partition -- and a query that is split into one scan per aggregate has one-aggregate chunks after this point)
    dec.narrow = kw == 1 && hc[CTRL_WIDE_KEYS] == 0;
    // strategy from the number of groups the calibration slice produced: the LDS front cache pays
    // when the groups fit it (every later row is an LDS atomic); for many groups per-row global
    // atomics would cap the query near 24 G rows/s, so rows are routed to their table blocks
    // instead (dfx_k_partition.hip); in between, the global table alone.
    dec.occupied_known = hc[CTRL_OCCUPIED];
    {  // share of the slice's rows that a 512-slot front cache absorbed: ~0 for a million uniform keys, a third and
       // more under a Zipf-like distribution (statistics stripes of K7; one more small synchronous copy, once per stream)
      std::vector<uint64_t> hs((size_t)kStatStripes * STAT_WORDS, 0);
      DFX_HIP(hipMemcpy(hs.data(), stats.get(), sizeof(uint64_t) * hs.size(), hipMemcpyDeviceToHost));
      uint64_t hit = 0, miss = 0, passed = 0;
      for (int i = 0; i < kStatStripes; ++i) {
        hit += hs[(size_t)i * STAT_WORDS + STAT_LDS_HIT];
        miss += hs[(size_t)i * STAT_WORDS + STAT_LDS_MISS];
        passed += hs[(size_t)i * STAT_WORDS + STAT_PASSED];
      }
      dec.dense_seen = passed * 2 > (uint64_t)n0;
      dec.mostly_seen = passed * 3 > (uint64_t)n0 * 2;
      dec.skew_seen = dec.occupied_known >= kPartitionGroupsMin && miss > 0 && hit * 8 >= miss;  // (`miss` counts every row that went through the cache) >= 12.5 % reused although the groups do not fit
    }
    if (memo) memo->remember(program_fingerprint(), dec.pack());
    DFX_RETURN_IF_ERROR(apply_group_count(n));
    row0 = n0;
  } else if (!dec.calibrated) {
    if (o.strategy == 1) dec.lds_enabled = false;
  }
  if (decided && dec.calibrated) {  // (consume_batch: the decision is what was asked for; rows [0, row0) are done)
    *decided = row0;
    rows_seen += row0;
    return Status::OK();
  }
  {  // a scan that routes most of its rows: launches of at most partition_split_rows rows (regions sized for that many)
    // (selective scans: twice that -- 2^27-row launches measured best, 2^28-row ones 7 % slower)
    int64_t split = (dec.use_partition && o.partition_split_rows >= (1 << 20)) ? (((int64_t)o.partition_split_rows * (dec.dense_seen ? 1 : 2)) & ~(int64_t)63) : 0;
    if (dec.use_partition && row0 == 0)  // (the table keeps a routed shadow of these columns: launches of whole windows, each one kernel)
      if (const int64_t w = routed_split_rows(prog, cols)) split = w;
    launch_rows_hint = split;
    Status lst = Status::OK();
    if (split > 0 && n - row0 > split) {
      for (int64_t at = row0; at < n && lst.ok(); at += split) lst = launch_rows(b, prog, cols, at, std::min(split, n - at));
    } else {
      lst = launch_rows(b, prog, cols, row0, n - row0);
    }
    launch_rows_hint = 0;
    DFX_RETURN_IF_ERROR(lst);
  }
  if (!dec.calibrated) {  // first batch of a stream that skipped the calibration slice: decide now
    uint32_t hc[CTRL_WORDS];
    DFX_RETURN_IF_ERROR(read_ctrl(hc));
    DFX_RETURN_IF_ERROR(handle_ctrl(hc, n));
    if (o.strategy == 0) dec.lds_enabled = dec.occupied_known <= kLdsGroupsMax;
    dec.calibrated = true;
  } else {
    const int prev = (int)((ctl.batch_seq & 1) ^ 1);
    DFX_RETURN_IF_ERROR(post_ctrl(n));       // snapshot of THIS batch, examined after the next launch
    DFX_RETURN_IF_ERROR(examine_ctrl(prev)); // the previous batch's snapshot (normally complete by now)
    DFX_RETURN_IF_ERROR(early_keys_maybe());
  }
  rows_seen += n;
  if (decided) *decided = n;  // (a batch too small for a calibration slice: it ran whole, decided afterwards)
  return Status::OK();
}

// One input batch through every chunk of accumulators.  With several chunks each chunk's kernels are checked
// synchronously (errors, spilled rows, growth) before the next chunk runs: the spill list and the routing scratch carry
// rows of ONE chunk's width at a time.
static DeviceBatch rows_from(const DeviceBatch& b, int64_t row0) {  // rows [row0, end) of a batch, zero copy (row0: a multiple of 64)
  DeviceBatch r;
  r.num_rows = b.num_rows - row0;
  r.columns.reserve(b.columns.size());
  for (const DeviceColumn& c : b.columns) {
    DeviceColumn s = c;
    s.length = r.num_rows;
    if (!c.absent) {
      if (c.dtype == DFX_UTF8) {
        if (c.offsets) s.offsets = c.offsets + row0;
        s.data_bytes = 0;
      } else if (c.dtype == DFX_BOOLEAN) {
        if (c.values) s.values = (const uint8_t*)c.values + (row0 >> 3);
      } else if (c.values) {
        s.values = (const uint8_t*)c.values + (size_t)row0 * dtype_width(c.dtype);
      }
      if (c.validity) s.validity = c.validity + (row0 >> 3);
      if (c.null_count != 0) s.null_count = -1;
    }
    r.columns.push_back(std::move(s));
  }
  return r;
}

Status AggregateRelation::Impl::consume_batch(const DeviceBatch& b) {
  if (phase == Phase::Undecided) {
    // The strategy decision first (calibration slice, the resident table's memo, a forced strategy), with the all-aggregates
    // program and nothing else of the batch; if it says "partitioned", the per-aggregate chunking takes over from there.
    const bool forced = opt().strategy == 3;  // (no decision to wait for: the chunk loop below turns the strategy on itself)
    int64_t decided_rows = 0;
    if (!forced) DFX_RETURN_IF_ERROR(consume_batch_chunk(b, &decided_rows));
    // decided = a strategy has been chosen.  An empty first batch (or one a real FilterRelation emptied) chooses nothing:
    // the next batch comes back here (round-4 advisor finding: a decision recorded before any calibration left a later
    // "partitioned" verdict with the split pending for good -- every launch on per-row global atomics)
    const bool split_decided = forced || dec.calibrated || (decided_rows == 0 && b.num_rows > 0);
    force_partition_maybe();  // (before the choice below looks at `narrow`)
    if (split_decided && (dec.use_partition || forced)) {
      DFX_RETURN_IF_ERROR(finish_launched(0, false));
      if ((split_is_shared ? opt().shared_planes : opt().pair_scan) && dec.use_partition && pair_batch_ok(b)) {
        phase = Phase::PairScan;  // the all-aggregates program goes on: one scan for both operands (single_chunks stays in reserve)
      } else {
        install_chunks(std::move(single_chunks));
        single_chunks.clear();
        phase = Phase::PerAggregate;
      }
    } else if (split_decided) {
      phase = Phase::OneScan;
    }
    if (decided_rows >= b.num_rows) return Status::OK();
    if (decided_rows == 0) return consume_batch(b);
    return consume_batch(rows_from(b, decided_rows));
  }
  if (pair_scan() && (pair_wide_seen || !pair_batch_ok(b))) DFX_RETURN_IF_ERROR(pair_fall_back());
  if (chunks.size() <= 1) return consume_batch_chunk(b);
  if (kw > 0 && opt().chunk_hold > 1) {  // grouped, several chunks: hold the batch (see `held`)
    size_t bytes = 0;
    for (const DeviceColumn& c : b.columns) bytes += (size_t)std::max<int64_t>(c.length, 0) * (size_t)std::max(1, dtype_width(c.dtype));
    held.push_back(b);
    held_bytes += bytes;
    if ((int)held.size() < opt().chunk_hold && held_bytes < ((size_t)8 << 30)) return Status::OK();
    return run_held();
  }
  TermCacheScope cache_scope(*this);
  for (int c = 0; c < (int)chunks.size(); ++c) {
    activate(c);
    const int64_t seen = rows_seen;
    DFX_RETURN_IF_ERROR(consume_batch_chunk(b));
    rows_seen = seen;
    if (kw > 0) DFX_RETURN_IF_ERROR(finish_launched(b.num_rows));
  }
  activate(0);
  rows_seen += b.num_rows;
  return Status::OK();
}

// Can this batch go through the pair scan (Phase::PairScan)?  Host work only: the program is bound to the batch and the scan plan to that.
bool AggregateRelation::Impl::pair_batch_ok(const DeviceBatch& b) {
  const bool dbg = getenv("DFX_DEBUG") != nullptr;
  auto no = [&](const char* why) {
    if (dbg) fprintf(stderr, "[dfx] pair scan: no (%s)\n", why);
    return false;
  };
  if (!kNarrowLine || !dec.narrow || kw != 1 || chunks.size() != 1 || (int)single_chunks.size() != na() || !dicts.empty() || unfused_now) return no("shape");
  if (split_is_shared ? !(na() >= 2 && na() <= kMaxAggs && same_operand_all() && opt().shared_planes) : !(split_distinct == 2 && na() >= 2 && na() <= kMaxAggs)) return no("aggregates");
  const AggOptions& o = opt();
  // Skewed keys (the calibration slice's front cache absorbed a sizeable share of its rows): the one-value scans keep the heavy keys
  // in LDS (PTF_HOT) -- the pair rows and the planes have no such thing, a heavy key overflows its regions into the spill list and
  // the replay queues on a few addresses (Zipf(1.0), 10^9 rows: SUM(v), MIN(w) 51 ms against 12.2 for a scan per aggregate;
  // SUM(v), MIN(v) 43 ms, 96 with the all-planes blocks).  One scan per aggregate then.
  if (o.hot_keys > 0 || (o.hot_keys < 0 && dec.skew_seen)) return no("skewed keys: the one-value scans have the hot-key pairs");
  if (!split_is_shared && (!o.plan || !o.fast)) return no("options");
  if (!split_is_shared && !scan_plan_shape_ok(active().builder->program(), active().fast, kw, na(), val_xform())) return no("scan plan shape");  // (also: a predicate over nulls stays fused, consume_batch_chunk)
  const uint64_t S = (uint64_t)T.block_mask + 1;
  // (the layout's own conditions, as ensure_partition will ask them: dfx_pass1_layout.hpp)
  if (S != 8192 || !pair_layout_fits(layout_options(), (uint32_t)((T.mask + 1) / S), split_is_shared)) return no("layout options or table blocks");
  if (b.num_rows <= 0) return true;
  DevProgram prog;
  DevColumns cols;
  if (!active().builder->bind(b, &prog, &cols).ok()) return no("bind");
  const DevFastPlan fp = fast_plan(false);
  if (split_is_shared) {  // the raw operand through the one-value kernels: a null-free batch, a signature or the plan's fixed-slot binding
    if (!partition_planes_supported(prog, fp, cols, T)) return no("one-value binding of the shared operand");
  } else if (!partition_pair_supported(prog, fp, cols, T)) {
    return no("plan binding");
  }
  return true;
}

// the pair scan no longer applies: one scan per aggregate from the next batch on (a batch boundary: nothing is half launched)
Status AggregateRelation::Impl::pair_fall_back() {
  const bool flushed = win.pending > 0;
  DFX_RETURN_IF_ERROR(finish_launched(0, flushed));  // (the pass 2 just launched has no snapshot of its own: rows it spilled carry EVERY accumulator -- replay them under this view)
  ++counters().agg_pair_fallbacks;
  if (flushed) ++counters().agg_pair_fallbacks_pending;
  install_chunks(std::move(single_chunks));
  single_chunks.clear();
  phase = Phase::PerAggregate;
  if (pair_wide_seen) dec.narrow = false;  // (16-byte routed rows from here on; install_chunks has invalidated the layout)
  return Status::OK();
}

// every chunk over every held batch, one control-block check per chunk
Status AggregateRelation::Impl::run_held() {
  if (held.empty()) return Status::OK();
  std::vector<DeviceBatch> hb;
  hb.swap(held);
  ++counters().agg_held_runs;
  held_bytes = 0;
  const int64_t seen = rows_seen;
  int64_t total = 0;
  for (const DeviceBatch& b : hb) total += b.num_rows;
  TermCacheScope cache_scope(*this);  // the string terms' bitmaps: once per held batch, for every chunk
  for (int c = 0; c < (int)chunks.size(); ++c) {
    activate(c);
    rows_seen = seen;
    for (const DeviceBatch& b : hb) DFX_RETURN_IF_ERROR(consume_batch_chunk(b));
    DFX_RETURN_IF_ERROR(finish_launched(total));
  }
  activate(0);
  rows_seen = seen + total;
  return Status::OK();
}

}  // namespace dfx
