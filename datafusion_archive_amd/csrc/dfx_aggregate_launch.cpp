// dfx_aggregate_launch.cpp -- AggregateRelation: the routing regions of the partitioned strategy (Pass2Window), the launches of one slice of rows.
#include "dfx_aggregate_impl.hpp"

namespace dfx {

// the active chunk's 2..3 aggregates all take the same operand (AVG's SUM and COUNT, SUM + MIN + MAX of one column ...):
// with narrow keys and no nulls in this batch, routed rows carry that one operand (PTF_SHARED)
bool AggregateRelation::Impl::shared_operand() const {
  if (kw != 1 || na() < 2 || na() > 3 || !opt().shared_operand) return false;
  for (int a = 1; a < na(); ++a)
    if (active().plan.arg[a] != active().plan.arg[0]) return false;
  return true;
}

// what choose_routed_layout (dfx_pass1_layout.hpp) is asked for a batch of `rows` rows; both_shadows: launch_rows' both_shadows_bind
RoutedLayoutQuery AggregateRelation::Impl::layout_query(int64_t rows, bool nulls_now, bool both_shadows) const {
  RoutedLayoutQuery q = {};
  q.rows = rows, q.nulls_now = nulls_now, q.kw = kw, q.na = na();
  q.table_slots = T.mask + 1, q.block_slots = (uint64_t)T.block_mask + 1, q.cu_count = device_cu_count();
  q.phase = !pair_scan() ? PairPhase::none : split_is_shared ? PairPhase::planes : PairPhase::pair;
  q.split_distinct = split_distinct, q.split_ops = split_ops, q.split_arg1 = split_arg1;
  q.shared_operand = shared_operand(), q.same_operand_all = same_operand_all();
  q.has_pred = has_pred, q.unfused_now = unfused_now;
  q.narrow = dec.narrow, q.dense_seen = dec.dense_seen, q.mostly_seen = dec.mostly_seen, q.skew_seen = dec.skew_seen;
  q.opt = layout_options();
  q.both_shadows = both_shadows && opt().routed_row8 != 0;
  return q;
}

// scratch for the partitioned strategy, sized for a batch of `rows` rows (worst case: all pass).  The policy -- which pass-1 flavour
// routes the rows, the row form, the regions' geometry -- is choose_routed_layout (dfx_pass1_layout.hpp)
Status AggregateRelation::Impl::ensure_partition(int64_t rows, bool nulls_now, bool both_shadows) {
  const RoutedLayout L = choose_routed_layout(layout_query(rows, nulls_now, both_shadows));
  if (L.kind == RoutedLayoutKind::refused_pair_scan) return Status::Err(DFX_NOT_IMPLEMENTED, "pair scan: not for this table");
  const uint32_t form = PTF_NARROW | PTF_SHARED | PTF_PAIR | PTF_PLANES | PTF_ROW8;  // (pass 2 reads a window in ONE row form)
  if (win.layout_valid && rows <= win.layout_rows && PT.n_parts == L.PT.n_parts && PT.n_words == L.PT.n_words && (PT.flags & form) == L.want_flags)
    return Status::OK();  // same table, a batch the regions were sized for: keep appending
  DFX_RETURN_IF_ERROR(flush_pass2());  // rows routed under the old layout
  win.layout_valid = false;
  PT = L.PT;
  if (L.kind == RoutedLayoutKind::refused_table_blocks) return Status::Err(DFX_NOT_IMPLEMENTED, "partitioned strategy: too many table blocks");
  win.worst = L.worst;
  Status st;
  ScopedUs t_alloc(&counters().agg_alloc_us);
  if (!win.rows || win.rows_bytes < L.row_bytes) {
    win.rows.reset();
    win.rows = device_alloc(L.row_bytes, &st);
    if (!win.rows) return st;
    win.rows_bytes = L.row_bytes;
  }
  if (!win.counts || win.cnt_bytes < L.cnt_bytes) {
    win.counts.reset();
    win.counts = device_alloc(L.cnt_bytes, &st);
    if (!win.counts) return st;
    win.cnt_bytes = L.cnt_bytes;
  }
  PT.rows = (uint64_t*)win.rows.get();
  PT.counts = (uint32_t*)win.counts.get();
  win.layout_valid = true;
  win.layout_rows = rows;
  win.closed();
  return Status::OK();
}

// pass 2 over everything the pending pass-1 launches routed (no-op when nothing is pending)
Status AggregateRelation::Impl::flush_pass2(uint32_t* snap_to) {
  if (win.pending == 0) return Status::OK();
  ++counters().agg_pass2_launches;
  if (win.pending > 1) ++counters().agg_deferred_windows;
  DevPartition pt = PT;
  if (snap_to) pt.snap_host = snap_to, pt.snap_done = (uint32_t*)win.snap_done.get();
  DFX_HIP(launch_partition_agg(T, pt, spill, 0, ctx().stream));
  win.closed();
  win.last_p2_seq = ctl.batch_seq;
  return Status::OK();
}

// the bound columns advanced to row0 (a multiple of 64); *bytes: what a launch over n rows of them reads
static void slice_at(const DevProgram& prog, DevColumns* cols, int64_t row0, int64_t n, double* bytes) {
  *bytes = 0;
  for (int i = 0; i < prog.n_cols; ++i) {
    const int w = prog.col_dtype[i] == T_BOOL ? 0 : dtype_width(prog.col_dtype[i]);
    if (w) cols->c[i].values = (const uint8_t*)cols->c[i].values + (size_t)row0 * w;
    else cols->c[i].bit_offset += row0;
    if (cols->c[i].validity && w) cols->c[i].bit_offset += row0;
    *bytes += (double)n * (w ? w : 0.125);
  }
}

// The launch's program, columns and DevPartition (it starts from PT, which is laid out) with the column shadows bound where they bind.
// prog_in, cols_in: the batch as the operator bound it (before row0); *prog, *cols: the slice (slice_at); *bytes: what the launch reads
Status AggregateRelation::Impl::bind_shadows(const DevProgram& prog_in, const DevColumns& cols_in, const DevFastPlan& fpp, int64_t row0, int64_t n,
                                             int64_t layout_rows, DevProgram* prog, DevColumns* cols, DevPartition* pt_out, double* bytes) {
  DevPartition pt = PT;
  pt.flags &= ~PTF_ROW8;  // (the shadows first: the form is put back below once both are bound)
  if (win.pending > 0) pt.flags |= PTF_RESUME;
  // the key column's Int32 shadow, bound in place of the column for this launch: 12 bytes per row.  Everything behind the
  // hash image -- routed rows, pass 2, the table, the result's Int64 key column -- is what it was
  if (const uint32_t* key_words = key_shadow_words(prog_in, fpp, cols_in, pt)) {
    const int ks = fpp.keycol[0];
    cols->c[ks].values = key_words + row0;
    prog->col_dtype[ks] = T_U32;
    pt.flags |= PTF_KEY4;
    *bytes -= 4.0 * (double)n;
    ++counters().agg_key_shadow_launches;
    ++shadows.key_shadow_launches;
    // ... and the operand's Float32 shadow beside it, where every value of the column is exactly its float: 8 bytes per row.
    // The scanners widen it back to the column's own bits; predicate, routed rows and everything behind them are what they were
    int vc = 0;
    if (const uint32_t* value_words = value_shadow_words(*prog, fpp, cols_in, pt, &vc)) {
      cols->c[vc].values = value_words + row0;
      prog->col_dtype[vc] = T_F32;
      pt.flags |= PTF_VAL4;
      *bytes -= 4.0 * (double)n;
      ++counters().agg_value_shadow_launches;
      ++shadows.value_shadow_launches;
      if (!shadows.routed_keys) {  // (the pair a routed shadow would be of: routed_shadow_maybe, after the last batch)
        int64_t at = 0;
        if (!routed_pair(prog_in, fpp, cols_in, &shadows.routed_keys, &shadows.routed_values, &shadows.routed_rows, &at)) shadows.routed_keys = nullptr;
      }
    }
  }
  if (PT.flags & PTF_ROW8) {
    if (pt.flags & PTF_VAL4) {
      pt.flags |= PTF_ROW8;
      ++counters().agg_row8_launches;
      ++shadows.row8_launches;
    } else {
      // a shadow that was there a moment ago did not bind after all (memory, a slice off the 64-row grid): 8-byte regions never
      // meet such a launch -- close the window, lay the regions out for 12-byte rows
      DFX_RETURN_IF_ERROR(ensure_partition(layout_rows, prog->has_nulls != 0, false));
      const uint32_t keep = pt.flags & (PTF_KEY4 | PTF_VAL4);
      pt = PT;
      pt.flags |= keep;  // (nothing is pending after the flush: no PTF_RESUME)
    }
  }
  *pt_out = pt;
  return Status::OK();
}

// pass 1 of this slice into the routing regions and, when the window closes with it, pass 2 over the window.  The LAST kernel of
// the batch publishes the control block (arm_snapshot): pass 1, or the closing pass 2
Status AggregateRelation::Impl::launch_routed(const DevProgram& prog, const DevFastPlan& fpp, const DevColumns& cols, const DevAggPlan& p, DevPartition pt, int64_t n, double bytes) {
  const bool close_window = window_closes();
  uint32_t* snap_to = nullptr;
  DFX_RETURN_IF_ERROR(arm_snapshot(&snap_to));
  if (!close_window) pt.snap_host = snap_to, pt.snap_done = (uint32_t*)win.snap_done.get();
  DFX_HIP(launch_partition(prog, fpp, cols, p, T, pt, spill, n, bytes, ctx().stream));
  if (pt.flags & PTF_SHARED) ++counters().agg_shared_operand_launches;
  if (pt.flags & PTF_PAIR) ++counters().agg_pair_launches;
  if (pt.flags & PTF_PLANES) ++counters().agg_plane_launches;
  if (pt.flags & PTF_HOT) ++counters().agg_hot_key_launches;
  ++win.pending;
  win.fill_bound += win.worst;
  win.rows_in_flight += n;
  return close_window ? flush_pass2(snap_to) : Status::OK();
}

// rows straight into the table (no routing)
Status AggregateRelation::Impl::launch_table(const DevProgram& prog, const DevColumns& cols, DevAggPlan p, int64_t n, double bytes) {
  hipStream_t s = ctx().stream;
  const DevFastPlan fp = fast_plan();
  // a handful of groups (the calibration slice / earlier batches saw <= 8): register accumulators.  Should more
  // groups turn up later the kernel still handles them (through the table), and the next batch goes back to K7.
  if (dec.lds_enabled && dec.calibrated && !calibrating && opt().strategy != 1 && opt().fewgroup &&
      dec.occupied_known > 0 && dec.occupied_known <= 8 && fewgroup_supported(prog, fp, T)) {
    DFX_HIP(launch_fewgroup_agg(prog, fp, cols, p, T, spill, n, bytes, s));
    ++counters().agg_fewgroup_launches;
    return Status::OK();
  }
  FrontCacheShape cache = {0, 1};  // (no front cache)
  if (dec.lds_enabled && opt().strategy != 1) cache = front_cache_shape(opt().lds_slots, opt().lds_copies, calibrating, dec.calibrated, dec.occupied_known, kw, na());
  p.lds_slots = cache.slots, p.lds_copies = cache.copies;
  DFX_HIP(launch_hash_agg(prog, fp, cols, p, T, spill, n, bytes, s));
  return Status::OK();
}

Status AggregateRelation::Impl::launch_rows(const DeviceBatch& b, const DevProgram& prog_in, const DevColumns& cols_in,
                                            int64_t row0, int64_t n) {
  win.snap_armed = false;
  DevProgram prog = prog_in;
  DevColumns cols = cols_in;
  double bytes = 0;
  slice_at(prog, &cols, row0, n, &bytes);
  const DevAggPlan p = active().plan;
  bool partition_now = dec.use_partition && partition_allowed();
  const int64_t layout_rows = launch_rows_hint > 0 ? std::max<int64_t>(n, std::min<int64_t>(launch_rows_hint, b.num_rows)) : std::max<int64_t>(n, b.num_rows);  // (the slice after the calibration rows: size for the whole batch)
  if (partition_now) {
    // the row form is the layout's: ask first whether this launch will bind both shadows (8-byte rows), then lay out.  A launch
    // that will not closes a pending window of 8-byte rows here (the form differs: flush_pass2, regions laid out again)
    const bool both = both_shadows_bind(prog_in, fast_plan(), cols_in, layout_rows, row0);
    if (both) {  // exactly one window of the table's routed shadow: one kernel, no routing
      bool took = false;
      DFX_RETURN_IF_ERROR(routed_shadow_launch(prog_in, fast_plan(), cols_in, row0, n, &took));
      if (took) return Status::OK();
    }
    Status pst = ensure_partition(layout_rows, prog.has_nulls != 0, both);
    if (!pst.ok() && pst.code == DFX_NOT_IMPLEMENTED) partition_now = false;  // global-atomic path instead
    else if (!pst.ok()) return pst;
  }
  if (!partition_now) return launch_table(prog, cols, p, n, bytes);
  const DevFastPlan fpp = fast_plan();
  DevPartition pt;
  DFX_RETURN_IF_ERROR(bind_shadows(prog_in, cols_in, fpp, row0, n, layout_rows, &prog, &cols, &pt, &bytes));
  return launch_routed(prog, fpp, cols, p, pt, n, bytes);
}

}  // namespace dfx
