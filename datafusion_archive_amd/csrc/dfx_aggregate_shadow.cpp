// dfx_aggregate_shadow.cpp -- AggregateRelation: what speaks to the resident table's ScanMemo -- the column shadows a pass-1 launch binds, the routed shadow.
#include "dfx_aggregate_impl.hpp"

namespace dfx {

// The device side of a column shadow's build (dfx_key_shadow.hpp, dfx_value_shadow.hpp) on stream s: `launch` is the streaming
// kernel that writes the 4-byte copy and ORs its verdict into one device word; build_us: the counter the attempt's wall time goes to.
typedef hipError_t (*ShadowLaunch)(const uint64_t* in, int64_t n, uint32_t* out, uint32_t* verdict, hipStream_t s);
static KeyShadowDevice shadow_device(hipStream_t s, ShadowLaunch launch, long long* build_us) {
  KeyShadowDevice dev;
  dev.free_bytes = device_free_bytes;
  dev.alloc = [](size_t bytes) { return device_alloc_optional(bytes); };
  dev.narrow = [s, launch, build_us](const void* src, int64_t rows, void* dst, uint32_t* dropped) -> bool {
    ScopedUs t_build(build_us);
    std::shared_ptr<void> word = device_alloc_optional(sizeof(uint32_t));
    if (!word) return false;
    bool ok = hipMemsetAsync(word.get(), 0, sizeof(uint32_t), s) == hipSuccess;
    ok = ok && launch((const uint64_t*)src, rows, (uint32_t*)dst, (uint32_t*)word.get(), s) == hipSuccess;
    ok = ok && hipMemcpyAsync(dropped, word.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
  };
  return dev;
}

// what this query holds -- routing regions and counts, the spill list, the table's key and accumulator planes --: a shadow is built
// only if as much stays free after it
size_t AggregateRelation::Impl::shadow_query_bytes() const {
  const int widest = widest_chunk();
  return win.rows_bytes + win.cnt_bytes + (size_t)spill.capacity * 8 * (size_t)(kw + widest) + ((size_t)T.mask + 2) * 8 * (size_t)(kw + widest);
}

int AggregateRelation::Impl::key_shadow_column(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt) const {
  const AggOptions& o = opt();
  if (o.key_shadow == 0 || calibrating || !dec.narrow || kw != 1 || !fp.valid || prog.has_nulls || !input) return -1;
  const int ks = fp.keycol[0];
  if (ks >= prog.n_cols || prog.col_dtype[ks] != T_I64 || cols.c[ks].validity) return -1;
  if (!partition_key_shadow_supported(prog, fp, cols, T, pt)) return -1;  // (no pass-1 kernel reads this shape's key from 4-byte words)
  return ks;
}

const uint32_t* AggregateRelation::Impl::key_shadow_words(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt) {
  const AggOptions& o = opt();
  const int ks = key_shadow_column(prog, fp, cols, pt);
  if (ks < 0) return nullptr;
  ScanMemo* memo = input->column_memo();
  if (!memo) return nullptr;
  const KeyShadowDevice dev = shadow_device(ctx().stream, launch_narrow_keys, &counters().agg_key_shadow_build_us);
  const bool first = !shadows.key_shadow_asked;
  shadows.key_shadow_asked = true;
  bool built = false;
  const uint32_t* words = memo->key_shadows.acquire(cols.c[ks].values, o.key_shadow, first, shadow_query_bytes(), dev, &built);
  if (built) ++counters().agg_key_shadow_builds, shadows.shadow_built_here = true;
  return words;
}

// prog, pt: the launch with the key shadow bound; cols: the batch as the operator bound it (before row0).  The kernels' own
// condition (partition_value_shadow_supported: one of the two signatures -- the operand a plain Float64 column, every predicate
// term on it, SUM or the shared raw operand) and the operator's: no nulls, no calibration slice, a resident table below.
int AggregateRelation::Impl::value_shadow_column(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt) const {
  const AggOptions& o = opt();
  if (o.value_shadow == 0 || calibrating || !(pt.flags & PTF_KEY4) || prog.has_nulls || !input) return -1;
  int vc = 0;
  if (!partition_value_shadow_supported(prog, fp, cols, T, pt, &vc) || cols.c[vc].validity) return -1;
  return vc;
}

const uint32_t* AggregateRelation::Impl::value_shadow_words(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const DevPartition& pt, int* operand_col) {
  const AggOptions& o = opt();
  const int vc = value_shadow_column(prog, fp, cols, pt);
  if (vc < 0) return nullptr;
  ScanMemo* memo = input->column_memo();
  if (!memo) return nullptr;
  const ValueShadowDevice dev = shadow_device(ctx().stream, launch_narrow_values, &counters().agg_value_shadow_build_us);
  const bool first = !shadows.value_shadow_asked;
  shadows.value_shadow_asked = true;
  bool built = false;
  const uint32_t* words = memo->value_shadows.acquire(cols.c[vc].values, o.value_shadow, first, shadow_query_bytes(), dev, &built);
  if (built) ++counters().agg_value_shadow_builds, shadows.shadow_built_here = true;
  *operand_col = vc;
  return words;
}

// prog, cols: the batch as the operator bound it (before row0).  The layout the launch would be sized by stands in for the
// launch's flags: the kernels' conditions look at the shape (PTF_WS, PTF_NARROW ...), not at the regions.
bool AggregateRelation::Impl::both_shadows_bind(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, int64_t rows, int64_t row0) {
  if (opt().routed_row8 == 0 || shadows.shadow_built_here || calibrating || !input) return false;
  const RoutedLayout L = choose_routed_layout(layout_query(rows, prog.has_nulls != 0, true));
  if (!(L.PT.flags & PTF_ROW8)) return false;  // (not the one-value wave-specialised layout)
  ScanMemo* memo = input->column_memo();
  if (!memo) return false;
  DevPartition pt = L.PT;
  const int ks = key_shadow_column(prog, fp, cols, pt);
  if (ks < 0 || !memo->key_shadows.peek(cols.c[ks].values)) return false;
  DevProgram prog4 = prog;
  prog4.col_dtype[ks] = T_U32;
  pt.flags |= PTF_KEY4;
  const int vc = value_shadow_column(prog4, fp, cols, pt);
  (void)row0;  // (a slice's shadow words start on the same multiple of 64 rows as its columns: peek looks at the column's base)
  return vc >= 0 && memo->value_shadows.peek(cols.c[vc].values) != nullptr;
}

// ---- the routed shadow (dfx_routed_shadow.hpp) --------------------------------------------------------------------------------------
bool AggregateRelation::Impl::routed_pair(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, const void** keys, const void** values, int64_t* rows,
                                          int64_t* row) const {
  if (!input || !fp.valid || prog.n_cols != 2 || fp.keycol[0] >= 2) return false;
  ScanMemo* memo = input->column_memo();
  if (!memo) return false;
  const int ks = fp.keycol[0];
  int64_t krows = 0, vrows = 0, krow = 0, vrow = 0;
  *keys = memo->key_shadows.column_of(cols.c[ks].values, &krows, &krow);
  *values = memo->value_shadows.column_of(cols.c[1 - ks].values, &vrows, &vrow);
  if (!*keys || !*values || krows != vrows || krow != vrow) return false;
  *rows = krows;
  *row = krow;
  return true;
}

int64_t AggregateRelation::Impl::routed_split_rows(const DevProgram& prog, const DevColumns& cols) const {
  if (opt().routed_shadow == 0 || kw != 1 || na() != 1) return 0;
  const void *keys = nullptr, *values = nullptr;
  int64_t rows = 0, row = 0;
  if (!routed_pair(prog, fast_plan(), cols, &keys, &values, &rows, &row)) return 0;
  return input->column_memo()->routed_shadows.window_rows_of(keys, values);
}

// A window's geometry is a layout's DevPartition (pointers aside) and the table's mapping of images to partitions ...
static RoutedGeometry routed_geometry(const DevPartition& pt, const DevTable& T) {
  RoutedGeometry g;
  g.part_stride = pt.part_stride, g.prod_stride = pt.prod_stride, g.win_stride = pt.win_stride;
  g.n_parts = pt.n_parts, g.n_producers = pt.n_producers, g.cap_rows = pt.cap_rows, g.n_words = pt.n_words, g.part_shift = pt.part_shift;
  g.flags = pt.flags, g.shift = T.shift, g.block_slots = T.block_mask + 1;
  return g;
}

// ... and back: the launch's DevPartition over a window's regions.  (A field of the one is a field of the other: add it to both.)
static DevPartition routed_partition(const RoutedGeometry& g, void* regions, void* counts) {
  DevPartition pt = {};
  pt.rows = (uint64_t*)regions, pt.counts = (uint32_t*)counts;
  pt.part_stride = g.part_stride, pt.prod_stride = g.prod_stride, pt.win_stride = g.win_stride;
  pt.n_parts = g.n_parts, pt.n_producers = g.n_producers, pt.cap_rows = g.cap_rows, pt.n_words = g.n_words, pt.part_shift = g.part_shift;
  pt.mode = 2u, pt.block = 1024u, pt.flags = g.flags;
  return pt;
}

// prog, fp, cols: the batch as the operator bound it (both_shadows_bind said yes: one SUM of the plain operand column, every
// predicate term on it, no nulls, no calibration slice).  [row0, row0 + n) must be exactly one window, routed for this table's
// geometry; a table that grew, another block count, a slice off the grid keep the two passes.
Status AggregateRelation::Impl::routed_shadow_launch(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, int64_t row0, int64_t n, bool* took) {
  *took = false;
  if (opt().routed_shadow == 0 || calibrating || kw != 1 || na() != 1 || T.acc_kind[0] != ACC_ADD_F64 || T.val_xform[0] != VT_RAW) return Status::OK();
  if (fp.np != 0 && fp.np != 2) return Status::OK();
  const void *keys = nullptr, *values = nullptr;
  int64_t col_rows = 0, at = 0;
  if (!routed_pair(prog, fp, cols, &keys, &values, &col_rows, &at)) return Status::OK();
  RoutedWindow w;
  const uint32_t n_parts = (uint32_t)((T.mask + 1) / ((uint64_t)T.block_mask + 1));
  if (!input->column_memo()->routed_shadows.bind(keys, values, at + row0, n, opt().routed_shadow, T.shift, T.block_mask + 1, n_parts, &w)) return Status::OK();
  DevRowPred pred = {};
  pred.np = (uint32_t)fp.np;
  const int vc = 1 - fp.keycol[0];
  for (int i = 0; i < fp.np; ++i) {
    if (fp.term[i].col != vc || fp.term[i].dtype != T_F64) return Status::OK();  // (the signatures' terms: on the operand, as Float64)
    pred.imm[i] = fp.term_imm[i], pred.m[i] = fp.term[i].m, pred.inv[i] = fp.term[i].inv;
  }
  DFX_RETURN_IF_ERROR(flush_pass2());  // (a pending window of routed rows first: the two paths may alternate, they aggregate into the same table)
  hipStream_t s = ctx().stream;
  DevPartition pt = routed_partition(w.g, w.regions.get(), w.counts.get());
  // the kernel publishes the control block itself, as a window's closing pass 2 does (post_ctrl)
  DFX_RETURN_IF_ERROR(arm_snapshot(&pt.snap_host));
  if (pt.snap_host) pt.snap_done = (uint32_t*)win.snap_done.get();
  DFX_HIP(launch_partition_scan(T, pt, spill, pred, 8.0 * (double)n, s));
  win.last_p2_seq = ctl.batch_seq;
  ++counters().agg_routed_shadow_launches;
  ++shadows.routed_shadow_launches;
  *took = true;
  return Status::OK();
}

// After the query's last batch.  The build is the existing dense wave-specialised pass 1 over both column shadows (the SigKeySum
// kernels of the key4 unit: SELECT k, SUM(v) GROUP BY k, every row routed), window by window into that window's own regions, in
// launches of agg.partition_split_rows rows with PTF_RESUME; no pass 2.  It runs against a control block of its own and no spill
// list: a row that finds no place in a region is counted there and nowhere else, and the count refuses the shadow for good.
Status AggregateRelation::Impl::routed_shadow_maybe() {
  const AggOptions& o = opt();
  if (o.routed_shadow == 0 || !shadows.routed_keys || !input || !dec.use_partition || !dec.narrow || kw != 1 || na() != 1 || chunks.size() != 1) return Status::OK();
  if (T.acc_kind[0] != ACC_ADD_F64 || T.val_xform[0] != VT_RAW || o.routed_row8 == 0) return Status::OK();
  ScanMemo* memo = input->column_memo();
  if (!memo || memo->routed_shadows.state_of(shadows.routed_keys, shadows.routed_values) > 0) return Status::OK();  // (built or refused already)
  const uint32_t* key_words = memo->key_shadows.peek(shadows.routed_keys);
  const uint32_t* value_words = memo->value_shadows.peek(shadows.routed_values);
  if (!key_words || !value_words) return Status::OK();
  hipStream_t s = ctx().stream;
  Status ast;
  std::shared_ptr<void> bctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &ast);
  if (!bctrl) return Status::OK();  // (dropped: the next query asks again)
  if (hipMemsetAsync(bctrl.get(), 0, sizeof(uint32_t) * CTRL_WORDS, s) != hipSuccess) {
    (void)hipGetLastError();
    return Status::OK();
  }
  DevTable Tb = T;
  Tb.ctrl = (uint32_t*)bctrl.get();
  Tb.stats = nullptr;
  RoutedShadowDevice dev;
  dev.free_bytes = device_free_bytes;
  dev.alloc = [](size_t bytes) { return device_alloc_optional(bytes); };
  dev.layout = [this](int64_t rows) -> RoutedWindowLayout {
    RoutedLayoutQuery q = layout_query(rows, false, true);
    q.has_pred = false, q.unfused_now = false, q.dense_seen = true, q.mostly_seen = true, q.skew_seen = false;  // every row is routed
    const RoutedLayout L = choose_routed_layout(q);
    RoutedWindowLayout l;
    if (L.kind != RoutedLayoutKind::ring16 || !(L.PT.flags & PTF_ROW8) || !partition_launchable(L.PT)) return l;
    l.g = routed_geometry(L.PT, T);
    l.region_bytes = L.row_bytes, l.count_bytes = L.cnt_bytes;
    shadows.ws_scanners_of_build = L.PT.ws_scanners;
    return l;
  };
  dev.route = [&](int64_t row0, int64_t rows, const RoutedGeometry& g, void* regions, void* counts) -> bool {
    DevProgram P = {};
    P.n_cols = 2, P.col_dtype[0] = T_U32, P.col_dtype[1] = T_F32;
    DevFastPlan F = {};
    F.valid = 1, F.np = 0, F.keycol[0] = 0;
    F.arg[0].nf = 1, F.arg[0].f[0].kind = FF_COL, F.arg[0].f[0].col = 1;
    DevAggPlan plan = {};
    plan.pred = kNoOperand;
    const int64_t split = o.partition_split_rows >= (1 << 20) ? ((int64_t)o.partition_split_rows & ~(int64_t)63) : rows;
    for (int64_t at = 0; at < rows; at += split) {
      const int64_t n = std::min(split, rows - at);
      DevColumns C = {};
      C.c[0].values = key_words + row0 + at;
      C.c[1].values = value_words + row0 + at;
      DevPartition pt = routed_partition(g, regions, counts);
      pt.ws_scanners = shadows.ws_scanners_of_build;
      pt.flags |= PTF_KEY4 | PTF_VAL4 | (at > 0 ? PTF_RESUME : 0u);
      if (launch_partition(P, F, C, plan, Tb, pt, no_spill_rows(), n, 8.0 * (double)n, s) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
    }
    return true;
  };
  dev.finish = [&](uint64_t* spilled, uint32_t* error) -> bool {
    uint32_t hc[CTRL_WORDS];
    bool ok = hipMemcpyAsync(hc, bctrl.get(), sizeof(hc), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      return false;
    }
    *spilled = ctrl_spilled(hc);
    *error = hc[CTRL_ERROR];
    return true;
  };
  int64_t w_rows = (int64_t)o.routed_shadow_window_rows & ~(int64_t)63;
  if (w_rows < 64) w_rows = kRoutedWindowRows;
  bool built_now = false;
  {
    ScopedUs t_build(&counters().agg_routed_shadow_build_us);
    built_now = memo->routed_shadows.build(shadows.routed_keys, shadows.routed_values, shadows.routed_rows, o.routed_shadow, true, w_rows, shadow_query_bytes(), dev);
    (void)hipStreamSynchronize(s);  // (a dropped build's launches have passed before its buffers go)
  }
  if (built_now) ++counters().agg_routed_shadow_builds;
  return Status::OK();
}

}  // namespace dfx
