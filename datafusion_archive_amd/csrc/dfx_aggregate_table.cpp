// dfx_aggregate_table.cpp -- AggregateRelation: the table, its spill list and routing regions, the launches of one slice of rows,
// the control-block pipeline that checks them one batch behind, growth and replay.
#include "dfx_aggregate_impl.hpp"

namespace dfx {

// ---- table management ------------------------------------------------------------------------------
Status AggregateRelation::Impl::alloc_table(int cap_log2, DevTable* Tn, std::vector<std::shared_ptr<void>>* owners,
                                            bool new_ctrl, uint64_t** full_accs_out) {
  hipStream_t s = ctx().stream;
  memset(Tn, 0, sizeof(*Tn));
  const uint64_t cap = 1ull << cap_log2;
  Tn->stride = cap + 64;
  Tn->mask = cap - 1;
  Tn->shift = 64 - cap_log2;
  Tn->kw = kw;
  Tn->load_limit = cap / 2;
  Tn->max_probe = (int)std::min<uint64_t>(cap, 1u << 30);
  {  // probing block = what one workgroup can hold in 128 KB of LDS (keys + the accumulators of the widest chunk)
    int widest = 1;
    for (const Chunk& ch : chunks) widest = std::max(widest, ch.n);
    if (phase != Phase::NotApplicable) widest = 1;  // (the partitioned strategy will run one accumulator per scan: blocks of 8192 slots, 256 partitions)
    uint64_t blk = 16384 / (uint64_t)(std::max(kw, 1) + widest);  // 128 KB of LDS per block (pass 2: one workgroup per CU)
    uint64_t p2 = 64;
    while (p2 * 2 <= blk) p2 *= 2;
    if (p2 > cap) p2 = cap;
    Tn->block_mask = (uint32_t)(p2 - 1);
  }
  set_algebra(Tn);
  Status st;
  auto keys = device_alloc(sizeof(uint64_t) * Tn->stride * (size_t)std::max(kw, 1), &st);
  if (!keys) return st;
  auto accs = device_alloc(sizeof(uint64_t) * Tn->stride * (size_t)std::max(na_total, 1), &st);  // every chunk's planes
  if (!accs) return st;
  Tn->keys = (uint64_t*)keys.get();
  Tn->accs = (uint64_t*)accs.get();
  owners->clear();
  owners->push_back(keys);
  owners->push_back(accs);
  if (kw > 1) {
    auto slot_state = device_alloc(sizeof(uint32_t) * Tn->stride, &st);
    if (!slot_state) return st;
    Tn->state = (uint32_t*)slot_state.get();
    owners->push_back(slot_state);
    DFX_HIP(hipMemsetAsync(Tn->state, 0, sizeof(uint32_t) * Tn->stride, s));
  } else {
    DFX_HIP(launch_fill_u64(Tn->keys, kEmptyKey, (int64_t)Tn->stride, s));
  }
  for (int a = 0; a < na_total; ++a) DFX_HIP(launch_fill_u64(Tn->accs + (size_t)a * Tn->stride, acc_init_all[a], (int64_t)Tn->stride, s));
  if (full_accs_out) *full_accs_out = Tn->accs;
  Tn->accs += (uint64_t)chunks[(size_t)cur_chunk].a0 * Tn->stride;  // the caller gets the ACTIVE chunk's view
  if (new_ctrl) {
    ctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
    if (!ctrl) return st;
    DFX_HIP(hipMemsetAsync(ctrl.get(), 0, sizeof(uint32_t) * CTRL_WORDS, s));
    stats = device_alloc(sizeof(uint64_t) * kStatStripes * STAT_WORDS, &st);
    if (!stats) return st;
    DFX_HIP(hipMemsetAsync(stats.get(), 0, sizeof(uint64_t) * kStatStripes * STAT_WORDS, s));
  }
  Tn->ctrl = (uint32_t*)ctrl.get();
  Tn->stats = (uint64_t*)stats.get();
  return Status::OK();
}

Status AggregateRelation::Impl::ensure_spill(int64_t rows) {
  if (rows <= 0) {
    return Status::OK();
  }
  if (spill.words && spill.capacity >= (uint64_t)rows) return Status::OK();
  DFX_RETURN_IF_ERROR(settle_ctrl());  // rows spilled by batches still in flight live in the old list
  ScopedUs t_alloc(&counters().agg_alloc_us);
  Status st;
  int widest = na();  // the list is shared by every chunk of accumulators: planes for the widest one
  for (const Chunk& ch : chunks) widest = std::max(widest, ch.n);
  spill_owner = device_alloc(sizeof(uint64_t) * (size_t)rows * (size_t)(kw + widest), &st);
  if (!spill_owner) return st;
  spill.words = (uint64_t*)spill_owner.get();
  spill.capacity = (uint64_t)rows;
  return Status::OK();
}

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
Status AggregateRelation::Impl::flush_pass2() {
  if (win.pending == 0) return Status::OK();
  ++counters().agg_pass2_launches;
  if (win.pending > 1) ++counters().agg_deferred_windows;
  DFX_HIP(launch_partition_agg(T, PT, spill, 0, ctx().stream));
  win.closed();
  win.last_p2_seq = ctl.batch_seq;
  return Status::OK();
}

Status AggregateRelation::Impl::read_ctrl(uint32_t* host_ctrl) {
  ScopedUs t(&counters().agg_sync_us);
  hipStream_t s = ctx().stream;
  DFX_HIP(hipMemcpyAsync(host_ctrl, ctrl.get(), sizeof(uint32_t) * CTRL_WORDS, hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  return Status::OK();
}

// queue an asynchronous snapshot of the control block after the batch just launched.  The copy runs on the side
// stream behind an event, so the next batch's kernels follow this batch's directly (an in-stream D2H copy costs
// ~10 us of idle device per batch: rocprofv3 timeline).  The snapshot may already contain counts of the NEXT batch;
// every word is monotone (errors, occupancy, spill cursor), so that only makes the check earlier.
Status AggregateRelation::Impl::alloc_ctrl_host() {
  Status st;
  ctl.host = pinned_alloc(sizeof(uint32_t) * CTRL_WORDS * 2, &st);
  if (!ctl.host) return st;
  for (int i = 0; i < 2; ++i) {
    DFX_HIP(hipEventCreateWithFlags(&ctl.ev[i], hipEventDisableTiming));
    DFX_HIP(hipEventCreateWithFlags(&ctl.main_ev[i], hipEventDisableTiming));
  }
  return Status::OK();
}

Status AggregateRelation::Impl::post_ctrl(int64_t rows) {
  hipStream_t s = ctx().stream;
  hipStream_t aux = ctx().aux;
  if (!ctl.host) DFX_RETURN_IF_ERROR(alloc_ctrl_host());
  const int slot = (int)(ctl.batch_seq & 1);
  if (win.snap_armed) {
    // the batch's last kernel writes the snapshot into this slot of the pinned buffer: all there is to wait for is the
    // kernel itself.  (The previous occupant of the slot, two batches back, was examined after the previous launch.)
    win.snap_armed = false;
    DFX_HIP(hipEventRecord(ctl.ev[slot], s));
  } else {
    if (ctl.pending[slot]) DFX_RETURN_IF_ERROR(examine_ctrl(slot));
    DFX_HIP(hipEventRecord(ctl.main_ev[slot], s));
    DFX_HIP(hipStreamWaitEvent(aux, ctl.main_ev[slot], 0));
    DFX_HIP(hipMemcpyAsync((uint32_t*)ctl.host.get() + slot * CTRL_WORDS, ctrl.get(), sizeof(uint32_t) * CTRL_WORDS,
                           hipMemcpyDeviceToHost, aux));
    DFX_HIP(hipEventRecord(ctl.ev[slot], aux));
  }
  ctl.pending[slot] = true;
  ctl.rows[slot] = rows;
  ctl.seq[slot] = ctl.batch_seq;
  ctl.unconfirmed_rows += (uint64_t)rows;
  ++ctl.batch_seq;
  return Status::OK();
}

// errors, growth: what the per-batch check has always done, on a (possibly one batch old) snapshot
Status AggregateRelation::Impl::handle_ctrl(const uint32_t* hc, int64_t n) {
  if (hc[CTRL_ERROR]) return error_from_ctrl(hc[CTRL_ERROR]);
  if (dec.narrow && hc[CTRL_WIDE_KEYS] && pair_scan()) pair_wide_seen = true;  // (no wide form fits a block that holds one plane: consume_batch falls back)
  if (dec.narrow && hc[CTRL_WIDE_KEYS] && !pair_scan()) {
    // a key without a 32-bit image turned up (it went to the spill list): 16-byte rows from now on
    DFX_RETURN_IF_ERROR(flush_pass2());
    dec.narrow = false;
    win.layout_valid = false;
    ++counters().agg_narrow_to_wide;
  }
  dec.occupied_known = hc[CTRL_OCCUPIED];
  const uint64_t spilled = ((uint64_t)hc[CTRL_SPILL_HI] << 32) | hc[CTRL_SPILL_LO];
  uint64_t passed_total = 0;
  if (getenv("DFX_DEBUG") && stats) {  // statistics stripes (debug only: one more synchronous copy)
    std::vector<uint64_t> hs((size_t)kStatStripes * STAT_WORDS);
    (void)hipMemcpy(hs.data(), stats.get(), sizeof(uint64_t) * hs.size(), hipMemcpyDeviceToHost);
    for (int i = 0; i < kStatStripes; ++i) passed_total += hs[(size_t)i * STAT_WORDS + STAT_PASSED];
  }
  if (getenv("DFX_DEBUG"))
    fprintf(stderr, "[dfx] batch n=%lld partition=%d lds=%d occupied=%u spilled=%llu saturated=%u passed=%llu cap=%llu "
            "parts=%u cap_rows=%u stage=%u spillcap=%llu\n", (long long)n, (int)dec.use_partition, (int)dec.lds_enabled,
            hc[CTRL_OCCUPIED], (unsigned long long)spilled, hc[CTRL_SATURATED],
            (unsigned long long)passed_total,
            (unsigned long long)(T.mask + 1), PT.n_parts, PT.cap_rows, PT.stage_rows, (unsigned long long)spill.capacity);
  if (spilled > 0 || hc[CTRL_SATURATED] || dec.occupied_known > T.load_limit) {
    // later batches may already be running against the saturated table: let them finish, then rebuild.  Rows still
    // waiting in the routing regions belong to the blocks of THIS table: aggregate them first.
    DFX_RETURN_IF_ERROR(flush_pass2());
    uint32_t now[CTRL_WORDS];
    DFX_RETURN_IF_ERROR(read_ctrl(now));
    ctl.forget();
    if (now[CTRL_ERROR]) return error_from_ctrl(now[CTRL_ERROR]);
    uint64_t spilled_now = ((uint64_t)now[CTRL_SPILL_HI] << 32) | now[CTRL_SPILL_LO];
    uint64_t replay_from = 0;
    if (opt().replay_in_place && spilled_now > 0 && !now[CTRL_SATURATED] && now[CTRL_OCCUPIED] <= T.load_limit &&
        2 * spilled_now <= spill.capacity) {
      // The table is not full: the rows were spilled by overflowing routing regions (a hot key).  Put them into the
      // table as it is; a row it cannot take is appended to the list BEHIND the rows being replayed (the cursor is not
      // reset), and only those make the table grow.
      hipStream_t s = ctx().stream;
      DFX_HIP(launch_merge_rows(spill, 0, (int64_t)spilled_now, T, spill, s));
      uint32_t after[CTRL_WORDS];
      DFX_RETURN_IF_ERROR(read_ctrl(after));
      if (after[CTRL_ERROR]) return error_from_ctrl(after[CTRL_ERROR]);
      const uint64_t cursor = ((uint64_t)after[CTRL_SPILL_HI] << 32) | after[CTRL_SPILL_LO];
      if (cursor == spilled_now && !after[CTRL_SATURATED] && after[CTRL_OCCUPIED] <= T.load_limit) {
        after[CTRL_SPILL_LO] = after[CTRL_SPILL_HI] = 0;
        DFX_HIP(hipMemcpyAsync(ctrl.get(), after, sizeof(uint32_t) * CTRL_WORDS, hipMemcpyHostToDevice, s));
        DFX_HIP(hipStreamSynchronize(s));  // `after` is a stack buffer
        dec.occupied_known = after[CTRL_OCCUPIED];
        ++counters().agg_replays_in_place;
        return Status::OK();
      }
      replay_from = spilled_now;
      spilled_now = cursor;
      memcpy(now, after, sizeof(now));
    }
    DFX_RETURN_IF_ERROR(grow_and_replay(now[CTRL_OCCUPIED], spilled_now, replay_from));
    DFX_RETURN_IF_ERROR(read_ctrl(now));
    dec.occupied_known = now[CTRL_OCCUPIED];
  }
  return Status::OK();
}

Status AggregateRelation::Impl::examine_ctrl(int slot) {
  if (!ctl.pending[slot]) return Status::OK();
  {
    ScopedUs t(&counters().agg_ctrl_wait_us);
    DFX_HIP(hipEventSynchronize(ctl.ev[slot]));
  }
  ctl.pending[slot] = false;
  ctl.unconfirmed_rows -= std::min<uint64_t>(ctl.unconfirmed_rows, (uint64_t)ctl.rows[slot]);
  uint32_t hc[CTRL_WORDS];
  memcpy(hc, (const uint32_t*)ctl.host.get() + slot * CTRL_WORDS, sizeof(hc));
  if (dec.use_partition && ctl.seq[slot] > win.last_p2_seq) {
    // the snapshot was taken after the launch with sequence number ctrl_seq[slot] (it may already show later launches:
    // only larger); every launch since then adds at most pt_worst rows to a region
    const uint64_t later = (uint64_t)std::max<int64_t>(0, ctl.batch_seq - 1 - ctl.seq[slot]);
    win.fill_bound = std::min<uint64_t>(win.fill_bound, (uint64_t)hc[CTRL_MAX_FILL] + later * win.worst);
  }
  return handle_ctrl(hc, ctl.rows[slot]);
}

// everything launched so far has been checked (end of input, or before the spill list is replaced)
Status AggregateRelation::Impl::settle_ctrl() {
  if (!ctl.pending[0] && !ctl.pending[1]) return Status::OK();
  const int older = (int)(ctl.batch_seq & 1);  // the slot the NEXT batch would use holds the older snapshot
  DFX_RETURN_IF_ERROR(examine_ctrl(older));
  DFX_RETURN_IF_ERROR(examine_ctrl(older ^ 1));
  return Status::OK();
}

// The table passed its load limit (or a probe sequence was exhausted): build a table at least 4x
// larger, rehash, then replay the spilled rows into it.  Afterwards occupancy <= 1/4.
Status AggregateRelation::Impl::grow_and_replay(uint64_t occupied, uint64_t spilled, uint64_t replay_from) {
  ++counters().agg_growths;
  hipStream_t s = ctx().stream;
  if (spilled > spill.capacity)
    return Status::Err(DFX_INTERNAL_ERROR, strfmt("group spill list overflow (%llu rows > capacity %llu)",
                                                  (unsigned long long)spilled, (unsigned long long)spill.capacity));
  const int cur_log2 = 64 - T.shift;
  const int need_log2 = ceil_log2(4 * (occupied + (spilled - replay_from) + 1));
  const int new_log2 = std::max(cur_log2 + 2, need_log2);
  if (new_log2 > 31) return Status::Err(DFX_EXECUTION_ERROR, "GROUP BY table would exceed 2^31 slots");
  DevTable Tn;
  std::vector<std::shared_ptr<void>> owners;
  uint64_t* accs_full_new = nullptr;
  DFX_RETURN_IF_ERROR(alloc_table(new_log2, &Tn, &owners, false, &accs_full_new));
  // reset the shared control words that describe the (new) table
  uint32_t host_ctrl[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(read_ctrl(host_ctrl));
  host_ctrl[CTRL_OCCUPIED] = 0;
  host_ctrl[CTRL_SPILL_LO] = host_ctrl[CTRL_SPILL_HI] = 0;
  host_ctrl[CTRL_SENTINEL] = 0;
  host_ctrl[CTRL_SATURATED] = 0;  // (rehash re-raises the sentinel word when it meets the sentinel slot)
  const DevRows no_spill = no_spill_rows();
  // `from` still needs the old CTRL_SENTINEL to know whether slot `cap` is occupied: give the old
  // table a private copy of the control block for the duration of the rehash
  Status st;
  auto old_ctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
  if (!old_ctrl) return st;
  DFX_HIP(hipMemcpyAsync(old_ctrl.get(), ctrl.get(), sizeof(uint32_t) * CTRL_WORDS, hipMemcpyDeviceToDevice, s));
  DFX_HIP(hipMemcpyAsync(ctrl.get(), host_ctrl, sizeof(uint32_t) * CTRL_WORDS, hipMemcpyHostToDevice, s));
  DFX_HIP(hipStreamSynchronize(s));  // host_ctrl is a stack buffer
  win.layout_valid = false;  // the routing regions are per table block
  DevTable Told = T;
  Told.ctrl = (uint32_t*)old_ctrl.get();
  DFX_HIP(launch_rehash(Told, Tn, no_spill, s));
  for (int c = 0; c < (int)chunks.size(); ++c) {  // the other chunks' planes move the same way (their keys are already in place)
    if (c == cur_chunk) continue;
    DFX_HIP(launch_rehash(view_of(Told, accs_full, c), view_of(Tn, accs_full_new, c), no_spill, s));
  }
  if (spilled > replay_from) DFX_HIP(launch_merge_rows(spill, (int64_t)replay_from, (int64_t)(spilled - replay_from), Tn, no_spill, s));
  replace_table(Tn, accs_full_new, owners, false);  // old buffers return to the pool once the stream has passed them
  DFX_HIP(hipStreamSynchronize(s));
  return Status::OK();
}

// The table is replaced (growth, import).  A key column copied ahead of time (agg.early_keys) was made from the OLD table's slot
// order and its side-stream kernels may still read the old planes: drop the copy (its buffers stay alive until they have run) and
// make any later validity check fail.  forget_snapshot: also forget the previous snapshot's group count, so that the next copy waits
// for two equal counts of the new table (the in-library exchange asks for it; growth and partial_import never did).
void AggregateRelation::Impl::replace_table(const DevTable& Tn, uint64_t* accs_full_new, const std::vector<std::shared_ptr<void>>& owners, bool forget_snapshot) {
  early.cancel();
  ++table_generation;
  if (forget_snapshot) early_last_occupied = ~0ull;
  T = Tn;
  accs_full = accs_full_new;
  table_owners = owners;
}

// everything launched so far is aggregated and checked: the pending pass 2, the snapshots in flight and -- read_back -- the
// control block as it is now (what ran after the last snapshot: errors, spilled rows, growth)
Status AggregateRelation::Impl::finish_launched(int64_t rows, bool read_back) {
  DFX_RETURN_IF_ERROR(flush_pass2());
  DFX_RETURN_IF_ERROR(settle_ctrl());
  if (!read_back) return Status::OK();
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(read_ctrl(hc));
  return handle_ctrl(hc, rows);
}

// The device side of a column shadow's build (dfx_key_shadow.hpp, dfx_value_shadow.hpp) on stream s: `launch` is the streaming
// kernel that writes the 4-byte copy and ORs its verdict into one device word; build_us: the counter the attempt's wall time goes to.
typedef hipError_t (*ShadowLaunch)(const uint64_t* in, int64_t n, uint32_t* out, uint32_t* verdict, hipStream_t s);
static KeyShadowDevice shadow_device(hipStream_t s, ShadowLaunch launch, long long* build_us) {
  KeyShadowDevice dev;
  dev.free_bytes = []() -> size_t {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return free_b;
  };
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
  int widest = na();
  for (const Chunk& ch : chunks) widest = std::max(widest, ch.n);
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
  const bool first = !key_shadow_asked;
  key_shadow_asked = true;
  bool built = false;
  const uint32_t* words = memo->key_shadows.acquire(cols.c[ks].values, o.key_shadow, first, shadow_query_bytes(), dev, &built);
  if (built) ++counters().agg_key_shadow_builds, shadow_built_here = true;
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
  const bool first = !value_shadow_asked;
  value_shadow_asked = true;
  bool built = false;
  const uint32_t* words = memo->value_shadows.acquire(cols.c[vc].values, o.value_shadow, first, shadow_query_bytes(), dev, &built);
  if (built) ++counters().agg_value_shadow_builds, shadow_built_here = true;
  *operand_col = vc;
  return words;
}

// prog, cols: the batch as the operator bound it (before row0).  The layout the launch would be sized by stands in for the
// launch's flags: the kernels' conditions look at the shape (PTF_WS, PTF_NARROW ...), not at the regions.
bool AggregateRelation::Impl::both_shadows_bind(const DevProgram& prog, const DevFastPlan& fp, const DevColumns& cols, int64_t rows, int64_t row0) {
  if (opt().routed_row8 == 0 || shadow_built_here || calibrating || !input) return false;
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

// the launch's DevPartition over a window's regions
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
  win.snap_armed = false;
  if (opt().ctrl_snapshot == 1 && dec.calibrated) {
    if (!ctl.host) DFX_RETURN_IF_ERROR(alloc_ctrl_host());
    if (!win.snap_done) {
      Status st;
      win.snap_done = device_alloc(sizeof(uint32_t) * 16, &st);
      if (!win.snap_done) return st;
      DFX_HIP(hipMemsetAsync(win.snap_done.get(), 0, sizeof(uint32_t) * 16, s));
    }
    pt.snap_host = (uint32_t*)ctl.host.get() + (size_t)(ctl.batch_seq & 1) * CTRL_WORDS;
    pt.snap_done = (uint32_t*)win.snap_done.get();
    win.snap_armed = true;
  }
  DFX_HIP(launch_partition_scan(T, pt, spill, pred, 8.0 * (double)n, s));
  win.last_p2_seq = ctl.batch_seq;
  ++counters().agg_routed_shadow_launches;
  ++routed_shadow_launches;
  *took = true;
  return Status::OK();
}

// After the query's last batch.  The build is the existing dense wave-specialised pass 1 over both column shadows (the SigKeySum
// kernels of the key4 unit: SELECT k, SUM(v) GROUP BY k, every row routed), window by window into that window's own regions, in
// launches of agg.partition_split_rows rows with PTF_RESUME; no pass 2.  It runs against a control block of its own and no spill
// list: a row that finds no place in a region is counted there and nowhere else, and the count refuses the shadow for good.
Status AggregateRelation::Impl::routed_shadow_maybe() {
  const AggOptions& o = opt();
  if (o.routed_shadow == 0 || !routed_keys || !input || !dec.use_partition || !dec.narrow || kw != 1 || na() != 1 || chunks.size() != 1) return Status::OK();
  if (T.acc_kind[0] != ACC_ADD_F64 || T.val_xform[0] != VT_RAW || o.routed_row8 == 0) return Status::OK();
  ScanMemo* memo = input->column_memo();
  if (!memo || memo->routed_shadows.state_of(routed_keys, routed_values) > 0) return Status::OK();  // (built or refused already)
  const uint32_t* key_words = memo->key_shadows.peek(routed_keys);
  const uint32_t* value_words = memo->value_shadows.peek(routed_values);
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
  dev.free_bytes = []() -> size_t {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return free_b;
  };
  dev.alloc = [](size_t bytes) { return device_alloc_optional(bytes); };
  dev.layout = [this](int64_t rows) -> RoutedWindowLayout {
    RoutedLayoutQuery q = layout_query(rows, false, true);
    q.has_pred = false, q.unfused_now = false, q.dense_seen = true, q.mostly_seen = true, q.skew_seen = false;  // every row is routed
    const RoutedLayout L = choose_routed_layout(q);
    RoutedWindowLayout l;
    if (L.kind != RoutedLayoutKind::ring16 || !(L.PT.flags & PTF_ROW8) || !partition_launchable(L.PT)) return l;
    RoutedGeometry& g = l.g;
    g.n_parts = L.PT.n_parts, g.n_producers = L.PT.n_producers, g.cap_rows = L.PT.cap_rows, g.n_words = L.PT.n_words, g.part_shift = L.PT.part_shift;
    g.flags = L.PT.flags, g.part_stride = L.PT.part_stride, g.prod_stride = L.PT.prod_stride, g.win_stride = L.PT.win_stride;
    g.shift = T.shift, g.block_slots = T.block_mask + 1;
    l.region_bytes = L.row_bytes, l.count_bytes = L.cnt_bytes;
    ws_scanners_of_build = L.PT.ws_scanners;
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
      pt.ws_scanners = ws_scanners_of_build;
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
    *spilled = ((uint64_t)hc[CTRL_SPILL_HI] << 32) | hc[CTRL_SPILL_LO];
    *error = hc[CTRL_ERROR];
    return true;
  };
  int64_t w_rows = (int64_t)o.routed_shadow_window_rows & ~(int64_t)63;
  if (w_rows < 64) w_rows = kRoutedWindowRows;
  bool built_now = false;
  {
    ScopedUs t_build(&counters().agg_routed_shadow_build_us);
    built_now = memo->routed_shadows.build(routed_keys, routed_values, routed_rows, o.routed_shadow, true, w_rows, shadow_query_bytes(), dev);
    (void)hipStreamSynchronize(s);  // (a dropped build's launches have passed before its buffers go)
  }
  if (built_now) ++counters().agg_routed_shadow_builds;
  return Status::OK();
}

Status AggregateRelation::Impl::launch_rows(const DeviceBatch& b, const DevProgram& prog_in, const DevColumns& cols_in,
                                            int64_t row0, int64_t n) {
  hipStream_t s = ctx().stream;
  win.snap_armed = false;
  DevProgram prog = prog_in;
  DevColumns cols = cols_in;
  double bytes = 0;
  for (int i = 0; i < prog.n_cols; ++i) {  // advance the bound columns to row0 (row0 is a multiple of 64)
    const int w = prog.col_dtype[i] == T_BOOL ? 0 : dtype_width(prog.col_dtype[i]);
    if (w) cols.c[i].values = (const uint8_t*)cols.c[i].values + (size_t)row0 * w;
    else cols.c[i].bit_offset += row0;
    if (cols.c[i].validity && w) cols.c[i].bit_offset += row0;
    bytes += (double)n * (w ? w : 0.125);
  }
  DevAggPlan p = active().plan;
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
  if (partition_now) {
    const DevFastPlan fpp = fast_plan();
    DevPartition pt = PT;
    pt.flags &= ~PTF_ROW8;  // (the shadows first: the form is put back below once both are bound)
    if (win.pending > 0) pt.flags |= PTF_RESUME;
    // the key column's Int32 shadow, bound in place of the column for this launch: 12 bytes per row.  Everything behind the
    // hash image -- routed rows, pass 2, the table, the result's Int64 key column -- is what it was
    if (const uint32_t* key_words = key_shadow_words(prog_in, fpp, cols_in, pt)) {
      const int ks = fpp.keycol[0];
      cols.c[ks].values = key_words + row0;
      prog.col_dtype[ks] = T_U32;
      pt.flags |= PTF_KEY4;
      bytes -= 4.0 * (double)n;
      ++counters().agg_key_shadow_launches;
      ++key_shadow_launches;
      // ... and the operand's Float32 shadow beside it, where every value of the column is exactly its float: 8 bytes per row.
      // The scanners widen it back to the column's own bits; predicate, routed rows and everything behind them are what they were
      int vc = 0;
      if (const uint32_t* value_words = value_shadow_words(prog, fpp, cols_in, pt, &vc)) {
        cols.c[vc].values = value_words + row0;
        prog.col_dtype[vc] = T_F32;
        pt.flags |= PTF_VAL4;
        bytes -= 4.0 * (double)n;
        ++counters().agg_value_shadow_launches;
        ++value_shadow_launches;
        if (!routed_keys) {  // (the pair a routed shadow would be of: routed_shadow_maybe, after the last batch)
          int64_t at = 0;
          if (!routed_pair(prog_in, fpp, cols_in, &routed_keys, &routed_values, &routed_rows, &at)) routed_keys = nullptr;
        }
      }
    }
    if (PT.flags & PTF_ROW8) {
      if (pt.flags & PTF_VAL4) {
        pt.flags |= PTF_ROW8;
        ++counters().agg_row8_launches;
        ++row8_launches;
      } else {
        // a shadow that was there a moment ago did not bind after all (memory, a slice off the 64-row grid): 8-byte regions never
        // meet such a launch -- close the window, lay the regions out for 12-byte rows
        DFX_RETURN_IF_ERROR(ensure_partition(layout_rows, prog.has_nulls != 0, false));
        const uint32_t keep = pt.flags & (PTF_KEY4 | PTF_VAL4);
        pt = PT;
        pt.flags |= keep;  // (nothing is pending after the flush: no PTF_RESUME)
      }
    }
    // close the window when one more batch could overflow a region (or the batch budget is used up; the calibration
    // slice is aggregated at once: the strategy decision reads the group count)
    const int max_batches = pair_scan() ? std::min(2, std::max(1, opt().partition_defer_batches)) : std::max(1, opt().partition_defer_batches);  // (pair scan: the spill list's sizing)
    const bool close_window = calibrating || win.pending + 1 >= max_batches || win.fill_bound + 2 * (uint64_t)win.worst > PT.cap_rows;
    // the LAST kernel of this batch publishes the control block itself (examined one batch later, see post_ctrl)
    win.snap_armed = false;
    uint32_t* snap_to = nullptr;
    if (opt().ctrl_snapshot == 1 && dec.calibrated && !calibrating) {
      if (!ctl.host) DFX_RETURN_IF_ERROR(alloc_ctrl_host());
      if (!win.snap_done) {
        Status st;
        win.snap_done = device_alloc(sizeof(uint32_t) * 16, &st);
        if (!win.snap_done) return st;
        DFX_HIP(hipMemsetAsync(win.snap_done.get(), 0, sizeof(uint32_t) * 16, s));
      }
      snap_to = (uint32_t*)ctl.host.get() + (size_t)(ctl.batch_seq & 1) * CTRL_WORDS;
      win.snap_armed = true;
    }
    if (!close_window) {
      pt.snap_host = snap_to;
      pt.snap_done = (uint32_t*)win.snap_done.get();
    }
    DFX_HIP(launch_partition(prog, fpp, cols, p, T, pt, spill, n, bytes, s));
    if (pt.flags & PTF_SHARED) ++counters().agg_shared_operand_launches;
    if (pt.flags & PTF_PAIR) ++counters().agg_pair_launches;
    if (pt.flags & PTF_PLANES) ++counters().agg_plane_launches;
    if (pt.flags & PTF_HOT) ++counters().agg_hot_key_launches;
    ++win.pending;
    win.fill_bound += win.worst;
    win.rows_in_flight += n;
    if (close_window) {
      PT.snap_host = snap_to;
      PT.snap_done = (uint32_t*)win.snap_done.get();
      Status fst = flush_pass2();
      PT.snap_host = nullptr;
      PT.snap_done = nullptr;
      DFX_RETURN_IF_ERROR(fst);
    }
    return Status::OK();
  }
  const DevFastPlan fp = fast_plan();
  // a handful of groups (the calibration slice / earlier batches saw <= 8): register accumulators.  Should more
  // groups turn up later the kernel still handles them (through the table), and the next batch goes back to K7.
  if (dec.lds_enabled && dec.calibrated && !calibrating && opt().strategy != 1 && opt().fewgroup &&
      dec.occupied_known > 0 && dec.occupied_known <= 8 && fewgroup_supported(prog, fp, T)) {
    DFX_HIP(launch_fewgroup_agg(prog, fp, cols, p, T, spill, n, bytes, s));
    ++counters().agg_fewgroup_launches;
    return Status::OK();
  }
  if (dec.lds_enabled && opt().strategy != 1) {
    const AggOptions& o = opt();
    int slots = o.lds_slots >= 0 ? o.lds_slots : 4096;
    if (calibrating && o.lds_slots < 0) slots = 512;  // calibration slice: the cache only has to tell few groups from many
    while (slots > 64 && (size_t)slots * ((size_t)(kw + na()) * 8 + (kw > 1 ? 4 : 0)) > 64 * 1024) slots >>= 1;
    int copies = o.lds_copies > 0 ? o.lds_copies : 1;
    if (o.lds_copies <= 0 && dec.calibrated) {  // few groups: lane-replicated sub-tables
      if (dec.occupied_known <= 16) copies = 16;
      else if (dec.occupied_known <= 128) copies = 4;
    }
    while (copies > 1 && slots / copies < 64) copies >>= 1;
    p.lds_slots = slots;
    p.lds_copies = copies;
  } else {
    p.lds_slots = 0;
    p.lds_copies = 1;
  }
  DFX_HIP(launch_hash_agg(prog, fp, cols, p, T, spill, n, bytes, s));
  return Status::OK();
}

}  // namespace dfx
