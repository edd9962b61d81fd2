// dfx_aggregate_ctrl.cpp -- AggregateRelation: the control-block pipeline (CtrlPipeline) that checks the launches one batch behind, and the end of everything launched.
#include "dfx_aggregate_impl.hpp"

namespace dfx {

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

// The LAST kernel of the batch about to be launched publishes the control block itself (examined one batch later: post_ctrl), into *snap_to -- this batch's
// slot of the pinned buffer -- or nowhere (null).  (routed_shadow_launch has returned by then when `calibrating`: one condition serves both callers.)
Status AggregateRelation::Impl::arm_snapshot(uint32_t** snap_to) {
  win.snap_armed = false, *snap_to = nullptr;
  if (opt().ctrl_snapshot != 1 || !dec.calibrated || calibrating) return Status::OK();
  if (!ctl.host) DFX_RETURN_IF_ERROR(alloc_ctrl_host());
  if (!win.snap_done) {
    Status st;
    win.snap_done = device_alloc(sizeof(uint32_t) * 16, &st);
    if (!win.snap_done) return st;
    DFX_HIP(hipMemsetAsync(win.snap_done.get(), 0, sizeof(uint32_t) * 16, ctx().stream));
  }
  *snap_to = (uint32_t*)ctl.host.get() + (size_t)(ctl.batch_seq & 1) * CTRL_WORDS;
  win.snap_armed = true;
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
  const uint64_t spilled = ctrl_spilled(hc);
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
  if (needs_rebuild(spilled, hc[CTRL_SATURATED], dec.occupied_known, T.load_limit)) {
    // later batches may already be running against the saturated table: let them finish, then rebuild.  Rows still
    // waiting in the routing regions belong to the blocks of THIS table: aggregate them first.
    DFX_RETURN_IF_ERROR(flush_pass2());
    uint32_t now[CTRL_WORDS];
    DFX_RETURN_IF_ERROR(read_ctrl(now));
    ctl.forget();
    if (now[CTRL_ERROR]) return error_from_ctrl(now[CTRL_ERROR]);
    uint64_t spilled_now = ctrl_spilled(now);
    uint64_t replay_from = 0;
    if (replay_in_place_ok(opt().replay_in_place, spilled_now, now[CTRL_SATURATED], now[CTRL_OCCUPIED], T.load_limit, spill.capacity)) {
      // The table is not full: the rows were spilled by overflowing routing regions (a hot key).  Put them into the
      // table as it is; a row it cannot take is appended to the list BEHIND the rows being replayed (the cursor is not
      // reset), and only those make the table grow.
      hipStream_t s = ctx().stream;
      DFX_HIP(launch_merge_rows(spill, 0, (int64_t)spilled_now, T, spill, s));
      uint32_t after[CTRL_WORDS];
      DFX_RETURN_IF_ERROR(read_ctrl(after));
      if (after[CTRL_ERROR]) return error_from_ctrl(after[CTRL_ERROR]);
      const uint64_t cursor = ctrl_spilled(after);
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
    win.fill_bound = fill_bound_after(win.fill_bound, hc[CTRL_MAX_FILL], ctl.batch_seq, ctl.seq[slot], win.worst);
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

}  // namespace dfx
