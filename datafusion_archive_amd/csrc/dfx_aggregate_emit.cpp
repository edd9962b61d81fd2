// dfx_aggregate_emit.cpp -- AggregateRelation: the key column copied ahead of time, and the result batch.
#include "dfx_aggregate_impl.hpp"

namespace dfx {

Status AggregateRelation::Impl::emit_ungrouped(DeviceBatch* out) {  // aggregate.rs:745-784
  uint64_t hs[2 * kMaxAccsTotal];
  memset(hs, 0, sizeof(hs));
  for (int c = 0; c < (int)chunks.size(); ++c) {  // every chunk keeps its own (has-value, bits) pairs
    DFX_HIP(hipMemcpy(hs + 2 * chunks[(size_t)c].a0, chunks[(size_t)c].state.get(), sizeof(uint64_t) * 2 * (size_t)chunks[(size_t)c].n, hipMemcpyDeviceToHost));
  }
  out->num_rows = 1;
  out->columns.clear();
  out->columns.resize(outs.size());
  for (size_t j = 0; j < outs.size(); ++j) {
    const int a = outs[j].acc;
    DeviceColumn& c = out->columns[j];
    c.dtype = outs[j].avg ? outs[j].dtype : out_dtype[a];
    c.length = 1;
    uint64_t bits = hs[2 * a + 1];
    bool has_value = hs[2 * a] != 0;
    if (outs[j].avg) {  // SUM / COUNT (deviation D7); None when nothing was counted
      const uint64_t cntv = hs[2 * (a + 1)] ? hs[2 * (a + 1) + 1] : 0;
      has_value = has_value && cntv != 0;
      bits = has_value ? host_avg_value((uint8_t)outs[j].dtype, bits, cntv) : 0;
    }
    uint8_t raw[8];
    memcpy(raw, &bits, 8);  // little endian: the low bytes are the narrow value
    std::shared_ptr<void> dv, dn;
    DFX_RETURN_IF_ERROR(upload_small(raw, 8, &dv));
    c.values = dv.get();
    c.owners.push_back(dv);
    const bool has = has_value;
    uint8_t vb[8] = {(uint8_t)(has ? 1 : 0), 0, 0, 0, 0, 0, 0, 0};
    DFX_RETURN_IF_ERROR(upload_small(vb, 8, &dn));
    c.validity = (const uint8_t*)dn.get();
    c.null_count = has ? 0 : 1;
    if (!has) c.null_count = 1;
    else c.validity = nullptr;
    c.owners.push_back(dn);
  }
  return Status::OK();
}

// Queues the key column's compaction and download on the side stream when the group count has stopped changing (see EarlyKeys).
Status AggregateRelation::Impl::early_keys_maybe() {
  const uint64_t prev = early_last_occupied;
  early_last_occupied = dec.occupied_known;
  if (early.armed && early.generation == table_generation && early.occupied == dec.occupied_known) return Status::OK();  // still good
  if (!opt().early_keys || !opt().emit_async || !dec.use_partition || kw != 1 || kw_out != 1 || !dicts.empty() || chunks.size() != 1)
    return Status::OK();
  if (dec.occupied_known < 32768 || dec.occupied_known != prev) return Status::OK();  // small results are not worth it; still growing
  early.cancel();
  hipStream_t aux = ctx().aux;
  Status st;
  const int64_t g = (int64_t)dec.occupied_known;
  const int64_t n_slots = (int64_t)T.mask + 2;
  const int64_t n_words = (n_slots + 63) / 64;
  const int64_t n_tiles = (n_slots + kTileRows - 1) / kTileRows;
  const int dt = key_dtype[0];
  // Speculative work: a buffer that cannot be had (memory pressure, the tests' allocation-failure injection) drops the
  // attempt -- the query itself does not need it and must not fail because of it.
  auto mask = device_alloc(sizeof(uint64_t) * (size_t)n_words, &st);
  auto counts = mask ? device_alloc(sizeof(uint32_t) * (size_t)n_tiles, &st) : nullptr;
  auto offsets = counts ? device_alloc(sizeof(uint64_t) * (size_t)(n_tiles + 1), &st) : nullptr;
  auto tmp = offsets ? device_alloc(sizeof(uint64_t) * (size_t)(n_tiles / 4096 + 4), &st) : nullptr;
  auto vals = tmp ? device_alloc((size_t)g * dtype_width(dt), &st) : nullptr;
  early.bytes = (size_t)g * dtype_width(dt);
  if (vals) early.host = pinned_alloc(early.bytes, &st);
  if (vals && early.host && !early.total) early.total = pinned_alloc(sizeof(uint64_t), &st);
  std::shared_ptr<void> dense;  // 4-byte keys: the compacted 8-byte key words before narrowing
  if (vals && dtype_width(dt) != 8) dense = device_alloc(sizeof(uint64_t) * (size_t)g, &st);
  if (!vals || !early.host || !early.total || (dtype_width(dt) != 8 && !dense)) {
    early.host.reset();
    return Status::OK();
  }
  *(uint64_t*)early.total.get() = ~0ull;
  if (!early.done) DFX_HIP(hipEventCreateWithFlags(&early.done, hipEventDisableTiming));
  if (!early.start) DFX_HIP(hipEventCreateWithFlags(&early.start, hipEventDisableTiming));
  early.scratch = {mask, counts, offsets, tmp, vals};
  if (dense) early.scratch.push_back(dense);
  early.keep = table_owners;  // (the side stream reads the key plane: it stays allocated until that has happened, whatever replaces the table)
  early.keep.push_back(ctrl);
  // The side stream starts behind everything queued on the main stream so far: the pool hands out blocks whose previous users may
  // still be queued there.  It is not ordered against what comes LATER: whatever those kernels add to the table makes the final
  // group count differ from `g`, and the copy is dropped.
  DFX_HIP(hipEventRecord(early.start, ctx().stream));
  DFX_HIP(hipStreamWaitEvent(aux, early.start, 0));
  DFX_HIP(launch_table_mask(T, (uint64_t*)mask.get(), (uint32_t*)counts.get(), aux));
  DFX_HIP(launch_scan_u32((const uint32_t*)counts.get(), (uint64_t*)offsets.get(), n_tiles, (uint64_t*)tmp.get(), aux));
  DFX_HIP(hipMemcpyAsync(early.total.get(), (uint64_t*)offsets.get() + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, aux));
  DFX_HIP(launch_fill_u64(T.keys + T.mask + 1, kEmptyKey, 1, aux));  // (as emit_grouped: the sentinel group's key word; always this constant)
  if (dtype_width(dt) == 8) {
    DFX_HIP(launch_compact(T.keys, 8, (const uint64_t*)mask.get(), (const uint64_t*)offsets.get(), n_slots, vals.get(), 0, aux, (uint64_t)g));
  } else {
    DFX_HIP(launch_compact(T.keys, 8, (const uint64_t*)mask.get(), (const uint64_t*)offsets.get(), n_slots, dense.get(), 0, aux, (uint64_t)g));
    DFX_HIP(launch_finalize((const uint64_t*)dense.get(), g, (uint8_t)dt, (uint8_t)VT_RAW, vals.get(), aux));
  }
  // by the copy engine, not by a kernel: pass 1's workgroups take a CU's whole register file, so a copy kernel's waves and a pass-1
  // workgroup cannot share a CU -- measured: the kernel copy made the pass-1 launches it met 0.2 ms longer, more than it saved
  DFX_HIP(hipMemcpyAsync(early.host.get(), vals.get(), early.bytes, hipMemcpyDeviceToHost, aux));
  DFX_HIP(hipEventRecord(early.done, aux));
  early.armed = true;
  early.occupied = dec.occupied_known;
  early.generation = table_generation;
  ++counters().agg_early_keys;
  return Status::OK();
}

Status AggregateRelation::Impl::emit_grouped(DeviceBatch* out, int64_t expected) {  // aggregate.rs:877-951
  ScopedUs t_emit(&counters().agg_emit_us);
  hipStream_t s = ctx().stream;
  const int64_t n_slots = (int64_t)T.mask + 2;
  const int64_t n_words = (n_slots + 63) / 64;
  const int64_t n_tiles = (n_slots + kTileRows - 1) / kTileRows;
  Status st;
  if (!emit_total) {
    emit_total = pinned_alloc(sizeof(uint64_t), &st);
    if (!emit_total) return st;
  }
  uint64_t* total = (uint64_t*)emit_total.get();
  // Round 6: when the key column was copied ahead of time (agg.early_keys) and is still valid -- the same table, the group count it
  // was made for, its own scan's total equal to it: groups are never removed, so the occupancy mask it compacted with IS the
  // table's -- that mask, its tile offsets and the compacted key column on the device are what emit would compute again: reuse
  // them (three kernels and their boundaries less behind the query's last pass 2: ~0.1 ms of a 4 ms step).
  std::shared_ptr<void> mask, counts, offsets, tmp, early_keys_dev;
  bool reuse_early = false;
  if (expected >= 0 && early.armed && early.generation == table_generation && early.occupied == (uint64_t)expected &&
      early.scratch.size() >= 5 && kw_out == 1 && dicts.empty()) {
    // (its kernels and copies ran on the side stream while the scan went on: long finished -- unless the copy engine stalled)
    if (early.ready() && *(const uint64_t*)early.total.get() == (uint64_t)expected && early.bytes == (size_t)expected * dtype_width(key_dtype[0])) {
      mask = early.scratch[0];
      offsets = early.scratch[2];
      early_keys_dev = early.scratch[4];
      reuse_early = true;
      *total = (uint64_t)expected;
      ++counters().agg_emit_reused_early;
    }
  }
  if (!reuse_early) {
    mask = device_alloc(sizeof(uint64_t) * (size_t)n_words, &st);
    if (!mask) return st;
    counts = device_alloc(sizeof(uint32_t) * (size_t)n_tiles, &st);
    if (!counts) return st;
    offsets = device_alloc(sizeof(uint64_t) * (size_t)(n_tiles + 1), &st);
    if (!offsets) return st;
    tmp = device_alloc(sizeof(uint64_t) * (size_t)(n_tiles / 4096 + 4), &st);
    if (!tmp) return st;
    DFX_HIP(launch_table_mask(T, (uint64_t*)mask.get(), (uint32_t*)counts.get(), s));
    DFX_HIP(launch_scan_u32((const uint32_t*)counts.get(), (uint64_t*)offsets.get(), n_tiles, (uint64_t*)tmp.get(), s));
    // The group count is already on the host (CTRL_OCCUPIED of the last control-block check), so the compaction kernels
    // are queued without waiting for the scan's total; the total comes back with the final synchronisation and must
    // agree.  `expected < 0`: second attempt after a disagreement, with the scan's own count (one extra round trip).
    *total = ~0ull;
    DFX_HIP(hipMemcpyAsync(total, (uint64_t*)offsets.get() + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (expected < 0) DFX_HIP(hipStreamSynchronize(s));
  }
  const int64_t g = expected < 0 ? (int64_t)*total : expected;
  out->num_rows = g;
  out->columns.clear();
  out->columns.resize((size_t)kw_out + outs.size());
  auto dense = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(g, 1), &st);
  if (!dense) return st;
  // the sentinel group's key word is not stored in the table: patch slot `cap` before compaction
  if (kw == 1 && !reuse_early) DFX_HIP(launch_fill_u64(T.keys + T.mask + 1, kEmptyKey, 1, s));
  for (int k = 0; k < kw_out; ++k) {  // (padding words beyond kw_out are constants: not part of the result)
    const uint64_t* plane = T.keys + (size_t)k * T.stride;
    const int dt = key_dtype[k];
    DeviceColumn& c = out->columns[k];
    c.dtype = dt;
    c.length = g;
    if (reuse_early) {  // (one key column, no dictionary: the side stream compacted -- and narrowed -- it already)
      c.values = early_keys_dev.get();
      c.owners.push_back(early_keys_dev);
      continue;
    }
    const DictKey* dk = nullptr;
    for (const DictKey& d : dicts)
      if (d.key == k) dk = &d;
    if (dk || dtype_width(dt) != 8)
      DFX_HIP(launch_compact(plane, 8, (const uint64_t*)mask.get(), (const uint64_t*)offsets.get(), n_slots, dense.get(), 0, s, (uint64_t)g));
    if (dk) {  // ids -> Arrow Utf8
      DFX_RETURN_IF_ERROR(dk->dict.to_utf8((const uint64_t*)dense.get(), g, nullptr, 0, "Utf8 group keys", &c));
      continue;
    }
    auto vals = device_alloc((size_t)std::max<int64_t>(g, 1) * dtype_width(dt), &st);
    if (!vals) return st;
    if (dtype_width(dt) == 8) {  // the plane's words ARE the column: compact straight into it (one kernel and 16 bytes per group less)
      DFX_HIP(launch_compact(plane, 8, (const uint64_t*)mask.get(), (const uint64_t*)offsets.get(), n_slots, vals.get(), 0, s, (uint64_t)g));
    } else {
      DFX_HIP(launch_finalize((const uint64_t*)dense.get(), g, (uint8_t)dt, (uint8_t)VT_RAW, vals.get(), s));
    }
    c.values = vals.get();
    c.owners.push_back(vals);
  }
  for (size_t j = 0; j < outs.size(); ++j) {
    const int a = outs[j].acc;
    const int dt = outs[j].avg ? outs[j].dtype : out_dtype[a];
    DeviceColumn& c = out->columns[(size_t)kw_out + j];
    c.dtype = dt;
    c.length = g;
    auto vals = device_alloc((size_t)std::max<int64_t>(g, 1) * dtype_width(dt), &st);
    if (!vals) return st;
    const bool raw8 = !outs[j].avg && dtype_width(dt) == 8 && (val_xform_all[a] == VT_RAW || val_xform_all[a] == VT_COUNT_VALID);  // SUM(f64 / i64), COUNT: no image to undo
    DFX_HIP(launch_compact(accs_full + (size_t)a * T.stride, 8, (const uint64_t*)mask.get(), (const uint64_t*)offsets.get(), n_slots,
                           raw8 ? vals.get() : dense.get(), 0, s, (uint64_t)g));
    if (raw8) {
    } else if (!outs[j].avg) {
      DFX_HIP(launch_finalize((const uint64_t*)dense.get(), g, (uint8_t)dt, val_xform_all[a], vals.get(), s));
    } else {  // SUM plane / COUNT plane (deviation D7); groups that counted nothing are null
      auto dense_cnt = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(g, 1), &st);
      if (!dense_cnt) return st;
      auto valid = device_alloc(sizeof(uint64_t) * (size_t)((g + 63) / 64 + 1), &st);
      if (!valid) return st;
      auto nulls = device_alloc(sizeof(uint64_t), &st);
      if (!nulls) return st;
      DFX_HIP(hipMemsetAsync(nulls.get(), 0, sizeof(uint64_t), s));
      DFX_HIP(launch_compact(accs_full + (size_t)(a + 1) * T.stride, 8, (const uint64_t*)mask.get(), (const uint64_t*)offsets.get(),
                             n_slots, dense_cnt.get(), 0, s, (uint64_t)g));
      DFX_HIP(launch_finalize_avg((const uint64_t*)dense.get(), (const uint64_t*)dense_cnt.get(), g, (uint8_t)dt, vals.get(),
                                  (uint64_t*)valid.get(), (uint64_t*)nulls.get(), s));
      uint64_t n_null = 0;
      DFX_HIP(hipMemcpyAsync(&n_null, nulls.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
      DFX_HIP(hipStreamSynchronize(s));
      if (n_null) {
        c.validity = (const uint8_t*)valid.get();
        c.null_count = (int64_t)n_null;
        c.owners.push_back(valid);
      }
    }
    c.values = vals.get();
    c.owners.push_back(vals);
  }
  DFX_HIP(hipStreamSynchronize(s));
  if ((int64_t)*total != g) {
    if (expected < 0) return Status::Err(DFX_INTERNAL_ERROR, "group count changed during emit");
    return emit_grouped(out, -1);  // the host's count was stale: redo with the table's own
  }
  if (early.armed) {  // the key column copied ahead of time: valid iff it was made from this table with this many groups -- and has arrived
    DeviceColumn& kc = out->columns[0];
    if (!early.ready()) {
      ++counters().agg_early_keys_late;
    } else if (early.generation == table_generation && early.occupied == (uint64_t)g && *(const uint64_t*)early.total.get() == (uint64_t)g &&
        early.bytes == (size_t)g * dtype_width(kc.dtype) && kc.values != nullptr) {
      kc.host_values = early.host;
      kc.host_values_of = kc.values;
      kc.host_bytes = early.bytes;
      ++counters().agg_early_keys_used;
    }
    early.drop();
  }
  return Status::OK();
}

}  // namespace dfx
