// dfx_distinct_sets.cpp -- the distinct sets per batch: a set's table and spill list, the control block read one batch behind, growth
// (rehash + spill replay), and consume(), which queues a batch's inserts on its way up to the inner aggregate.
#include "dfx_distinct_impl.hpp"

namespace dfx {

constexpr uint64_t kSetProbes = 256;

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

// a snapshot of the set's control block after an insert: errors, spill replay, growth
Status DistinctAggregateRelation::settle(DistinctSet& S, const uint32_t* hc, bool synced) {
  if (hc[CTRL_ERROR]) return error_from_ctrl(hc[CTRL_ERROR]);
  const uint64_t spilled = (uint64_t)hc[CTRL_SPILL_LO] | ((uint64_t)hc[CTRL_SPILL_HI] << 32);
  const uint64_t occupied = hc[CTRL_OCCUPIED] + (uint64_t)0;
  if (spilled == 0 && occupied <= S.T.load_limit) return Status::OK();
  if (spilled > S.spill.capacity) return Status::Err(DFX_INTERNAL_ERROR, "COUNT_DISTINCT: spill list overflow");
  if (!synced) DFX_HIP(hipStreamSynchronize(ctx().stream));
  return grow(S, occupied, spilled);
}

// ids of n strings for the sets' programs: null where the string is (the source's validity, bit offset and owners ride along)
Status DistinctAggregateRelation::encode_with_validity(DistinctDict& d, const DeviceColumn& src, int64_t n, DeviceColumn* ids_col) {
  DFX_RETURN_IF_ERROR(d.dict.encode(src, n, opt().dict_capacity_log2, ids_col));
  ids_col->null_count = src.null_count;
  ids_col->validity = src.null_count ? src.validity : nullptr;
  ids_col->bit_offset = src.bit_offset;
  ids_col->owners.insert(ids_col->owners.end(), src.owners.begin(), src.owners.end());  // (the validity bitmap)
  return Status::OK();
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
  for (DistinctDict& d : dicts_) DFX_RETURN_IF_ERROR(encode_with_validity(d, b.columns[(size_t)d.src_col], n, &ab.columns[(size_t)d.virt_col]));
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
      DFX_RETURN_IF_ERROR(settle(S, (const uint32_t*)S.snap.get(), false));
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
  }
  return Status::OK();
}

}  // namespace dfx
