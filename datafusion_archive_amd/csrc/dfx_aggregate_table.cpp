// dfx_aggregate_table.cpp -- AggregateRelation: the table and its spill list -- allocation, growth and replay, replacement.
#include "dfx_aggregate_impl.hpp"

namespace dfx {

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
  const int widest = phase != Phase::NotApplicable ? 1 : std::max(1, widest_chunk());  // (the partitioned strategy will run one accumulator per scan: blocks of 8192 slots, 256 partitions)
  Tn->block_mask = (uint32_t)(probe_block_slots(kw, widest, cap) - 1);
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
  spill_owner = device_alloc(sizeof(uint64_t) * (size_t)rows * (size_t)(kw + widest_chunk()), &st);  // (shared by every chunk of accumulators: planes for the widest one)
  if (!spill_owner) return st;
  spill.words = (uint64_t*)spill_owner.get();
  spill.capacity = (uint64_t)rows;
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
  const int new_log2 = grown_table_log2(64 - T.shift, occupied, spilled, replay_from);
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

}  // namespace dfx
