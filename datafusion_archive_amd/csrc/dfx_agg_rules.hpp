// dfx_agg_rules.hpp -- the grouped aggregate's numeric rules: how large a probing block, a grown table, a pass-2 window, the LDS
// front cache and the spill list are.  Plain arithmetic on what the operator knows, free of HIP, like dfx_pass1_layout.hpp: the
// translation units of the operator (dfx_aggregate_*.cpp) call these and keep no copy; tests/native/agg_rules_check.cpp holds each
// against a table written out by hand, as a stand-alone program under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace dfx {

inline int ceil_log2(uint64_t v) {
  int l = 0;
  while ((1ull << l) < v && l < 62) ++l;
  return l;
}

// alloc_table: the probing block = what one workgroup can hold in 128 KB of LDS (kw key words + the accumulators of the widest
// chunk per slot; pass 2 runs one workgroup per CU), a power of two from 64 slots up, at most the table
inline uint64_t probe_block_slots(int kw, int widest, uint64_t cap) {
  const uint64_t blk = 16384 / (uint64_t)(std::max(kw, 1) + widest);
  uint64_t p2 = 64;
  while (p2 * 2 <= blk) p2 *= 2;
  return std::min(p2, cap);
}

// grow_and_replay: at least 4x larger, and occupancy <= 1/4 once the rows still to be replayed are in.  (The caller refuses > 31.)
inline int grown_table_log2(int cur_log2, uint64_t occupied, uint64_t spilled, uint64_t replay_from) {
  return std::max(cur_log2 + 2, ceil_log2(4 * (occupied + (spilled - replay_from) + 1)));
}

// handle_ctrl: the table cannot go on as it is -- rows were spilled, a probe sequence was exhausted, the load limit is passed
inline bool needs_rebuild(uint64_t spilled, uint32_t saturated, uint64_t occupied, uint64_t load_limit) {
  return spilled > 0 || saturated || occupied > load_limit;
}

// ... but it is not full: the rows were spilled by overflowing routing regions (a hot key), and the list has room for them to be
// appended behind themselves once more.  They are put into the table as it is
inline bool replay_in_place_ok(int replay_in_place_opt, uint64_t spilled, uint32_t saturated, uint64_t occupied, uint64_t load_limit,
                               uint64_t spill_capacity) {
  return replay_in_place_opt && spilled > 0 && !saturated && occupied <= load_limit && 2 * spilled <= spill_capacity;
}

// examine_ctrl: the snapshot was taken after launch snap_seq (it may already show later launches: only larger); every launch since
// then adds at most `worst` rows to a region.  (A snapshot older than the last pass 2 says nothing: the caller passes no update.)
inline uint64_t fill_bound_after(uint64_t fill_bound, uint32_t max_fill, int64_t batch_seq, int64_t snap_seq, uint32_t worst) {
  const uint64_t later = (uint64_t)std::max<int64_t>(0, batch_seq - 1 - snap_seq);
  return std::min<uint64_t>(fill_bound, (uint64_t)max_fill + later * worst);
}

// batches a pass-2 window holds at most (agg.partition_defer_batches; pair scan: two, the spill list's sizing)
inline int window_max_batches(int defer_batches_opt, bool pair_scan) {
  return pair_scan ? std::min(2, std::max(1, defer_batches_opt)) : std::max(1, defer_batches_opt);
}

// launch_rows: close the window when one more batch could overflow a region, or the batch budget is used up; the calibration slice is
// aggregated at once (the strategy decision reads the group count)
inline bool window_must_close(bool calibrating, int pending, int defer_batches_opt, bool pair_scan, uint64_t fill_bound, uint32_t worst,
                              uint32_t cap_rows) {
  return calibrating || pending + 1 >= window_max_batches(defer_batches_opt, pair_scan) || fill_bound + 2 * (uint64_t)worst > cap_rows;
}

// launch_rows: the LDS front cache of the hash-aggregate kernel.  4096 slots (the calibration slice: 512, it only has to tell few
// groups from many), halved until they fit 64 KB; few groups: lane-replicated sub-tables of at least 64 slots each
struct FrontCacheShape {
  int slots, copies;
};
inline FrontCacheShape front_cache_shape(int lds_slots_opt, int lds_copies_opt, bool calibrating, bool calibrated, uint64_t occupied_known,
                                         int kw, int na) {
  int slots = lds_slots_opt >= 0 ? lds_slots_opt : 4096;
  if (calibrating && lds_slots_opt < 0) slots = 512;
  while (slots > 64 && (uint64_t)slots * ((uint64_t)(kw + na) * 8 + (kw > 1 ? 4 : 0)) > 64 * 1024) slots >>= 1;
  int copies = lds_copies_opt > 0 ? lds_copies_opt : 1;
  if (lds_copies_opt <= 0 && calibrated) {
    if (occupied_known <= 16) copies = 16;
    else if (occupied_known <= 128) copies = 4;
  }
  while (copies > 1 && slots / copies < 64) copies >>= 1;
  return {slots, copies};
}

// consume_batch_chunk: rows that a deferred pass 2 may still spill -- every row of the window (pair scan: once per OPERAND, by the
// last plane of each; planes of a shared operand: once)
inline int64_t spill_window_rows(bool use_partition, bool pair_scan, bool split_is_shared, int defer_batches_opt, int64_t n, int64_t layout_rows) {
  if (!use_partition) return 0;
  return (int64_t)window_max_batches(defer_batches_opt, pair_scan) * (pair_scan && !split_is_shared ? 2 : 1) * std::max(n, layout_rows);
}

}  // namespace dfx
