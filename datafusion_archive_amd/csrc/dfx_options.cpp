// dfx_options.cpp -- the library-level C ABI: init, device info, synchronise; the option keys of dfx_set_option and of every
// operator's own option set; the counters; the profiling and debug hooks.  Options and counters are looked up in two tables that
// name every field of their struct: a field that is not in its table does not compile.
#include <string.h>

#include "dfx_relation.hpp"

using namespace dfx;

namespace {

struct OptionKey {
  const char* key;
  int AggOptions::*field;
};
constexpr OptionKey kOptionKeys[] = {
    {"agg.strategy",                  &AggOptions::strategy},
    {"agg.capacity_log2",             &AggOptions::capacity_log2},
    {"agg.lds_slots",                 &AggOptions::lds_slots},
    {"agg.lds_copies",                &AggOptions::lds_copies},
    {"scan.fast",                     &AggOptions::fast},
    {"scan.plan",                     &AggOptions::plan},
    {"agg.partition_mode",            &AggOptions::partition_mode},
    {"agg.partition_block",           &AggOptions::partition_block},
    {"agg.fewgroup",                  &AggOptions::fewgroup},
    {"agg.replay_in_place",           &AggOptions::replay_in_place},
    {"agg.partition_pad",             &AggOptions::partition_pad},
    {"agg.dict_capacity_log2",        &AggOptions::dict_capacity_log2},
    {"agg.distinct_capacity_log2",    &AggOptions::distinct_capacity_log2},
    {"agg.partition_cap_rows",        &AggOptions::partition_cap_rows},
    {"agg.partition_defer",           &AggOptions::partition_defer},
    {"agg.partition_defer_batches",   &AggOptions::partition_defer_batches},
    {"agg.partition_split_rows",      &AggOptions::partition_split_rows},
    {"agg.pass2_stream",              &AggOptions::pass2_stream},
    {"agg.calibration_memo",          &AggOptions::calibration_memo},
    {"agg.emit_async",                &AggOptions::emit_async},
    {"agg.early_keys",                &AggOptions::early_keys},
    {"agg.hot_keys",                  &AggOptions::hot_keys},
    {"agg.partition_layout",          &AggOptions::partition_layout},
    {"agg.narrow_keys",               &AggOptions::narrow_keys},
    {"agg.key_shadow",                &AggOptions::key_shadow},
    {"agg.value_shadow",              &AggOptions::value_shadow},
    {"agg.routed_row8",               &AggOptions::routed_row8},
    {"agg.routed_shadow",             &AggOptions::routed_shadow},
    {"agg.routed_shadow_window_rows", &AggOptions::routed_shadow_window_rows},
    {"agg.narrow_chunk16",            &AggOptions::narrow_chunk16},
    {"agg.shared_operand",            &AggOptions::shared_operand},
    {"agg.ctrl_snapshot",             &AggOptions::ctrl_snapshot},
    {"export.kernel_copy",            &AggOptions::export_kernel_copy},
    {"agg.partition_producers",       &AggOptions::partition_producers},
    {"agg.pass1_ws",                  &AggOptions::pass1_ws},
    {"agg.pass1_ws_dense",            &AggOptions::pass1_ws_dense},
    {"agg.pass1_ws_dense_scanners",   &AggOptions::pass1_ws_dense_scanners},
    {"agg.merge_scan_batches",        &AggOptions::merge_scan_batches},
    {"filter.single_pass",            &AggOptions::filter_single_pass},
    {"filter.dense",                  &AggOptions::filter_dense},
    {"agg.split_aggregates",          &AggOptions::split_aggregates},
    {"agg.chunk_hold",                &AggOptions::chunk_hold},
    {"agg.pair_scan",                 &AggOptions::pair_scan},
    {"agg.shared_planes",             &AggOptions::shared_planes},
    {"csv.wave_tiles",                &AggOptions::csv_wave_tiles},
    {"host.stream",                   &AggOptions::host_stream},
    {"host.stage_threads",            &AggOptions::host_stage_threads},
    {"host.stage_mb",                 &AggOptions::host_stage_mb},
    {"host.stage_slots",              &AggOptions::host_stage_slots},
};
static_assert(sizeof(kOptionKeys) / sizeof(kOptionKeys[0]) == sizeof(AggOptions) / sizeof(int),
              "every field of AggOptions has its key in kOptionKeys (and nothing else is in the struct)");

struct CounterName {
  const char* name;
  long long Counters::*field;
};
constexpr CounterName kCounterNames[] = {
    {"h2d_bytes",                           &Counters::h2d_bytes},
    {"h2d_staged_bytes",                    &Counters::h2d_staged_bytes},
    {"filter_output_regrows",               &Counters::filter_output_regrows},
    {"filter_lookback_fallbacks",           &Counters::filter_lookback_fallbacks},
    {"csv_cells",                           &Counters::csv_cells},
    {"export_host_ready",                   &Counters::export_host_ready},
    {"agg_early_keys",                      &Counters::agg_early_keys},
    {"agg_early_keys_used",                 &Counters::agg_early_keys_used},
    {"agg_emit_reused_early",               &Counters::agg_emit_reused_early},
    {"agg_early_keys_late",                 &Counters::agg_early_keys_late},
    {"csv_tiles",                           &Counters::csv_tiles},
    {"csv_general_tiles",                   &Counters::csv_general_tiles},
    {"csv_write_cells",                     &Counters::csv_write_cells},
    {"csv_write_bytes",                     &Counters::csv_write_bytes},
    {"csv_write_general_tiles",             &Counters::csv_write_general_tiles},
    {"agg_ctrl_wait_us",                    &Counters::agg_ctrl_wait_us},
    {"agg_sync_us",                         &Counters::agg_sync_us},
    {"agg_emit_us",                         &Counters::agg_emit_us},
    {"agg_drain_us",                        &Counters::agg_drain_us},
    {"agg_alloc_us",                        &Counters::agg_alloc_us},
    {"agg_pass2_launches",                  &Counters::agg_pass2_launches},
    {"agg_pair_launches",                   &Counters::agg_pair_launches},
    {"agg_plane_launches",                  &Counters::agg_plane_launches},
    {"agg_key_shadow_builds",               &Counters::agg_key_shadow_builds},
    {"agg_key_shadow_launches",             &Counters::agg_key_shadow_launches},
    {"agg_key_shadow_build_us",             &Counters::agg_key_shadow_build_us},
    {"agg_value_shadow_builds",             &Counters::agg_value_shadow_builds},
    {"agg_value_shadow_launches",           &Counters::agg_value_shadow_launches},
    {"agg_value_shadow_build_us",           &Counters::agg_value_shadow_build_us},
    {"agg_row8_launches",                   &Counters::agg_row8_launches},
    {"agg_routed_shadow_builds",            &Counters::agg_routed_shadow_builds},
    {"agg_routed_shadow_launches",          &Counters::agg_routed_shadow_launches},
    {"agg_routed_shadow_build_us",          &Counters::agg_routed_shadow_build_us},
    {"agg_pair_fallbacks",                  &Counters::agg_pair_fallbacks},
    {"agg_growths",                         &Counters::agg_growths},
    {"agg_shared_operand_launches",         &Counters::agg_shared_operand_launches},
    {"agg_calibrations",                    &Counters::agg_calibrations},
    {"agg_memo_decisions",                  &Counters::agg_memo_decisions},
    {"agg_calibration_replays",             &Counters::agg_calibration_replays},
    {"agg_replays_in_place",                &Counters::agg_replays_in_place},
    {"agg_narrow_to_wide",                  &Counters::agg_narrow_to_wide},
    {"agg_fewgroup_launches",               &Counters::agg_fewgroup_launches},
    {"agg_hot_key_launches",                &Counters::agg_hot_key_launches},
    {"agg_unfused_batches",                 &Counters::agg_unfused_batches},
    {"agg_held_runs",                       &Counters::agg_held_runs},
    {"agg_pair_fallbacks_pending",          &Counters::agg_pair_fallbacks_pending},
    {"agg_deferred_windows",                &Counters::agg_deferred_windows},
    {"distinct_set_growths",                &Counters::distinct_set_growths},
    {"distinct_spill_rows",                 &Counters::distinct_spill_rows},
    {"distinct_inserted",                   &Counters::distinct_inserted},
    {"sort_passes_run",                     &Counters::sort_passes_run},
    {"sort_passes_skipped",                 &Counters::sort_passes_skipped},
    {"sort_topk_selects",                   &Counters::sort_topk_selects},
    {"parquet_chunk_bytes",                 &Counters::parquet_chunk_bytes},
    {"parquet_pages",                       &Counters::parquet_pages},
    {"parquet_dict_pages",                  &Counters::parquet_dict_pages},
    {"parquet_plain_pages",                 &Counters::parquet_plain_pages},
    {"parquet_rle_runs",                    &Counters::parquet_rle_runs},
    {"parquet_bitpacked_runs",              &Counters::parquet_bitpacked_runs},
    {"parquet_host_walked_strings",         &Counters::parquet_host_walked_strings},
    {"parquet_inflated_pages",              &Counters::parquet_inflated_pages},
    {"parquet_stored_pages",                &Counters::parquet_stored_pages},
    {"parquet_inflated_bytes",              &Counters::parquet_inflated_bytes},
    {"parquet_lz4_sequences",               &Counters::parquet_lz4_sequences},
    {"parquet_inflated_bytes_to_host",      &Counters::parquet_inflated_bytes_to_host},
    {"parquet_write_pages",                 &Counters::parquet_write_pages},
    {"parquet_write_bytes",                 &Counters::parquet_write_bytes},
    {"parquet_write_rle_level_pages",       &Counters::parquet_write_rle_level_pages},
    {"parquet_write_bitpacked_level_pages", &Counters::parquet_write_bitpacked_level_pages},
    {"parquet_write_row_groups",            &Counters::parquet_write_row_groups},
    {"parquet_write_dict_pages",            &Counters::parquet_write_dict_pages},
    {"parquet_write_dict_entries",          &Counters::parquet_write_dict_entries},
    {"parquet_write_dict_index_pages",      &Counters::parquet_write_dict_index_pages},
    {"parquet_write_dict_rle_index_pages",  &Counters::parquet_write_dict_rle_index_pages},
    {"parquet_write_dict_fallback_chunks",  &Counters::parquet_write_dict_fallback_chunks},
    {"parquet_write_lz4_pages",             &Counters::parquet_write_lz4_pages},
    {"parquet_write_lz4_bytes_in",          &Counters::parquet_write_lz4_bytes_in},
    {"parquet_write_lz4_bytes_out",         &Counters::parquet_write_lz4_bytes_out},
    {"parquet_write_lz4_sequences",         &Counters::parquet_write_lz4_sequences},
    {"xchg_calls",                          &Counters::xchg_calls},
    {"xchg_local_us",                       &Counters::xchg_local_us},
    {"xchg_wait_peers_us",                  &Counters::xchg_wait_peers_us},
    {"xchg_exchange_us",                    &Counters::xchg_exchange_us},
    {"xchg_rounds",                         &Counters::xchg_rounds},
    {"xchg_host_syncs",                     &Counters::xchg_host_syncs},
    {"export_us",                           &Counters::export_us},
    {"export_alloc_us",                     &Counters::export_alloc_us},
};
static_assert(sizeof(kCounterNames) / sizeof(kCounterNames[0]) == sizeof(Counters) / sizeof(long long),
              "every field of Counters has its name in kCounterNames (and nothing else is in the struct)");

}  // namespace

namespace dfx {
bool set_option_in(AggOptions& o, const char* key, int64_t value) {
  if (!key) return false;
  for (const OptionKey& k : kOptionKeys)
    if (!strcmp(key, k.key)) {
      o.*k.field = (int)value;
      return true;
    }
  return false;
}
}  // namespace dfx

extern "C" {

int32_t dfx_init(int32_t device_ordinal, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    Context& c = ctx();
    if (c.initialised && c.device != device_ordinal)
      return to_c(Status::Err(DFX_GENERAL, "dfx_init: the library is already bound to another device"), err, errlen);
    c.device = device_ordinal;
    return to_c(ensure_init(), err, errlen);
  });
}

int32_t dfx_device_info(char* name, size_t namelen, int32_t* n_cu, int64_t* hbm_bytes, int32_t* wavefront, char* err,
                        size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    Status st = ensure_init();
    if (!st.ok()) return to_c(st, err, errlen);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, ctx().device);
    if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, hipGetErrorString(e)), err, errlen);
    if (name && namelen) snprintf(name, namelen, "%s (%s)", prop.name, prop.gcnArchName);
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (wavefront) *wavefront = prop.warpSize;
    return DFX_OK;
  });
}

int32_t dfx_synchronize(char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    Status st = ensure_init();
    if (!st.ok()) return to_c(st, err, errlen);
    hipError_t e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, hipGetErrorString(e)), err, errlen);
    return DFX_OK;
  });
}

// ---- measurement hooks ---------------------------------------------------------------------------
int32_t dfx_profile_enable(int32_t on) {
  profile_enable(on != 0);
  return DFX_OK;
}
int32_t dfx_profile_reset(void) {
  profile_reset();
  return DFX_OK;
}
int32_t dfx_profile_count(void) { return profile_count(); }
int32_t dfx_profile_get(int32_t index, char* name, size_t namelen, int64_t* launches, double* total_ms, double* algo_bytes) {
  const char* nm = nullptr;
  int64_t l = 0;
  double ms = 0, b = 0;
  if (!profile_get(index, &nm, &l, &ms, &b)) return DFX_GENERAL;
  if (name && namelen) snprintf(name, namelen, "%s", nm);
  if (launches) *launches = l;
  if (total_ms) *total_ms = ms;
  if (algo_bytes) *algo_bytes = b;
  return DFX_OK;
}

uint64_t dfx_debug_group_hash(uint64_t key) { return host_hash_keys(&key, 1); }
uint32_t dfx_debug_unhash32(uint32_t image) { return host_unhash_word32(image); }

int64_t dfx_counter_get(const char* name) {
  if (!name) return -1;
  for (const CounterName& c : kCounterNames)
    if (!strcmp(name, c.name)) return counters().*c.field;
  return -1;
}
void dfx_counter_reset(void) { counters() = Counters(); }

int32_t dfx_set_option(const char* key, int64_t value) {
  if (!key) return DFX_GENERAL;
  if (!strcmp(key, "pool.trim")) {
    pool_trim();
    return DFX_OK;
  }
  if (!strcmp(key, "pool.inject_oom")) {  // test hook: the next `value` device allocations that miss the pool fail their first attempt
    pool_inject_oom((int)value);
    return DFX_OK;
  }
  if (!strcmp(key, "test.exchange_fail")) {  // test hook: rank << 8 | stage fails locally at that stage of dfx_aggregate_exchange (0: off)
    set_exchange_test_failure(value);
    return DFX_OK;
  }
  return set_option_in(agg_options(), key, value) ? DFX_OK : DFX_GENERAL;
}

}  // extern "C"
