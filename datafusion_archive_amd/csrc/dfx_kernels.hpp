// dfx_kernels.hpp -- host-callable launchers of the gfx950 kernels (implemented in dfx_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "dfx_device.hpp"
#include "dfx_parquet_lz4.hpp"
#include "dfx_parquet_rle.hpp"
#include "dfx_scan_rules.hpp"
#include "dfx_utf8_match.hpp"

namespace dfx {

constexpr int kTileRows = 4096;  // one compaction tile = 64 bitmap words
constexpr int kBlock = 256;

// kernel ids for the built-in profiler
enum KernelId : int {
  KID_PREDICATE_MASK = 0,
  KID_COMPACT,
  KID_PROJECT,
  KID_REDUCE,
  KID_HASH_AGG,
  KID_MERGE_ROWS,
  KID_REHASH,
  KID_EMIT_MASK,
  KID_FINALIZE,
  KID_SCAN,
  KID_SYNTH,
  KID_FILL,
  KID_GATHER_UTF8,
  KID_PARTIAL,
  KID_PARTITION,
  KID_PARTITION_AGG,
  KID_CSV,
  KID_SORT,
  KID_DISTINCT_INSERT,
  KID_DISTINCT_COUNT,
  KID_UTF8_PRED,
  KID_UTF8_EXTREMA,
  KID_CSV_WRITE,
  KID_PARQUET,
  KID_PARQUET_INFLATE,
  KID_PARQUET_WRITE,
  KID_PARQUET_WRITE_LZ4,
  KID_COUNT_
};
const char* kernel_name(int kid);

// ---- profiler (HIP events around tracked launches, on the launch stream) --------------------
void profile_enable(bool on);
void profile_reset();
int profile_count();
bool profile_get(int index, const char** name, int64_t* launches, double* total_ms, double* algo_bytes);

int device_cu_count();

// ---- scan plans (DevScanPlan, dfx_device.hpp; built in dfx_scan_plan.hpp) -----------------------------------------------
// Shape check at operator-creation time (no batch needed): <= 4 columns of 4 / 8-byte numeric types, a conjunction of
// `column <op> literal` terms, plain-column keys, plain-column arguments.
bool scan_plan_shape_ok(const DevProgram& P, const DevFastPlan& F, int kw, int na, const uint8_t* val_xform);
// Per launch: the plan-order column binding (Cout) and the plan itself (Fout->scan) for the bound batch.  fixed: one key in
// slot 0 and the (first) argument in slot 1 (PlanPolicy1).  False: the shape or this batch's buffers are not covered.
// key4_slots: the caller has slot look-up kernels for "the key in slot 0 is the only 4-byte column" (DevScanPlan::gen bit 2).
bool bind_scan_plan(const DevProgram& P, const DevFastPlan& F, const DevColumns& C, int kw, int na, const uint8_t* val_xform,
                    bool fixed, DevFastPlan* Fout, DevColumns* Cout, bool key4_slots = false);

// K1 predicate_mask: fused compare/AND/OR expression -> Arrow LSB bitmap (one __ballot per 64 rows)
//   replaces comparison_ops!/boolean_ops!/literal_array! closures (expression.rs:171-243, :410-465)
// tile_counts (may be null): popcount per 4096-row tile, for the compaction offsets.
// fast: shape-specialised plan (valid == 0 or nulls present: the generic interpreter runs)
hipError_t launch_mask_and_count(uint64_t* mask, const uint64_t* other, uint32_t* tile_counts, int64_t n, hipStream_t s);
hipError_t launch_predicate_mask(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, uint8_t pred,
                                 int64_t n, uint64_t* mask_words, uint32_t* tile_counts, uint32_t* ctrl,
                                 double algo_bytes, hipStream_t s);

// K1 + K4 in ONE pass (single-pass FilterRelation, filter.rs:46-110): evaluates the predicate, writes the Arrow bitmap
// words, the per-tile exclusive offsets (decoupled look-back over the tiles' kept counts: what launch_scan_u32 of the tile
// counts would give, tile_offsets[n_tiles] = kept rows) and compacts up to kFusedOutCols of the predicate's own columns
// from the values already in registers.  sync: filter_fused_sync_words(n) words, zeroed before the launch; sync[1] = kept.
size_t filter_fused_sync_words(int64_t n);
hipError_t launch_filter_fused(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, uint8_t pred, int64_t n,
                               uint64_t* mask_words, uint64_t* tile_offsets, uint64_t* sync, const DevFusedOut& O,
                               uint32_t* ctrl, double algo_bytes, hipStream_t s);

// exclusive scan of uint32 counts into uint64 offsets (out[n] = total); tmp: >= (n/4096 + 2) u64; afterwards tmp[scan_blocks(n)]
// (dfx_scan_rules.hpp) holds the 64-bit grand total
hipError_t launch_scan_u32(const uint32_t* in, uint64_t* out, int64_t n, uint64_t* tmp, hipStream_t s);
// exclusive scan of int32 lengths into int32 offsets (out[n] = total); tmp as above
hipError_t launch_scan_i32(const int32_t* in, int32_t* out, int64_t n, uint64_t* tmp, hipStream_t s);

// K4 compact: order-preserving stream compaction of one fixed-width column by bitmap
//   replaces fn filter (filter.rs:79-110).  width in {1,2,4,8} bytes.
hipError_t launch_compact(const void* in, int width, const uint64_t* mask_words,
                          const uint64_t* tile_offsets, int64_t n, void* out, double algo_bytes,
                          hipStream_t s, uint64_t out_limit = ~0ull);
// Utf8 support for K4: lengths from offsets, byte gather
hipError_t launch_utf8_lengths(const int32_t* offsets, int64_t n, int32_t* lengths, int32_t* starts, hipStream_t s);
hipError_t launch_utf8_gather(const uint8_t* data, const int32_t* src_starts, const int32_t* dst_offsets,
                              int64_t m, uint8_t* out, hipStream_t s);

// K2/K3 project: fused arithmetic / cast expression outputs (typed values + validity bitmaps)
//   replaces math_ops!/cast_column! closures (expression.rs:131-169, :246-280, :466-493)
hipError_t launch_project(const DevProgram& P, const DevColumns& C, const DevProjectPlan& plan,
                          int64_t n, uint32_t* ctrl, double algo_bytes, hipStream_t s);

// K5 reduce_all: ungrouped aggregates of one batch into per-aggregate batch partials, then the
// scalar fold (accumulate_scalar) into the running state.
//   replaces array_min/max/sum + without_group_by (aggregate.rs:344-546, :703-785)
// partial: na * 4 u64 words {acc, valid_count, first_valid_tag, unused}; state: na * 2 words {has, bits}
hipError_t launch_reduce(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevAggPlan& plan,
                         const DevTable& T /* kinds / xforms / inits only */, int64_t n,
                         uint64_t* partial, uint32_t* ctrl, double algo_bytes, hipStream_t s);
hipError_t launch_reduce_fold(const DevTable& T, const uint8_t* arg_dtype, const uint8_t* func,
                              uint64_t* partial, uint64_t* state, uint32_t* ctrl, hipStream_t s);

// K6/K7 hash_agg: (optional predicate) + group keys + aggregate arguments -> table updates, with
// an LDS front cache per workgroup and a spill list for rows the table cannot take.
//   replaces with_group_by + update_accumulators (aggregate.rs:787-875, :548-612)
hipError_t launch_hash_agg(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C,
                           const DevAggPlan& plan, const DevTable& T, const DevRows& spill, int64_t n,
                           double algo_bytes, hipStream_t s);
// K7 for a handful of groups (dfx_k_fewgroup.hip): per-lane register accumulators against a wave-uniform key
// dictionary; same table / spill contract as launch_hash_agg.  fewgroup_supported: fast plan, no nulls,
// <= 2 key words, <= 4 aggregates.
bool fewgroup_supported(const DevProgram& P, const DevFastPlan& fast, const DevTable& T);
hipError_t launch_fewgroup_agg(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C,
                               const DevAggPlan& plan, const DevTable& T, const DevRows& spill, int64_t n,
                               double algo_bytes, hipStream_t s);
// insert pre-evaluated rows (spill replays, LDS flushes of other ranks, all-to-all imports)
hipError_t launch_merge_rows(const DevRows& rows, int64_t row_begin, int64_t n_rows, const DevTable& T,
                             const DevRows& spill, hipStream_t s);
hipError_t launch_rehash(const DevTable& from, const DevTable& to, const DevRows& spill, hipStream_t s);
hipError_t launch_fill_u64(uint64_t* p, uint64_t v, int64_t n, hipStream_t s);
// the low halves of n 8-byte keys (in: 16-byte aligned) as 4-byte words (out: 8-byte aligned); the OR of the dropped halves is ORed into *dropped
hipError_t launch_narrow_keys(const uint64_t* in, int64_t n, uint32_t* out, uint32_t* dropped, hipStream_t s);
// n Float64 values (in: 16-byte aligned) as Float32 (out: 8-byte aligned); *inexact is ORed with 1 when some value is not exactly
// its float (dfx_value_shadow.hpp: other bits after widening back, a NaN, a Float32 denormal)
hipError_t launch_narrow_values(const uint64_t* in, int64_t n, uint32_t* out, uint32_t* inexact, hipStream_t s);
// device -> host-mapped pinned memory by a kernel on `s` (falls back to hipMemcpyAsync for unaligned pointers)
hipError_t launch_copy_to_host(const void* src_device, void* dst_pinned, size_t bytes, hipStream_t s);
hipError_t launch_fill_u32(uint32_t* p, uint32_t v, int64_t n, hipStream_t s);

// K8 emit_groups: occupancy bitmap of the table (then launch_scan_u32 + launch_compact on each
// plane), and the typed finalisation of one output column.
//   replaces the result macros (aggregate.rs:633-699, :877-951)
hipError_t launch_table_mask(const DevTable& T, uint64_t* mask_words, uint32_t* tile_counts, hipStream_t s);
// in: dense u64 plane; out: typed column. is_key: narrow only. xform/kind/func describe the agg.
hipError_t launch_finalize(const uint64_t* in, int64_t n, uint8_t out_dtype, uint8_t val_xform,
                           void* out, hipStream_t s);
// AVG columns: sum / count in the argument's type, validity bitmap (count == 0 -> null), null count
hipError_t launch_finalize_avg(const uint64_t* sum, const uint64_t* cnt, int64_t n, uint8_t out_dtype, void* out,
                               uint64_t* validity, uint64_t* null_count, hipStream_t s);
uint64_t host_avg_value(uint8_t t, uint64_t sum, uint64_t cnt);

// multi-GPU partial export: count per destination rank, then scatter into bucketed planes
hipError_t launch_partial_count(const DevTable& T, int world, uint64_t* counts, hipStream_t s);
hipError_t launch_partial_scatter(const DevTable& T, int world, const uint64_t* bucket_base,
                                  const uint64_t* bucket_count, uint64_t* cursors, uint64_t* dst,
                                  hipStream_t s);
// merge bucketed planes (layout of dfx_aggregate_partial_export) into a table
hipError_t launch_merge_bucket(const uint64_t* bucket, uint64_t count, const DevTable& T,
                               const DevRows& spill, hipStream_t s);

// Utf8 GROUP BY keys (dfx_k_dict.hip): strings -> stable 64-bit ids and back
hipError_t launch_dict_encode(const int32_t* offsets, const uint8_t* data, int64_t n, const DevDict& D, uint64_t n_known, uint64_t* ids,
                              hipStream_t s);  // n_known: ids the dictionary already holds (complete: written by earlier launches)
hipError_t launch_dict_rebuild(const DevDict& D, uint64_t n_ids, hipStream_t s);
hipError_t launch_dict_remap_plane(uint64_t* plane, uint64_t n_slots, const uint64_t* remap, uint64_t n_ids, hipStream_t s);
hipError_t launch_dict_lengths(const uint64_t* ids, int64_t g, const DevDict& D, uint32_t* lens, hipStream_t s);
hipError_t launch_dict_gather(const uint64_t* ids, int64_t g, const DevDict& D, const uint64_t* starts, int32_t* offsets,
                              uint8_t* out, hipStream_t s);

// Utf8 string terms (dfx_k_utf8pred.hip, deviation D9): one compiled term (dfx_utf8_match.hpp) over one Utf8 column -> Arrow LSB
// bitmap, (n + 63) / 64 whole words (bits past n are zero).  T.lit: DEVICE buffer of utf8_term_image_bytes(T.t) bytes (dfx_utf8_match.hpp:
// the literal bytes, padded to 4, then the segment table).  validity may be null.  Every load stays inside the bytes the batch
// references, data + [offsets[0], offsets[n]).
struct DevUtf8Pred {
  Utf8Term t;
  const uint8_t* lit;
};
hipError_t launch_utf8_pred(const int32_t* offsets, const uint8_t* data, const uint8_t* validity, int64_t bit_offset, int64_t n,
                            const DevUtf8Pred& T, uint64_t* mask_words, double algo_bytes, hipStream_t s);
// popcount per 4096-row tile of a finished bitmap (the compaction offsets of a filter whose mask is one term's bitmap)
hipError_t launch_mask_tile_counts(const uint64_t* mask_words, uint32_t* tile_counts, int64_t n, hipStream_t s);

// partitioned GROUP BY (dfx_k_partition.hip, pass 2: dfx_k_pass2.hip): pass 1 routes passing rows to per-(producer, partition)
// regions, pass 2 aggregates every partition in an LDS copy of its table block.  Single-word keys.  (The LDS bytes of pass 1 and the
// routed layout a table takes: dfx_pass1_layout.hpp.)
bool partition_planes_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T);  // PTF_PLANES: ... the one-value kernels with the raw operand
bool partition_pair_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T);  // PTF_PAIR: this bound batch fits the pair kernels
bool partition_key_shadow_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T, const DevPartition& PT);  // PTF_KEY4: a pass-1 kernel reads this batch's key from its Int32 shadow
// PTF_VAL4: ... and the operand from its Float32 shadow.  P, PT: the launch with the key shadow already bound (key T_U32, PTF_KEY4)
// one window of a routed shadow through pass 2's scan form (dfx_k_pass2.hip; dfx_routed_shadow.hpp)
hipError_t launch_partition_scan(const DevTable& T, const DevPartition& PT, const DevRows& spill, const DevRowPred& pred, double algo_bytes, hipStream_t s);
bool partition_value_shadow_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T, const DevPartition& PT, int* operand_col);
hipError_t launch_probe_wide_keys(const DevTable& T, hipStream_t s);
hipError_t launch_partition(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevAggPlan& plan,
                            const DevTable& T, const DevPartition& PT, const DevRows& spill, int64_t n,
                            double algo_bytes, hipStream_t s);
hipError_t launch_partition_agg(const DevTable& T, const DevPartition& PT, const DevRows& spill, double algo_bytes,
                                hipStream_t s);

// CSV text -> Arrow columns (dfx_k_csv.hip): record boundaries by parallel simulation of the csv automaton, then one
// thread per record converts the cells.  buf must be readable up to the next multiple of 32 bytes past n.
//   boundaries_count: tile_trans / tile_state / tile_counts have one entry per csv_tile_bytes() of text;
//   (scan tile_counts into tile_offsets, total = number of records) then boundaries_write fills row_start[0..total).
int64_t csv_tile_bytes();
hipError_t launch_csv_boundaries_count(const uint8_t* buf, uint64_t n, uint32_t* tile_trans, uint32_t* block_vec, uint8_t* tile_state,
                                       uint32_t* tile_counts, hipStream_t s);
hipError_t launch_csv_boundaries_write(const uint8_t* buf, uint64_t n, const uint32_t* tile_trans, const uint8_t* tile_state,
                                       const uint64_t* tile_offsets, uint64_t* row_start, hipStream_t s);
hipError_t launch_csv_count_fields(const uint8_t* buf, const uint64_t* row_start, int64_t row, uint32_t* out,
                                   hipStream_t s);
hipError_t launch_csv_parse(const uint8_t* buf, const uint64_t* row_start, int64_t r0, int64_t nb,
                            const DevCsvPlan& plan, double avg_record_bytes, int wave_tiles, double algo_bytes, hipStream_t s);
hipError_t launch_csv_utf8_gather(const uint8_t* buf, const uint64_t* row_start, int64_t r0, int64_t nb, int field,
                                  const int32_t* offsets, const uint64_t* starts, uint8_t* out, hipStream_t s);

// Parquet column chunk -> Arrow column (dfx_k_parquet.hip, deviation D12).  One column chunk of one row group: `chunk` is the
// chunk's bytes on the device, `pages` its host-validated page table (dfx_parquet_rle.hpp: every extent inside the chunk).
struct DevPqColumn {
  const uint8_t* chunk;
  const PqPage* pages;
  uint32_t n_pages;
  uint32_t rows;      // of the row group
  uint32_t optional;  // 1: definition levels -> validity
  uint32_t dtype;     // the Arrow type stored (dfx_datatype)
  uint32_t width;     // bytes of a stored PLAIN value (4 / 8; 0: Boolean, Utf8)
  uint32_t dict_off, dict_n;  // the dictionary's PLAIN values (fixed width: dict_n * width bytes inside the chunk)
  const uint32_t* dict_str;   // Utf8: offsets of the dictionary's length prefixes, dict_n + 1
  const uint32_t* str_offs;   // Utf8: the same for PLAIN data pages (PqPage::str_base, PqPage::pad entries + 1 per page)
  uint64_t* validity;      // optional: (rows + 63) / 64 + 1 words, zeroed
  uint64_t* dense_bits;    // RLE Boolean pages: (sum of num_values + 63) / 64 + 1 words, zeroed
  uint32_t* dense_idx;     // dictionary pages: sum of num_values entries
  uint32_t* word_rank;     // optional: WalkedChunk::rank_total entries
  uint32_t* page_nonnull;  // n_pages
  uint32_t* page_decoded;  // n_pages
  uint32_t* ctrl;          // CTRL_WORDS words: PQ_ERR_* bits are ORed into CTRL_ERROR
  uint64_t* stats;         // zeroed: [0] RLE runs walked, [1] bit-packed runs, [2] null rows, [3] Utf8: bytes of all rows (64-bit sum)
};
// The inflate stage of a compressed chunk (k_pq_inflate), run before the kernels above: every page of `pages` (the host's header
// pass checked every extent: dfx_parquet_lz4.hpp) is inflated or copied from `chunk` into `image`, which DevPqColumn::chunk then names.
struct DevPqInflate {
  const uint8_t* chunk;        // the chunk as the file holds it
  uint8_t* image;              // the inflated image, zeroed: a page whose block is malformed keeps zeros from the bad sequence on
  const PqInflatePage* pages;
  uint32_t n_pages;
  PqPrologue* prologues;       // n_pages: what the host's body pass reads of each inflated page
  uint32_t* ctrl;              // CTRL_WORDS words: PQ_ERR_INFLATE is ORed into CTRL_ERROR
  uint64_t* stats;             // zeroed: [0] sequences parsed
};
hipError_t launch_pq_inflate(const DevPqInflate& I, double image_bytes, hipStream_t s);
// out: the values (fixed width, Boolean words); Utf8: out_starts / out_lens, rows entries each (source offsets into the chunk, lengths)
hipError_t launch_pq_decode(const DevPqColumn& C, bool has_rle_bool, bool has_dict, void* out, int32_t* out_starts, int32_t* out_lens,
                            double algo_bytes, hipStream_t s);

// ORDER BY (dfx_k_sort.hip): order-preserving key images, stable LSD radix sort of (image, row) pairs, gathers
hipError_t launch_sort_image(const void* values, const uint8_t* validity, int64_t bit_offset, uint8_t dtype, int asc, int64_t n,
                             uint64_t* image, uint64_t* null_image, hipStream_t s);
// Utf8 key: chunk >= 0: big-endian image of bytes [8 * chunk, 8 * chunk + 8) zero padded; chunk < 0: the length.  max_len (may be
// null): atomicMax of the string lengths
hipError_t launch_sort_image_utf8(const int32_t* offsets, const uint8_t* data, const uint8_t* validity, int64_t bit_offset, int chunk,
                                  int asc, int64_t n, uint64_t* image, uint64_t* null_image, uint32_t* max_len, hipStream_t s);
hipError_t launch_sort_iota(uint32_t* idx, int64_t n, hipStream_t s);
hipError_t launch_sort_gather_u64(const uint64_t* src, const uint32_t* idx, int64_t n, uint64_t* dst, hipStream_t s);
hipError_t launch_radix_hist8(const uint64_t* img, int64_t n, uint64_t* hist /* [8][256], zeroed */, hipStream_t s);
// top-k: histogram of one digit over the elements matching a prefix (radix select), bitmap of img <= threshold
hipError_t launch_select_hist(const uint64_t* img, int64_t n, uint64_t prefix, uint64_t mask, int shift, uint64_t* hist /* [256], zeroed */,
                              hipStream_t s);
hipError_t launch_select_mask(const uint64_t* img, int64_t n, uint64_t threshold, uint64_t* mask_words, uint32_t* tile_counts,
                              hipStream_t s);
int64_t radix_tiles(int64_t n);  // counts / offsets hold 256 * radix_tiles(n) entries, digit-major
hipError_t launch_radix_count(const uint64_t* img, int64_t n, int shift, uint32_t* counts, hipStream_t s);
hipError_t launch_radix_scatter(const uint64_t* img_in, const uint32_t* idx_in, int64_t n, int shift, const uint64_t* offsets,
                                uint64_t* img_out, uint32_t* idx_out, hipStream_t s);
hipError_t launch_sort_locate(const uint32_t* idx, int64_t n, const uint64_t* starts, int nb, uint64_t* loc, hipStream_t s);
hipError_t launch_gather_fixed(const void* const* bases, const uint64_t* loc, int64_t n, int width, void* out, hipStream_t s);
hipError_t launch_gather_bits(const uint8_t* const* bases, const int64_t* bit_offsets, const uint64_t* loc, int64_t n,
                              uint64_t* out, uint64_t* zero_count, hipStream_t s);
hipError_t launch_gather_utf8_lens(const int32_t* const* offsets, const uint64_t* loc, int64_t n, int32_t* lens, hipStream_t s);
hipError_t launch_gather_utf8_copy(const int32_t* const* offsets, const uint8_t* const* data, const uint64_t* loc, int64_t n,
                                   const int32_t* dst_offsets, uint8_t* out, hipStream_t s);

// COUNT(DISTINCT x) (dfx_k_distinct*.hip, deviation D8): distinct sets are DevTables with na == 0 whose key is the tuple
// (group key words, zero padding, canonical argument image); growth and spill replay use launch_rehash / launch_merge_rows.
// insert: rows -> tuples (null arguments skipped, floats canonicalised) -> set, rows it cannot take -> spill; *plan_kernel: the
// scan-plan flavour ran (else the SSA interpreter).  count: ungrouped (S.kw == 1) the tuples into *total, grouped +1 per tuple
// into the count table Cnt (key prefix, one ACC_ADD_U64).  lookup: emitted group keys -> counts (0 when absent).
hipError_t launch_distinct_insert(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevAggPlan& plan, int kw_out,
                                  const DevTable& T, const DevRows& spill, int64_t n, bool* plan_kernel, hipStream_t s);
hipError_t launch_distinct_count(const DevTable& S, const DevTable& Cnt, uint64_t* total, hipStream_t s);
hipError_t launch_distinct_lookup(const DevTable& Cnt, const DevDistinctKeys& K, int kw_out, int64_t n, uint64_t* out, hipStream_t s);

// MIN / MAX of a Utf8 column (dfx_k_utf8agg.hip, deviation D10): folded at emit from the distinct set of (key words, padding,
// dictionary id of the argument).  fold: every tuple of S into the extrema table Ex (the count table's twin: S.kw words, the
// argument word zeroed, two zeroed planes min id + 1 / max id + 1; ungrouped, S.kw == 1: Ex.stride == 1, its one entry), strings
// compared out of D (n_ids: the ids D holds); planes: bit 0 the minimum, bit 1 the maximum.  lookup: emitted group keys -> the ids
// of plane `plane` (null_id where the group has none), the validity words ((n + 63) / 64) and *nulls += null rows.
hipError_t launch_utf8_extrema_fold(const DevTable& S, const DevTable& Ex, const DevDict& D, uint64_t n_ids, uint32_t planes, hipStream_t s);
hipError_t launch_utf8_extrema_lookup(const DevTable& Ex, const DevDistinctKeys& K, int kw_out, int64_t n, int plane, uint64_t null_id,
                                      uint64_t* ids, uint64_t* validity, uint64_t* nulls, hipStream_t s);

// synthetic columns (definition shared with oracle/dfx_oracle.c: orc_synth_fill)
hipError_t launch_synth(int kind, int column_id, double p0, double p1, uint64_t seed, int64_t row_begin,
                        int64_t n, void* out, hipStream_t s);
// validity bitmap of a synthetic column with nulls (DFX_SYNTH_NULL_PERMILLE): (n + 63) / 64 words; *nulls += null rows
hipError_t launch_synth_validity(int column_id, uint32_t permille, uint64_t seed, int64_t row_begin, int64_t n, uint64_t* words,
                                 uint64_t* nulls, hipStream_t s);

// host mirror of the device hash (rank ownership in tests)
uint64_t host_hash_keys(const uint64_t* key, int kw);
uint32_t host_unhash_word32(uint32_t image);

}  // namespace dfx
