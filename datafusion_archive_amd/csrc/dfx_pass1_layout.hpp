// dfx_pass1_layout.hpp -- pass 1 of the partitioned GROUP BY: its LDS arithmetic, THE list of routed layouts and which one a
// table takes.  choose_routed_layout is everything AggregateRelation::Impl::ensure_partition (dfx_aggregate_launch.cpp) decides
// before it allocates: the flavour that routes the rows or a refusal, the row form, the region geometry, strides and capacities.
// select_pass1 (dfx_k_partition.hip) and choose_pass2 (dfx_pass2_forms.hpp) take its DevPartition as their input.  A new layout
// is one name here and its branch in choose_routed_layout.
// Host only and free of HIP: tests/native/pass1_layout_check.cpp holds it against tables written out by hand.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "dfx_device.hpp"

namespace dfx {

// ---- the LDS arithmetic of pass 1 (the kernels carve their dynamic LDS by the same constants) ----------------------------------
constexpr int ring_queue_rows(int rp) { return rp == 16 ? 192 : 128; }  // (32- and 30-row rings: 96 KB of ring, 128-row queues)  // (32-row rings: 16-row chunks of 12-byte rows need the LDS)
constexpr int kRingBlock = 1024;
constexpr int kHotSlots = 1024;        // hot-key pairs per pass-1 workgroup, 16-byte rows
constexpr int kHotSlotsNarrow = 2048;  // ... with 12-byte rows (the ring is 16 KB smaller)
constexpr int kSortMaxCap = 8192;  // LDS buffer rows (upper bound: 13-bit row index in the permutation word)
constexpr int kWsQueueRows = 256;  // per scanner wave (power of two): 3 KB {u32 key, u64 operand}; PTF_ROW8: 2 KB {u32 key, u32 Float32 bits}
constexpr int kWsCH = kNarrowChunkRows, kWsRP = kNarrowRingRows, kWsNCH = kWsRP / kWsCH;  // (dfx_device.hpp: LINE chunks of ten rows, three slots)

struct WsCtl {  // one per queue (= per router wave)
  uint32_t tail;  // rows produced (written by the queue's scanner)
  uint32_t head;  // rows consumed (written by its router)
  uint32_t done;  // the scanner has published its last row
  uint32_t pad;
};

// LDS of the ring kernels (k_partition_ring): kRingRP ring rows per partition
inline size_t partition_ring_bytes(uint32_t n_words, uint32_t n_parts, int kRingRP, bool hot = false, bool narrow = false, int queue_rows = 0) {
  const int kRingQ = queue_rows > 0 ? queue_rows : ring_queue_rows(kRingRP);
  const size_t ring = (narrow && kNarrowLine && kRingRP == kNarrowRingRows) ? (size_t)n_parts * kNarrowRingSlots * kNarrowSlotBytes
                                                                            : (size_t)n_parts * kRingRP * (narrow ? 12 : n_words * 8);
  return ring + (size_t)(kRingBlock / 64) * kRingQ * n_words * 8 +
         (size_t)(kRingBlock / 64) * 64 * (kRingRP >= 16 ? 8 : 4) + (size_t)n_parts * 4 * (1 + 2 * 4) + 64 +
         (hot ? (size_t)(narrow ? kHotSlotsNarrow : kHotSlots) * 16 : 0);
}

// LDS of the wave-specialised pass-1 kernel (PTF_WS)
// row8 (PTF_ROW8): the queues' operand plane holds 4-byte words; the ring is three 128-byte slots per partition either way
inline size_t partition_ws_bytes(uint32_t n_parts, int ns, int nv = 1, bool row8 = false) {  // nv: routed operands per row (2: PTF_PAIR -- a second operand plane per queue)
  const int nq = kRingBlock / 64 - ns;  // one queue per ROUTER wave (a scanner feeds (16 - ns) / ns of them in turn)
  return (size_t)n_parts * kNarrowRingSlots * kNarrowSlotBytes + (size_t)(kRingBlock / 64) * 64 * 8 /* jobs */ + (size_t)n_parts * 4 * (1 + 2 * kWsNCH) +
         (size_t)nq * kWsQueueRows * (4 + (row8 ? 4 : 8 * (size_t)nv)) + (size_t)nq * sizeof(WsCtl) + 64;
}

// LDS rows of the write-combining buffer for a workgroup of `block` lanes and an LDS budget
inline uint32_t partition_sort_capacity(uint32_t n_words, uint32_t n_parts, uint32_t block, size_t lds_budget) {
  const size_t fixed = (size_t)n_parts * 12 + (2 + 16) * 4 + 16;
  if (lds_budget <= fixed) return 0;
  size_t cap = (lds_budget - fixed) / ((size_t)n_words * 8 + 4);
  cap = cap / block * block;
  if (cap > (size_t)kSortMaxCap) cap = kSortMaxCap;
  return (uint32_t)cap;
}

// dynamic LDS of the pass-1 launch of this layout
inline size_t partition_stage_bytes(const DevPartition& PT) {
  if ((PT.mode & 15u) == 0) return (size_t)PT.n_parts * 4 + 16;
  if ((PT.mode & 15u) == 2 && (PT.flags & PTF_WS)) return partition_ws_bytes(PT.n_parts, PT.ws_scanners == 4 ? 4 : 8, (PT.flags & PTF_PAIR) ? 2 : 1, (PT.flags & PTF_ROW8) != 0);
  if ((PT.mode & 15u) == 2)
    return partition_ring_bytes(PT.n_words, PT.n_parts, (PT.flags & PTF_CHUNK16) ? kNarrowRingRows : (PT.mode & 0x100u) ? 8 : 16, (PT.flags & PTF_HOT) != 0,
                                (PT.flags & PTF_NARROW) != 0, (PT.flags & PTF_SHARED) ? 128 : 0);
  return (size_t)PT.stage_rows * ((size_t)PT.n_words * 8 + 4) + (size_t)PT.n_parts * 12 + (2 + 16) * 4 + 16;
}

constexpr size_t kPass1LdsLimit = 160 * 1024;  // what launch_partition accepts: the LDS of a CU, one workgroup on it
// What the host gives the ring flavours: 2 KB below the launch's limit, because the byte counts above are the DYNAMIC LDS alone --
// the kernels' static LDS (publish_max_fill's word) and the padding of the arrays they carve out of it come on top.
constexpr size_t kPass1LdsBudget = 158 * 1024;
constexpr uint32_t kPass1MaxParts = 4096;

// Does launch_partition take this layout?  (false: hipErrorInvalidValue)
inline bool partition_launchable(const DevPartition& PT) {
  const size_t lds_bytes = partition_stage_bytes(PT);
  const uint32_t mode = PT.mode & 15u;
  if (mode == 0) return lds_bytes <= 65536;
  if (mode == 2) return lds_bytes <= kPass1LdsLimit;
  if (mode == 1)
    return lds_bytes <= kPass1LdsLimit && PT.stage_rows != 0 && PT.stage_rows <= (uint32_t)kSortMaxCap && PT.n_parts <= kPass1MaxParts && (PT.block == 512 || PT.block == 1024);
  return true;
}

// PTF_ROW8 regions hold 8-byte rows of Float32 bits: only a wave-specialised one-value launch that binds both shadows (PTF_VAL4)
// writes them.  select_pass1 / launch_partition refuse every other combination (hipErrorInvalidValue).
inline bool partition_row8_consistent(uint32_t flags) {
  if (!(flags & PTF_ROW8)) return true;
  const uint32_t need = PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_KEY4 | PTF_VAL4;
  return kNarrowLine && (flags & need) == need && !(flags & (PTF_SHARED | PTF_PAIR | PTF_PLANES | PTF_HOT));
}

// ---- the routed layouts ---------------------------------------------------------------------------------------------------------
// shared_ring: 16-row rings of {image, raw operand} rows, 2..3 aggregates of one operand (PTF_SHARED); planes: the same rows through
// the wave-specialised kernel, one pass 2 per accumulator plane (PTF_PLANES); pair_rows: 20-byte rows of two operands (PTF_PAIR);
// ring16: the 16-row ring family -- hot-key pairs (PTF_HOT), large chunks (PTF_CHUNK16) and wave specialisation (PTF_WS) are
// properties of it, and so is the 8-byte row of two shadows (PTF_ROW8); ring8: 8-row rings for rows of three and more words; sort: the LDS counting sort; direct: a store per row.
enum class RoutedLayoutKind : int { refused_pair_scan = -2, refused_table_blocks = -1, shared_ring, planes, pair_rows, ring16, ring8, sort, direct };
constexpr const char* kRoutedLayoutName[] = {"shared_ring", "planes", "pair_rows", "ring16", "ring8", "sort", "direct"};

// Where the stream stands (AggregateRelation::Impl::Phase): no pair scan; the pair scan over two operands; the pair scan's
// shared-operand flavour (split_is_shared: planes).
enum class PairPhase : int { none, pair, planes };

struct Pass1LayoutOptions {  // AggOptions (dfx_relation.hpp), the values the layout depends on
  int narrow_keys, narrow_chunk16, hot_keys, pass2_stream;
  int pass1_ws, pass1_ws_dense, pass1_ws_dense_scanners;
  int partition_mode, partition_layout, partition_block, partition_producers, partition_defer, partition_cap_rows, partition_pad;
};

struct RoutedLayoutQuery {
  int64_t rows;      // the batch (or launch) the regions are sized for
  bool nulls_now;    // it has nulls
  int kw, na;        // key words; the ACTIVE chunk's aggregates
  uint64_t table_slots, block_slots;  // T.mask + 1, T.block_mask + 1
  int cu_count;
  PairPhase phase;
  int split_distinct;
  uint32_t split_ops, split_arg1;
  bool shared_operand, same_operand_all;  // the active chunk's aggregates take one operand: two or three of them / any number
  bool has_pred, unfused_now;
  bool narrow, dense_seen, mostly_seen, skew_seen;  // StrategyDecision
  Pass1LayoutOptions opt;
  // every launch sized by this layout will bind both column shadows (PTF_VAL4): the one-value wave-specialised layout then routes
  // 8-byte rows (PTF_ROW8).  false: the layout as it is without the form
  bool both_shadows = false;
};

struct RoutedLayout {
  RoutedLayoutKind kind = RoutedLayoutKind::refused_pair_scan;
  DevPartition PT = {};  // every field that is not a pointer (refused_table_blocks: n_parts, n_words and part_shift alone)
  // PTF_NARROW | PTF_SHARED | PTF_PAIR | PTF_PLANES as the query WANTS them (and PTF_ROW8 as the layout HAS it): what ensure_partition compares the layout in use with
  // ("same table, keep appending").  An oddity, kept: PTF_NARROW is wanted for every narrow one-value query, but only the ring
  // family's 12-byte rows set it -- under ring8, sort, direct and agg.partition_mode = 2 | 0x80 such a query never finds its own
  // layout "the same" and lays the regions out again (a pass 2) with every batch.
  uint32_t want_flags = 0;
  uint32_t worst = 0;    // Pass2Window::worst
  size_t row_bytes = 0;  // of DevPartition::rows
  size_t cnt_bytes = 0;  // of DevPartition::counts
};

// The option preconditions and the LDS test that pair rows and planes share: whole-line chunks through the wave-specialised
// kernel -- 8 scanners and two operand planes per queue, or (planes) the dense split's 4 scanners whatever ws_scanners ends up as.
inline bool pair_layout_fits(const Pass1LayoutOptions& o, uint32_t n_parts, bool planes) {
  return kNarrowLine && o.narrow_keys != 0 && o.narrow_chunk16 && o.pass1_ws > 0 && o.partition_layout != 2 && ((uint32_t)o.partition_mode & 0x8Fu) == 2u &&
         partition_ws_bytes(n_parts, planes ? 4 : 8, planes ? 1 : 2) <= kPass1LdsBudget;
}

inline RoutedLayout choose_routed_layout(const RoutedLayoutQuery& q) {
  RoutedLayout r;
  DevPartition& PT = r.PT;
  const Pass1LayoutOptions& o = q.opt;
  const uint32_t n_parts = (uint32_t)(q.table_slots / q.block_slots);
  const bool pair_scan = q.phase != PairPhase::none;
  const bool raw_ok = !q.nulls_now || (q.has_pred && !q.unfused_now);  // (a raw operand has no validity: fine under an absorbed predicate -- every surviving slot is valid)
  const bool want_planes = q.phase == PairPhase::planes && q.narrow && raw_ok && q.same_operand_all && pair_layout_fits(o, n_parts, true);
  const bool want_shared = !pair_scan && q.narrow && o.narrow_keys != 0 && !q.nulls_now && q.shared_operand && ((uint32_t)o.partition_mode & 0x8Fu) == 2u &&
                           partition_ring_bytes(2, n_parts, 16, false, true, 128) <= kPass1LdsBudget;
  const bool want_pair = q.phase == PairPhase::pair && q.narrow && q.kw == 1 && q.na >= 2 && q.split_distinct == 2 && (q.na == 2 || raw_ok) && pair_layout_fits(o, n_parts, false);
  if (pair_scan && !want_pair && !want_planes)  // (a table block holds ONE accumulator plane in this mode: no other routed form fits; until the
    return r;                                   // next batch boundary the rows go through the global table)
  const bool want_narrow = q.narrow && q.kw == 1 && (q.na == 1 || want_shared || want_pair || want_planes) && o.narrow_keys != 0;
  r.want_flags = (want_narrow ? PTF_NARROW : 0u) | (want_shared || want_planes ? PTF_SHARED : 0u) | (want_pair ? PTF_PAIR : 0u) | (want_planes || (want_pair && q.na > 2) ? PTF_PLANES : 0u);
  PT.n_parts = n_parts;
  PT.n_words = (want_shared || want_planes) ? 2u : (uint32_t)(q.kw + q.na);
  while ((1ull << PT.part_shift) < q.block_slots) ++PT.part_shift;
  if (PT.n_parts > kPass1MaxParts) {
    r.kind = RoutedLayoutKind::refused_table_blocks;
    return r;
  }
  // pass-1 flavour (agg.partition_mode).  Scattered 16-byte stores are transaction-bound at ~87 G rows/s on
  // MI355X while runs of >= 64 bytes reach > 400 G rows/s (tools/ubench2.hip), so routed rows are write-combined
  // in LDS whenever the partition count allows it:
  //   2 (default)  lock-free per-partition LDS rings, 128-byte chunks, no barrier in the scan loop
  //   1            workgroup-wide LDS counting sort (also for partition counts whose rings do not fit LDS)
  //   0            one 16-byte store per row straight from registers (very many partitions)
  const uint32_t block = o.partition_block == 512 ? 512u : 1024u;
  // (the counting sort's budget: 156 KB; agg.partition_block = 512: two workgroups per CU, 79 KB each)
  const uint32_t sort_cap = partition_sort_capacity(PT.n_words, PT.n_parts, block, block == 512 ? (size_t)79 * 1024 : (size_t)156 * 1024);
  const int want = o.partition_mode & 15;
  const uint32_t mode_bits = (uint32_t)o.partition_mode & ~15u;  // (0x80: 16-byte rows in 4-row chunks, A/B)
  // the split of the wave-specialised kernel: 8 scanners + 8 routers; dense scans (more than two thirds of the rows routed): 4 + 12
  // (agg.pass1_ws_dense_scanners; agg.pass1_ws = 4: that split whatever the selectivity -- tests)
  const uint32_t ws_scanners = (o.pass1_ws == 4 || (q.mostly_seen && o.pass1_ws_dense_scanners == 4)) ? 4u : 8u;
  // what the five ring layouts share: one producer workgroup of 1024 lanes per CU (agg.partition_producers: that many), no staging rows
  const uint32_t per_cu = (uint32_t)std::min(1024, q.cu_count);
  PT.mode = 2u;
  PT.block = 1024;
  PT.stage_rows = 0;
  PT.n_producers = o.partition_producers > 0 ? (uint32_t)std::min(1024, o.partition_producers) : per_cu;
  if (want_shared) {
    r.kind = RoutedLayoutKind::shared_ring;
    PT.flags |= PTF_NARROW | PTF_SHARED;
  } else if (want_planes) {
    r.kind = RoutedLayoutKind::planes;
    PT.flags |= PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_SHARED | PTF_PLANES;
    PT.ws_scanners = ws_scanners;  // (as for one aggregate)
  } else if (want_pair) {
    r.kind = RoutedLayoutKind::pair_rows;
    PT.flags |= PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_PAIR;
    if (q.na > 2) PT.flags |= PTF_PLANES;  // raw operands, a transform per accumulator in pass 2
    PT.pair_ops = q.split_ops;
    PT.pair_arg1 = q.split_arg1;
    PT.ws_scanners = 8u;
  } else if (want == 2 && partition_ring_bytes(PT.n_words, PT.n_parts, 16) <= kPass1LdsBudget) {
    r.kind = RoutedLayoutKind::ring16;
    const bool hot = o.hot_keys > 0 || (o.hot_keys < 0 && q.skew_seen);
    const bool chunks8 = !(mode_bits & 0x80u);
    if (want_narrow && chunks8) PT.flags |= PTF_NARROW;
    if (hot && q.na == 1 && chunks8 && partition_ring_bytes(PT.n_words, PT.n_parts, 16, true, (PT.flags & PTF_NARROW) != 0) <= kPass1LdsBudget)
      PT.flags |= PTF_HOT;
    if ((PT.flags & PTF_NARROW) && !(PT.flags & PTF_HOT) && o.narrow_chunk16 && !(kNarrowLine && o.partition_layout == 2) /* LINE chunks: contiguous regions */ &&
        partition_ring_bytes(PT.n_words, PT.n_parts, kNarrowRingRows, false, true) <= kPass1LdsBudget)
      PT.flags |= PTF_CHUNK16;
    // selective scans: the scanning and the routing belong to different waves (dfx_k_partition_ws_inl.hpp).  When most rows
    // pass, every wave has rows to route all the time and the ring kernel's symmetric waves are the better fit
    // (round 5, 2^26-row launches, us per launch: ring kernel / 8 + 8 waves / 4 + 12 waves -- selectivity 0.2: - / 415 / 535; 0.5: 326 /
    // 261 / 292; 0.8: 403 / 371 / 353; every row routed: 434 / 438 / 417-424 -- profiles/r05_pass1_ws_by_selectivity.txt.  So: always
    // the wave-specialised kernel, four scanners once more than two thirds of the rows are routed.  agg.pass1_ws_dense = -1: never
    // above one half, round 4's rule)
    const bool ws_fits = o.pass1_ws_dense >= 0 || !q.dense_seen;
    if ((PT.flags & PTF_CHUNK16) && o.pass1_ws > 0 && ws_fits && !mode_bits) {
      PT.ws_scanners = ws_scanners;  // (an oddity, kept: it stays set when the kernel's LDS does not fit and PTF_WS is not)
      if (partition_ws_bytes(PT.n_parts, (int)PT.ws_scanners) <= kPass1LdsBudget) PT.flags |= PTF_WS;
    }
    // both shadows bound by every launch: {image, Float32 bits}, sixteen rows per line (the operand's 4 shadow bytes ARE the operand)
    if (q.both_shadows && kNarrowLine && (PT.flags & PTF_WS) && q.na == 1 && q.kw == 1) {
      PT.flags |= PTF_ROW8;
      r.want_flags |= PTF_ROW8;
    }
    PT.mode = 2u | mode_bits;
  } else if (want == 2 && partition_ring_bytes(PT.n_words, PT.n_parts, 8) <= kPass1LdsBudget) {
    // several aggregates: rows of 3+ words.  8-row rings (two 4-row chunks) still fit where 16-row ones do not
    // (an oddity, kept: so they do for two-word rows at 512 table blocks -- 120896 bytes --, ahead of the counting sort)
    r.kind = RoutedLayoutKind::ring8;
    PT.mode = 2u | 0x100u;
  } else if (want != 0 && PT.n_parts <= 1024 && sort_cap >= 4 * PT.n_parts) {
    r.kind = RoutedLayoutKind::sort;
    PT.mode = 1u | mode_bits;
    PT.block = block;
    PT.stage_rows = sort_cap;
    PT.n_producers = (uint32_t)std::min(1024, q.cu_count * (int)(1024 / block));  // (agg.partition_producers: the ring layouts only)
  } else {
    // one producer workgroup (1024 lanes) per CU: producers x partitions x 128 B of open region lines
    r.kind = RoutedLayoutKind::direct;
    PT.mode = 0;
    PT.n_producers = per_cu;
  }
  const uint64_t avg = (uint64_t)q.rows / ((uint64_t)PT.n_producers * PT.n_parts) + 1;
  // capacities are whole 64-row trips; LINE chunks (ten rows per 128-byte line, PTF_CHUNK16): whole lines as well
  const bool pair_rows = (PT.flags & PTF_PAIR) != 0;                  // a region is cap_rows / 6 lines of 128 bytes
  const bool line_chunks = (PT.flags & PTF_CHUNK16) && kNarrowLine;  // ... cap_rows / 10 lines
  const bool row8 = (PT.flags & PTF_ROW8) != 0;                       // ... cap_rows / 16 lines, no padding: cap_rows * 8 bytes
  const uint64_t capq = pair_rows ? (uint64_t)kPairCapQuantum : row8 ? (uint64_t)kRow8CapQuantum : line_chunks ? (uint64_t)kNarrowCapQuantum : 64ull;
  r.worst = (uint32_t)((2 * avg + 64 + capq - 1) / capq * capq);
  // regions hold `window` worst-case batches.  Deferral pays when few rows are routed (headline, 20 %: 2 batches per
  // pass 2 = -3 % per query); when most rows are, the twice-as-long regions cost pass 1 more than the saved launches
  // give back (config 3, 1e9 rows: 11.05 ms at 2, 10.08 ms at 1)
  int window = o.partition_defer > 0 ? std::min(o.partition_defer, 16) : (int)std::max<int64_t>(1, std::min<int64_t>(8, ((int64_t)1 << 27) / std::max<int64_t>(q.rows, 1)));
  if (q.dense_seen) window = 1;
  PT.cap_rows = r.worst * (uint32_t)window;
  if (o.partition_cap_rows > 0) {  // tests: tiny regions (overflow -> spill list); no deferral
    PT.cap_rows = (uint32_t)(((uint64_t)o.partition_cap_rows + capq - 1) / capq * capq);
    r.worst = PT.cap_rows;
  }
  if (o.pass2_stream && q.na == 1 && q.kw == 1) PT.flags |= PTF_STREAM_PASS2;
  uint64_t pad_words = (uint64_t)(o.partition_pad >= 0 ? o.partition_pad : 0) / 8;
  if (line_chunks) pad_words = (pad_words + 15) / 16 * 16;  // (every region starts on a 128-byte line)
  const uint64_t region_words = pair_rows ? (uint64_t)(PT.cap_rows / (uint32_t)kPairChunkRows) * 16u
                                : row8 ? (uint64_t)PT.cap_rows * (4u * kRow8Dwords) / 8
                                : line_chunks ? (uint64_t)(PT.cap_rows / (uint32_t)kNarrowChunkRows) * (kNarrowSlotBytes / 8)
                                : (PT.flags & PTF_NARROW) ? (uint64_t)PT.cap_rows * 12 / 8 : (uint64_t)PT.cap_rows * PT.n_words;
  // one pass-2 trip's worth (64 contiguous rows, or six LINE chunks = 60 rows: 768 bytes either way): regions are contiguous (layouts 0 and 1)
  PT.win_stride = pair_rows ? (uint64_t)(kPairTripBytes / 8u) : row8 ? (uint64_t)(kRow8TripBytes / 8u) : line_chunks ? 96u : region_words / (PT.cap_rows / 64);
  uint64_t row_words;
  if (o.partition_layout == 2) {  // windowed: window w of every partition of a producer side by side
    PT.part_stride = PT.win_stride;
    PT.win_stride = (uint64_t)PT.n_parts * PT.part_stride;
    PT.prod_stride = (uint64_t)(PT.cap_rows / 64) * PT.win_stride + pad_words;
    row_words = (uint64_t)PT.n_producers * PT.prod_stride;
  } else if (o.partition_layout == 0) {  // partition-major (round 1)
    PT.prod_stride = region_words;
    PT.part_stride = (uint64_t)PT.n_producers * PT.prod_stride + pad_words;
    row_words = (uint64_t)PT.n_parts * PT.part_stride;
  } else {  // producer-major
    PT.part_stride = region_words;
    PT.prod_stride = (uint64_t)PT.n_parts * PT.part_stride + pad_words;
    row_words = (uint64_t)PT.n_producers * PT.prod_stride;
  }
  r.row_bytes = sizeof(uint64_t) * (size_t)row_words;
  r.cnt_bytes = sizeof(uint32_t) * (size_t)PT.n_parts * PT.n_producers;
  return r;
}

}  // namespace dfx
